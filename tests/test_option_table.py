"""Which training options combine, without a device: the command line's refusals pair by pair against the outcomes and
words recorded before the refusals became a table (tests/golden/option_conflicts_cli.json), deepqnetwork.CONFLICTS against the library's
table (csrc/option_table.h through sdqn_option_name / sdqn_option_conflict), and the library's words against the ones its setters
spoke on the device before the change (tests/golden/option_conflicts_lib.json)."""
import ctypes as C
import itertools
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN_CLI = os.path.join(HERE, "golden", "option_conflicts_cli.json")
GOLDEN_LIB = os.path.join(HERE, "golden", "option_conflicts_lib.json")

# the 14 flags and the words that switch each on
FLAGS = {"double_dqn": ["--double_dqn", "true"], "munchausen": ["--munchausen", "true"], "advantage_learning": ["--advantage_learning", "0.5"],
         "cql_alpha": ["--cql_alpha", "1.0"], "bootstrap_heads": ["--bootstrap_heads", "2"], "quantiles": ["--quantiles", "2"],
         "dueling": ["--dueling", "true"], "noisy_nets": ["--noisy_nets", "true"], "batch_norm": ["--batch_norm", "true"],
         "clip_grad_norm": ["--clip_grad_norm", "5"], "target_tau": ["--target_tau", "0.1"], "random_shift": ["--random_shift", "4"],
         "prioritized_replay": ["--prioritized_replay", "true"], "n_step": ["--n_step", "3"]}


class DeviceTouched(Exception):
    pass


def cli_outcome(main, _lib, words):
    """main.run on these words with the library out of reach: the ValueError's text, or None when the run gets as far as the device"""
    def boom(*a, **k):
        raise DeviceTouched()
    saved = _lib.load, _lib.bind_device
    _lib.load = _lib.bind_device = boom
    try:
        main.run(main.build_parser().parse_args(words + ["--random_steps", "0", "--epochs", "0"]))
    except ValueError as e:
        return str(e)
    except DeviceTouched:
        return None
    finally:
        _lib.load, _lib.bind_device = saved
    raise AssertionError("main.run came back without the library: %r" % (words,))


def record_cli(main, _lib):
    """every unordered pair of FLAGS, the words in the order of FLAGS: what tests/golden/option_conflicts_cli.json holds"""
    return [{"flags": [a, b], "message": cli_outcome(main, _lib, FLAGS[a] + FLAGS[b])} for a, b in itertools.combinations(FLAGS, 2)]


def test_command_line_refuses_what_it_refused_in_the_same_words():
    from simple_dqn_amd import _lib, main
    golden = json.load(open(GOLDEN_CLI))
    assert [tuple(g["flags"]) for g in golden] == list(itertools.combinations(FLAGS, 2)) and len(golden) == 91
    assert sum(g["message"] is not None for g in golden) == 39
    for g in golden:
        a, b = g["flags"]
        assert cli_outcome(main, _lib, FLAGS[a] + FLAGS[b]) == g["message"], (a, b)
        back = cli_outcome(main, _lib, FLAGS[b] + FLAGS[a])                    # the other way round on the command line
        assert (back is None) == (g["message"] is None), (b, a, back)
        if back is not None:
            assert "--" + a in back and "--" + b in back, (b, a, back)


def _library_table():
    import simple_dqn_amd as sd
    lib = sd.load()
    names = []
    while lib.sdqn_option_name(len(names)) is not None:
        names.append(lib.sdqn_option_name(len(names)).decode())
    assert lib.sdqn_option_name(-1) is None and lib.sdqn_option_name(len(names) + 1) is None
    words = {}
    buf = C.create_string_buffer(256)
    for i, j in itertools.product(range(len(names)), repeat=2):
        rc = lib.sdqn_option_conflict(i, j, 2, 2, buf, len(buf))
        assert rc in (0, 1), (names[i], names[j], rc)
        assert (buf.value != b"") == (rc == 1)
        if rc:
            words[names[i], names[j]] = buf.value.decode()
    assert lib.sdqn_option_conflict(0, len(names), 0, 0, None, 0) < 0 and lib.sdqn_option_conflict(-1, 0, 0, 0, None, 0) < 0
    return names, words


def test_python_table_is_the_library_table():
    from simple_dqn_amd.deepqnetwork import CONFLICTS
    names, words = _library_table()
    assert names == ["double_dqn", "munchausen", "advantage_learning", "cql_alpha", "bootstrap_heads", "quantiles", "dueling", "noisy_nets",
                     "batch_norm", "clip_grad_norm", "target_tau"]
    assert all((b, a) in words for a, b in words) and not any(a == b for a, b in words)          # symmetric, nothing with itself
    lib_pairs = {frozenset(k) for k in words}
    py_pairs = {frozenset(r[:2]) for r in CONFLICTS if r[0] in names and r[1] in names}
    assert lib_pairs == py_pairs, (lib_pairs ^ py_pairs)
    assert len(lib_pairs) == 36
    for (a, b), text in words.items():
        value = {"bootstrap_heads": " 2", "quantiles": " 2"}
        assert text.startswith("%s%s cannot be combined with %s%s" % (a, value.get(a, ""), b, value.get(b, ""))), text
    for first, second, message in CONFLICTS:                                    # every row's message names both flags with --
        assert "--" + first in message and (second == "geometry" or "--" + second in message), message


def test_library_words_are_the_recorded_ones():
    """what sdqn_option_conflict formats is what the setters said on the device before the change (values 2, as recorded)"""
    _, words = _library_table()
    golden = [g for g in json.load(open(GOLDEN_LIB)) if g["message"] is not None]
    assert {(g["second"], g["first"]) for g in golden} <= set(words)            # (the setter of `second` was refused with `first` on)
    for g in golden:
        assert words[g["second"], g["first"]] == g["message"], g
    settable = {k for k in words if k[0] != "batch_norm"}                      # batch_norm is a property of the network: no setter
    assert {(g["second"], g["first"]) for g in golden} == settable


def test_feature_reasons_are_the_library_ones():
    """--redo_interval, --reset_interval and --weight_decay / --l2_init refuse properties of the net, so they are rows of their own
    (csrc/option_table.h: FEATURES): the reason deepqnetwork.py gives beside --batch_norm and --noisy_nets is the one in the library's line of
    the recorded trace (tests/golden/step_trace_events.txt)"""
    import argparse
    from simple_dqn_amd import deepqnetwork as D
    trace = open(os.path.join(HERE, "golden", "step_trace_events.txt")).read().splitlines()
    cases = ((D.check_redo, dict(redo_interval=5), "redo_interval"), (D.check_reset, dict(reset_interval=5), "reset_interval"),
             (D.check_regularizer, dict(weight_decay=0.1), "weight_decay"), (D.check_regularizer, dict(l2_init=0.01), "l2_init"))
    for check, on, flag in cases:
        for prop in ("batch_norm", "noisy_nets"):
            try:
                check(argparse.Namespace(**dict(on, **{prop: True})))
                said = None
            except ValueError as e:
                said = str(e)
            assert said is not None and said.startswith("--%s " % flag) and " cannot be combined with --%s: " % prop in said, (flag, prop, said)
            lines = [l for l in trace if l.startswith("  ERROR %s cannot be combined with %s: " % (flag, prop))]
            assert len(lines) == 1, (flag, prop)
            assert said.split(": ", 1)[1] == lines[0].split(": ", 1)[1], (flag, prop)


def test_symbols_in_signatures_header_and_library():
    import simple_dqn_amd as sd
    from simple_dqn_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in ("sdqn_option_name", "sdqn_option_conflict"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name), name
        assert name + "(" in header, name
