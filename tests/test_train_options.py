"""The target options' state is one plain struct (simple_dqn_amd/csrc/train_options.h).  tests/emul/train_options.cpp includes
the header and prints its defaults and, for a handful of settings, the derived predicates and the output arithmetic; here the defaults are
held to the values the C ABI documents (and, on a device, to the getters of a fresh handle on both train paths), and the arithmetic to
DeepQNetwork's `_net_actions`: bootstrap_heads x quantiles x num_actions outputs, num_actions + 1 for a dueling net.
Every test here builds that program, so none of them runs on a tree without the header: they hold the header to the documented values.
What pins the library's behaviour against an older build of it is tests/test_gpu_option_state.py, which needs only the C ABI."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import make_args  # noqa: E402

GAME_ACTIONS = 4            # what train_options.cpp prints its arithmetic for
# setting -> (bootstrap_heads, quantiles, dueling) and the predicates that are true under it
CASES = {
    "off": ((1, 1, False), ()),
    "double_dqn": ((1, 1, False), ()),
    "n_step": ((1, 1, False), ()),
    "munchausen": ((1, 1, False), ("prestate_target_forward",)),
    "advantage_learning": ((1, 1, False), ("advantage_on", "prestate_target_forward")),
    "persistent_advantage": ((1, 1, False), ("advantage_on", "prestate_target_forward")),
    "cql_alpha": ((1, 1, False), ("cql_on",)),
    "bootstrap_heads": ((3, 1, False), ("bootstrap_on",)),
    "quantiles": ((1, 2, False), ("quantiles_on",)),
    "dueling": ((1, 1, True), ()),
}
PREDICATES = ("advantage_on", "cql_on", "bootstrap_on", "quantiles_on", "prestate_target_forward")
# include/sdqn.h: the values a network has before any setter ran
DEFAULTS = {"double_dqn": 0, "n_step": 1, "munchausen": 0, "mu_alpha": 0.9, "mu_tau": 0.03, "mu_clip": -1.0, "al_alpha": 0.0, "al_persistent": 0,
            "cql_alpha": 0.0, "boot_K": 1, "boot_P": 1.0, "boot_seed": 0, "boot_thresh": 1 << 53, "quant_N": 1, "dueling": 0}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_options") / "train_options")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "emul", "train_options.cpp")])
    rows = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        words = line.split()
        name = words[0] if words[0] == "default" else words[1]
        rows[name] = dict(w.split("=") for w in words[(1 if words[0] == "default" else 2):])
    return rows


def _net_actions(num_actions, bootstrap_heads, quantiles, dueling):
    """DeepQNetwork.__init__'s arithmetic"""
    return num_actions + 1 if dueling else bootstrap_heads * quantiles * num_actions


def test_defaults(printed):
    d = printed["default"]
    assert set(d) == set(DEFAULTS) | {"gamma_n"}
    for k, v in DEFAULTS.items():
        assert (float(d[k]) if isinstance(v, float) else int(d[k])) == v, (k, d[k])


def test_predicates_and_output_arithmetic(printed):
    assert set(printed) == set(CASES) | {"default"}
    for name, ((K, N, dueling), true) in CASES.items():
        row = printed[name]
        for p in PREDICATES:
            assert int(row[p]) == (1 if p in true else 0), (name, p)
        assert int(row["multiplier"]) == K * N, name
        assert int(row["outputs"]) == _net_actions(GAME_ACTIONS, K, N, dueling), name
        assert int(row["game_actions"]) == GAME_ACTIONS, name


def test_header_is_plain_cpp():
    text = open(os.path.join(HERE, "..", "simple_dqn_amd", "csrc", "train_options.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True], ids=["tuned", "generic"])
def test_a_fresh_handle_reports_the_defaults(printed, generic):
    import simple_dqn_amd as sd
    lib, d = sd.load(), printed["default"]
    kw = dict(screen_height=36, screen_width=36, history_length=2, datatype="float64") if generic else {}
    net = sd.DeepQNetwork(3, make_args(batch_size=4, **kw))

    def get(fn, *types):
        out = [t() for t in types]
        assert getattr(lib, fn)(net._h, *[C.byref(o) for o in out]) == 0
        return [o.value for o in out]
    assert get("sdqn_net_get_munchausen", C.c_int, C.c_double, C.c_double, C.c_double) == [int(d["munchausen"]), float(d["mu_alpha"]), float(d["mu_tau"]), float(d["mu_clip"])]
    assert get("sdqn_net_get_advantage_learning", C.c_double, C.c_int) == [float(d["al_alpha"]), int(d["al_persistent"])]
    assert get("sdqn_net_get_cql", C.c_double) == [float(d["cql_alpha"])]
    assert get("sdqn_net_get_bootstrap", C.c_int, C.c_double, C.c_uint64) == [int(d["boot_K"]), float(d["boot_P"]), int(d["boot_seed"])]
    assert get("sdqn_net_get_quantiles", C.c_int) == [int(d["quant_N"])]
    assert get("sdqn_net_get_dueling", C.c_int) == [int(d["dueling"])]
