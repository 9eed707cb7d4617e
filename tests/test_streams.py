"""The counter-based generator and the net layout (csrc/stream.h, csrc/net_layout.h) without a device, held to known answers.
tests/golden/stream_kat.json was recorded from the library BEFORE the two headers existed (its "recorded_from" names the commit), through
the entry points that restate each stream on the host: every case is [entry point, arguments, result], words as integers, floats by their
bit patterns.  Three checks:
  * the library gives the recorded results, bit for bit;
  * tests/emul/streams.cpp, a host program that includes hd.h, stream.h and net_layout.h and nothing else of the project, writes each
    derivation out of the headers' functions and gives the recorded results too: the headers stand alone, and they are the whole formula;
  * layer_of, layer_first and init_bound agree with layer_shapes() and sqrt(3 / fan_in) computed here.
`python tests/test_streams.py --record` prints a new golden file from the library SDQN_LIB_PATH names (that is how the file was made)."""
import ctypes as C
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "golden", "stream_kat.json")

SEEDS = [0, 1, 2 ** 64 - 1]
COUNTS = [0, 1, 2 ** 32]                       # step and event numbers
# the flat weight buffer's layer boundaries, written out (csrc/net_layout.h must agree with these, not the other way round)
OFF = [0, 256 * 32, 256 * 32 + 512 * 64, 256 * 32 + 512 * 64 + 576 * 64, 256 * 32 + 512 * 64 + 576 * 64 + 3136 * 512]
END = OFF[4] + 512 * 18
EDGES = [0, OFF[1] - 1, OFF[1], OFF[2] - 1, OFF[2], OFF[3] - 1, OFF[3], OFF[4] - 1, OFF[4], END - 1]
GAMES = {"catch": "sdqn_env_get_state", "breakout": "sdqn_env_get_state_breakout", "freeway": "sdqn_env_get_state_freeway"}


def layer_of(i):
    return 1 + sum(i >= o for o in OFF[1:])


def cases():
    out = []
    for seed in SEEDS:
        for c in COUNTS:
            for slot in (0, 1):
                for layer in (0, 1):
                    for side in (0, 1):
                        out.append(["sdqn_noisy_words", [seed, c, slot, layer, side, 3]])
            for i in EDGES:
                out.append(["sdqn_redo_draw", [seed, c, i, min(layer_of(i), 4)]])
                out.append(["sdqn_reset_draw", [seed, c, i, layer_of(i)]])
            for L in (1, 2, 3, 4, 5):
                if L < 5:
                    out.append(["sdqn_redo_draw", [seed, c, 7, L]])
                out.append(["sdqn_reset_draw", [seed, c, 7, L]])
            for n in (0, 1, 31):
                for s in (0, 1):
                    for P in (1, 8):
                        out.append(["sdqn_random_shift_draw", [seed, c, n, s, P]])
            for K in (2, 18):
                for P in (0.5, 1.0):
                    out.append(["sdqn_bootstrap_mask", [seed, P, K, c]])
                for episode in COUNTS:
                    out.append(["sdqn_bootstrap_head_of", [seed, K, c, episode]])
        for game in GAMES:
            out.append(["env", [game, seed, 24]])
    return out


def evaluate(lib, fn, a):
    from simple_dqn_amd._lib import check
    if fn == "sdqn_noisy_words":
        w = (C.c_uint64 * a[5])()
        check(lib.sdqn_noisy_words(*a, w))
        return list(w)
    if fn in ("sdqn_redo_draw", "sdqn_reset_draw"):
        w, v = C.c_uint64(), C.c_float()
        check(getattr(lib, fn)(*a, C.byref(w), C.byref(v)))
        return [w.value, struct.unpack("<I", struct.pack("<f", v.value))[0]]
    if fn == "sdqn_random_shift_draw":
        dy, dx = C.c_int(), C.c_int()
        check(lib.sdqn_random_shift_draw(*a, C.byref(dy), C.byref(dx)))
        return [dy.value, dx.value]
    if fn == "sdqn_bootstrap_mask":
        m = (C.c_uint8 * a[2])()
        check(lib.sdqn_bootstrap_mask(*a, m))
        return list(m)
    if fn == "sdqn_bootstrap_head_of":
        k = C.c_int()
        check(lib.sdqn_bootstrap_head_of(*a, C.byref(k)))
        return [k.value]
    # a freshly created game (12 x 12 pixels, episodes of 3): its state and sticky generator, then `steps` agent steps under frame_skip 2
    # and sticky actions (p = 0.25), the action cycling, restarted at every terminal: [reward, terminal, sticky generator, state words]
    game, seed, steps = a
    from simple_dqn_amd import _lib as L
    st = {"catch": L.EnvState, "breakout": L.EnvStateBreakout, "freeway": L.EnvStateFreeway}[game]()
    words = lambda: list(struct.unpack("<%dI" % (C.sizeof(st) // 4), bytes(st)))
    h, n, sticky, r, t = C.c_void_p(), C.c_int(), C.c_uint64(), C.c_int(), C.c_int()
    check(lib.sdqn_env_create(C.byref(h), game.encode(), 12, 12, seed, 3))
    try:
        check(lib.sdqn_env_num_actions(h, C.byref(n)))
        check(lib.sdqn_env_set_dynamics(h, 2, 0.25))
        rows = []
        for k in range(steps + 1):
            if k:
                check(lib.sdqn_env_step(h, k % n.value, C.byref(r), C.byref(t)))
            check(getattr(lib, GAMES[game])(h, C.byref(st)))
            check(lib.sdqn_env_get_dynamics(h, None, None, None, C.byref(sticky)))
            rows.append([r.value, t.value, sticky.value] + words())
            if t.value:
                check(lib.sdqn_env_restart(h))
                t.value = 0
        return rows
    finally:
        lib.sdqn_env_destroy(h)


def record():
    import simple_dqn_amd as sd
    lib = sd.load()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    rows = [[fn, a, evaluate(lib, fn, a)] for fn, a in cases()]
    print('{"recorded_from": "%s",\n "cases": [' % commit)
    print(",\n".join("  " + json.dumps(r) for r in rows))
    print(" ]}")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def lib():
    import simple_dqn_amd as sd
    return sd.load()


def test_the_golden_file_covers_the_edges(golden):
    assert [[fn, a] for fn, a, _ in golden] == cases()
    assert len(golden) > 300


def test_library_gives_the_recorded_answers(lib, golden):
    bad = [(fn, a) for fn, a, want in golden if evaluate(lib, fn, a) != want]
    assert not bad, bad[:5]


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "emul", "streams")
    src = os.path.join(HERE, "emul", "streams.cpp")
    csrc = os.path.join(ROOT, "simple_dqn_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("hd.h", "stream.h", "net_layout.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-o", exe, src])

    def run(lines):
        text = "".join(" ".join(str(x) for x in l) + "\n" for l in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in l.split()] for l in out]
    return run


def test_only_the_three_headers_are_included():
    src = open(os.path.join(HERE, "emul", "streams.cpp")).read()
    quoted = [l.split('"')[1] for l in src.splitlines() if l.startswith("#include") and '"' in l]
    assert sorted(os.path.basename(q) for q in quoted) == ["hd.h", "net_layout.h", "stream.h"]
    for h in ("hd.h", "stream.h", "net_layout.h"):
        text = open(os.path.join(ROOT, "simple_dqn_amd", "csrc", h)).read()
        assert "hip/" not in text and all(l.split('"')[1] in ("hd.h", "stream.h") for l in text.splitlines() if l.startswith("#include") and '"' in l), h


def test_standalone_headers_give_the_recorded_answers(program, golden):
    """every recorded case but the games' rules: a game's first draw and its sticky generator's seed are checked on catch, whose spawn is
    one line (col = d % 12, dx = (d / 12) % 3 - 1)"""
    lines, want = [], []
    for fn, a, out in golden:
        if fn == "sdqn_noisy_words":
            for i in range(a[5]):
                lines.append(["noisy"] + a[:5] + [i]); want.append([out[i]])
        elif fn in ("sdqn_redo_draw", "sdqn_reset_draw"):
            lines.append([fn[5:-5]] + a); want.append(out)
        elif fn == "sdqn_random_shift_draw":
            lines.append(["shift"] + a); want.append(out)
        elif fn == "sdqn_bootstrap_mask":
            seed, P, K, index = a
            for k in range(K):
                lines.append(["mask", seed, int(math.ceil(math.ldexp(P, 53))), index, k]); want.append([out[k]])
        elif fn == "sdqn_bootstrap_head_of":
            lines.append(["head"] + a); want.append(out)
        elif a[0] == "catch":
            r, t, sticky, row, col, dx, paddle, balls, terminal, rng_lo, rng_hi = out[0]
            lines.append(["game", a[1]]); want.append([col, dx - 2 ** 32 if dx >> 31 else dx, rng_lo | rng_hi << 32, sticky])
    got = program(lines)
    bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:5]


def test_layout_agrees_with_layer_shapes(program):
    from simple_dqn_amd.deepqnetwork import layer_shapes
    A = 18
    shapes = layer_shapes(A)
    sizes = [int(np.prod(s)) for s in shapes]
    firsts = [sum(sizes[:l]) for l in range(5)]
    assert firsts == OFF and sum(sizes) == END
    fan_in = [int(np.prod(s[:-1])) for s in shapes[:3]] + [s[1] for s in shapes[3:]]
    assert fan_in == [256, 512, 576, 3136, 512]
    bound = [struct.unpack("<I", struct.pack("<f", math.sqrt(3.0 / f)))[0] for f in fan_in]
    got = program([["layer", L] for L in (1, 2, 3, 4, 5)])
    assert got == [[firsts[L - 1], bound[L - 1]] for L in (1, 2, 3, 4, 5)]
    probe = sorted(set(EDGES + [1, END - 512, OFF[4] + 511, OFF[4] + 512]))
    assert program([["layer_of", i] for i in probe]) == [[layer_of(i)] for i in probe]
    # the ReLU layers' unit counts and their scores' offsets: the output features of conv1..3 and fc4
    units = [shapes[0][-1], shapes[1][-1], shapes[2][-1], shapes[3][0]]
    assert program([["units", l] for l in range(4)]) == [[units[l], sum(units[:l])] for l in range(4)]
    assert program([["units", 4]]) == [[0, sum(units)]]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"]
    record()
