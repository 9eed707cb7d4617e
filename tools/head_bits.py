"""Bits of the option heads' train steps: for each cell of a fixed grid — the Munchausen, advantage-learning (AL / PAL),
bootstrap and quantile heads over their action buckets, with n-step returns and prioritized replay where the head takes them, float16,
batch sizes on both sides of the launch structures' edges, and the fc4 split-K loop (option s4 = 3) — two seeded train_from_memory steps
from seeded Xavier weights on a small seeded ring, then one JSON line with the sha256 of the step's buffers (debug_read: q, a4, d4, dq,
cost_terms, g; quantile_targets for the quantile head), both steps' bytes in one digest.  `--generic` prints the generic path's grid instead
(generic_net.hip's head_kernel, whose branches are the rule headers of DESIGN.md §31): the standard, Double DQN, Munchausen, AL, PAL,
bootstrap, quantile, dueling and CQL heads with prioritized replay and 3-step returns where the head takes them, in float64 at 84 x 84 x 4
and in float32 at 36 x 36 x 5, batch size 3; a digest of what the public API shows of both steps (last_q, the cost, every layer's gradient
sums and weights), since debug_read is the tuned path's.  The kernels have fixed summation orders and no
atomics: two builds that compute the same thing print the same lines, so `diff` of two outputs is the comparison.  Uses only the public
Python API; SDQN_LIB_PATH (simple_dqn_amd/_lib.py) points it at another build of the library.
    python tools/head_bits.py [--generic] [--out FILE] [-k substring]"""
import argparse, hashlib, json, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args

PER = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6)
MODES = {"plain": {}, "n3": dict(n_step=3), "per": PER, "n3_per": dict(PER, n_step=3)}
HEADS = {   # head: (option keywords from x = Q-heads K / quantiles N, modes)
    "munchausen": (lambda x: dict(munchausen=True, munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-0.05), ["plain", "n3", "per", "n3_per"]),
    "al": (lambda x: dict(advantage_learning=0.9), ["plain", "n3", "per", "n3_per"]),
    "pal": (lambda x: dict(advantage_learning=0.9, persistent_advantage=True), ["plain", "per"]),
    "bootstrap": (lambda x: dict(bootstrap_heads=x, bootstrap_mask_probability=0.5, random_seed=5), ["plain", "n3"]),
    "quantile": (lambda x: dict(quantiles=x), ["plain", "n3"]),
}
SHAPES = {"munchausen": [(1, 3), (1, 8), (1, 18)], "al": [(1, 3), (1, 8), (1, 18)], "pal": [(1, 3), (1, 8), (1, 18)],      # (rows per action, A)
          "bootstrap": [(2, 1), (3, 3), (9, 2)], "quantile": [(2, 2), (4, 2), (6, 3), (18, 1)]}


def cells():
    for head, (_, modes) in HEADS.items():
        for x, A in SHAPES[head]:
            for m in modes:
                yield head, x, A, 8, "float32", m, 7
        if head in ("munchausen", "al", "pal"):
            for m in modes:
                yield head, 1, 4, 32, "float16", m, 7
        x, A = SHAPES[head][1]
        for B in (33, 129):                       # the other launch structures: the fc4 split (S4 = 7) is the same in every regime
            yield head, x, A, B, "float32", "plain", 7
        yield head, x, A, 8, "float32", "plain", 3      # option s4 = 3: the split-K loop


def run(head, x, A, B, dt, mode, s4):
    kw = dict(HEADS[head][0](x), **MODES[mode])
    args = make_args(batch_size=B, datatype=dt, **kw)
    mem = sd.ReplayMemory(600, args)
    synthetic_fill(mem, 3, num_actions=A)
    rng = np.random.RandomState(4)
    mem.terminals[:] = rng.rand(600) < 0.05
    mem.rewards[:] = rng.randint(-3, 4, 600)      # outside the clip range too
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    net.set_weights(xavier_weights(x * A, 171), 1)
    net.set_weights(xavier_weights(x * A, 71), 0)
    net.set_option("keep_gradients", 1)
    if s4 != 7:
        net.set_option("s4", s4)
    rows = x * A
    bufs = {"q": 2 * B * rows, "a4": 2 * B * 512, "d4": B * 512, "dq": B * rows, "cost_terms": B,
            "g": sum(np.asarray(net.get_layer(i)).size for i in range(5))}
    if head == "quantile":
        bufs["quantile_targets"] = B * x
    digest = {k: hashlib.sha256() for k in bufs}
    random.seed(17)
    for _ in range(2):
        net.train_from_memory(mem, 1)
        for k, n in bufs.items():
            digest[k].update(net.debug_read(k, n).tobytes())
    return {k: d.hexdigest() for k, d in digest.items()}


GENERIC_HEADS = {   # head: (outputs per game action: (multiplier, extra rows), game actions, option keywords, modes)
    "standard": ((1, 0), 4, {}, ["plain", "n3", "per", "n3_per"]),
    "double": ((1, 0), 4, dict(double_dqn=True), ["plain", "n3", "per", "n3_per"]),
    "munchausen": ((1, 0), 4, HEADS["munchausen"][0](1), ["plain", "n3", "per", "n3_per"]),
    "al": ((1, 0), 4, HEADS["al"][0](1), ["plain", "n3", "per", "n3_per"]),
    "pal": ((1, 0), 4, HEADS["pal"][0](1), ["plain", "per"]),
    "bootstrap": ((6, 0), 3, HEADS["bootstrap"][0](6), ["plain", "n3"]),
    "quantile": ((4, 0), 2, dict(quantiles=4), ["plain", "n3"]),
    "dueling": ((1, 1), 4, dict(dueling=True), ["plain", "n3", "per", "n3_per"]),
    "cql": ((1, 0), 4, dict(cql_alpha=0.5), ["plain", "n3", "per", "n3_per"]),
}
GENERIC_NETS = [("float64", 4, 84, 84), ("float32", 5, 36, 36)]      # (datatype, history, height, width); the second: tests/test_gpu_generic.py's smallest


def generic_cells():
    for head, (_, A, _, modes) in GENERIC_HEADS.items():
        for dt, hist, H, W in GENERIC_NETS:
            for m in modes:
                yield head, A, dt, hist, H, W, m


def run_generic(head, A, dt, hist, H, W, mode):
    (mul, extra), _, kw, _ = GENERIC_HEADS[head]
    B, rows = 3, mul * A + extra
    args = make_args(batch_size=B, datatype=dt, history_length=hist, screen_height=H, screen_width=W, **dict(kw, **MODES[mode]))
    mem = sd.ReplayMemory(600, args)
    synthetic_fill(mem, 3, num_actions=A)
    rng = np.random.RandomState(4)
    mem.terminals[:] = rng.rand(600) < 0.05
    mem.rewards[:] = rng.randint(-3, 4, 600)      # outside the clip range too
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    npd = np.float64 if dt == "float64" else np.float32
    net.set_weights(xavier_weights(rows, 171, npd, hist, H, W), 1)
    net.set_weights(xavier_weights(rows, 71, npd, hist, H, W), 0)
    digest = {k: hashlib.sha256() for k in ("cost", "preq", "maxq", "g", "theta")}
    random.seed(17)
    for _ in range(2):
        digest["cost"].update(np.float64(net.train_from_memory(mem, 1, want_cost=True)).tobytes())
        preq, maxq = net.last_q()
        digest["preq"].update(preq.tobytes()); digest["maxq"].update(maxq.tobytes())
        for i in range(5):
            digest["g"].update(np.ascontiguousarray(net.get_layer(i, 3)).tobytes())
            digest["theta"].update(np.ascontiguousarray(net.get_layer(i, 0)).tobytes())
    return {k: d.hexdigest() for k, d in digest.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("-k", default=None, help="only the cells whose name holds this substring")
    ap.add_argument("--generic", action="store_true", help="the generic path's grid (float64, and float32 at another geometry)")
    a = ap.parse_args()
    for c in (generic_cells() if a.generic else cells()):
        name = ("generic %s A%d %s %dx%dx%d %s" if a.generic else "%s x%d A%d B%d %s %s s4=%d") % c
        if a.k and a.k not in name:
            continue
        line = json.dumps(dict(cell=name, **(run_generic(*c) if a.generic else run(*c))))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
