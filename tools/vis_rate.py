"""Device time of the filter visualisation (DeepQNetwork.visualize, csrc/sdqn_vis.hip): the maximum-activation search over N states
read from a device replay ring at max_fm = 64 (all 160 maps) — states/s and the fraction of the fp32 peak — and the projection launch
(160 records, one workgroup each).  Times are the launches' own HIP event pairs on the library stream, median of the repeats."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from util import make_args

FLOP_PER_STATE = 2 * (400 * 256 * 32 + 81 * 512 * 64 + 49 * 576 * 64)     # conv1 + conv2 + conv3 = 15.47 MFLOP
PEAK = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--states", type=int, default=10000)
ap.add_argument("--max_fm", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
args = make_args(batch_size=32)
mem = sd.ReplayMemory(a.states + 8, args)
rng = np.random.RandomState(1)
mem.screens[:] = rng.randint(0, 256, size=mem.screens.shape, dtype=np.uint8)
mem.count, mem.current = mem.size, 0
net = sd.DeepQNetwork(4, args)
idx = np.arange(4, 4 + a.states, dtype=np.int64)
search, project = [], []
for i in range(a.repeats + 1):
    t = {}
    net.visualize(mem=mem, indexes=idx, max_fm=a.max_fm, timing=t)
    if i:                                            # (the first call warms the code objects and the caches up)
        search.append(t["search_ms"]); project.append(t["project_ms"])
s_ms, p_ms = float(np.median(search)), float(np.median(project))
print(json.dumps({"states": a.states, "max_fm": a.max_fm, "search_ms": round(s_ms, 3), "states_per_s": round(a.states / s_ms * 1e3),
                  "search_tflops": round(FLOP_PER_STATE * a.states / s_ms / 1e9, 2),
                  "fraction_of_fp32_peak": round(FLOP_PER_STATE * a.states / (s_ms * 1e-3) / PEAK, 4),
                  "project_us": round(p_ms * 1e3, 1), "search_ms_all": [round(x, 3) for x in search]}))
