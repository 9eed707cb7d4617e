"""Learning curves of --munchausen on catch: tests/test_gpu_catch.py's loop with an evaluation every 5 000 environment
steps, one seed per call, with and without the option.  Prints one JSON line: the curve and the first evaluation at which the mean reward
per ball reaches the midpoint between the random policy's and +1 (the learning tests' criterion)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import simple_dqn_amd as sd
from test_gpu_catch import _midpoint, learning_run

ap = argparse.ArgumentParser()
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--steps", type=int, default=60000)
ap.add_argument("--every", type=int, default=5000)
ap.add_argument("--munchausen", type=int, default=1)
ap.add_argument("--tau", type=float, default=0.03)
ap.add_argument("--alpha", type=float, default=0.9)
ap.add_argument("--clip", type=float, default=-1.0)
a = ap.parse_args()
kw = dict(munchausen=True, munchausen_alpha=a.alpha, munchausen_tau=a.tau, munchausen_clip=a.clip) if a.munchausen else {}
before, curve = learning_run(sd, a.seed, a.steps, every=a.every, **kw)
cross = next((s for s, v in curve if v >= _midpoint()), None)
print(json.dumps({"seed": a.seed, "munchausen": bool(a.munchausen), "tau": a.tau, "alpha": a.alpha, "clip": a.clip, "midpoint": round(_midpoint(), 4),
                  "untrained": round(before, 4), "curve": [[s, round(v, 4)] for s, v in curve], "first_crossing": cross}), flush=True)
