"""Learning curves on catch under frame skip / sticky actions: tests/test_gpu_dynamics.py's loop (tests/test_gpu_catch.py's
arguments with --train_envs 32 --eval_envs 32) with an evaluation every 5 000 environment steps, one seed per call.  Prints one JSON line:
the curve and the first evaluation at which the mean reward per ball reaches the criterion, half-way between the uniformly random policy
and the landing-column policy, both played by the Python oracle under the same dynamics.
    python tools/dynamics_curves.py [--seed 1] [--steps 60000] [--every 5000] [--repeat_action_probability 0.25] [--frame_skip 1]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import simple_dqn_amd as sd
from test_gpu_dynamics import criterion, learning_run

ap = argparse.ArgumentParser()
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--steps", type=int, default=60000)
ap.add_argument("--every", type=int, default=5000)
ap.add_argument("--repeat_action_probability", type=float, default=0.25)
ap.add_argument("--frame_skip", type=int, default=1)
a = ap.parse_args()
assert a.frame_skip == 1, "the criterion's two oracle policies are defined for frame_skip 1"
rnd, best, mid = criterion(a.repeat_action_probability)
t0 = time.time()
before, curve = learning_run(sd, a.seed, a.steps, every=a.every, p=a.repeat_action_probability, frame_skip=a.frame_skip)
cross = next((s for s, v in curve if v >= mid), None)
print(json.dumps({"seed": a.seed, "repeat_action_probability": a.repeat_action_probability, "frame_skip": a.frame_skip, "random": round(rnd, 4),
                  "landing_column": round(best, 4), "criterion": round(mid, 4), "untrained": round(before, 4),
                  "curve": [[s, round(v, 4)] for s, v in curve], "first_crossing": cross, "seconds": round(time.time() - t0, 1)}), flush=True)
