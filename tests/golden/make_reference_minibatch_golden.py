"""Generates tests/golden/reference_minibatch.json by EXECUTING the reference's own ReplayMemory class (loaded by
oracle/ref_loader.py, unmodified) on the synthetic fills of tests/test_oracle_replay.py::test_oracle_vs_live_reference:
three getMinibatch() calls per configuration, each returned array pinned by dtype, shape and CRC-32, and the generator state
after the calls.  Run only where the reference is present; the JSON it writes is the committed fixture the test compares the
oracle with, so the test itself needs nothing outside the repository.

    python tests/golden/make_reference_minibatch_golden.py
"""
import json
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_loader import load_reference_replay_memory  # noqa: E402
from oracle.replay_numpy import synthetic_fill  # noqa: E402
from util import crc, make_args  # noqa: E402

# (size, batch_size, current, count, seed): the configurations of the test
CONFIGS = ((3000, 32, 1000, 3000, 11), (500, 16, 77, 400, 3), (2000, 64, 0, 2000, 9))
NAMES = ("prestates", "actions", "rewards", "poststates", "terminals")


def main():
    RefMem, origin = load_reference_replay_memory()
    if RefMem is None:
        sys.exit("reference not available: %s" % origin)
    warnings.simplefilter("ignore")
    cases = []
    for size, B, cur, cnt, seed in CONFIGS:
        ref = RefMem(size, make_args(batch_size=B))
        synthetic_fill(ref, seed, count=cnt, current=cur)
        random.seed(seed)
        calls = []
        for _ in range(3):
            calls.append({n: {"dtype": str(x.dtype), "shape": list(x.shape), "crc": crc(x)} for n, x in zip(NAMES, ref.getMinibatch())})
        cases.append(dict(size=size, B=B, current=cur, count=cnt, seed=seed, calls=calls,
                          mt_after_crc=crc(np.array(random.getstate()[1], dtype=np.uint32))))
    path = os.path.join(HERE, "reference_minibatch.json")
    with open(path, "w") as f:
        json.dump({"python": sys.version.split()[0], "numpy": np.__version__, "cases": cases}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
