"""Generates tests/golden/ref_wnms_cases.npz from the REFERENCE's own wnms (oracle/_ref, built by `make -C oracle ref` where the
reference tree is present): the inputs and outputs of tests/test_oracle_pin.py's comparisons with the compiled reference, so that
those tests also run where oracle/_ref cannot be built.  Data only.  Run in the build container:
    python tests/golden/make_ref_wnms_cases.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import cpu_ops as O  # noqa: E402
from rangedet_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ref = O.ref_module()
assert ref is not None, "build oracle/_ref first (make -C oracle ref)"


def seed_dets(seed):
    """test_wnms_vs_compiled_reference's input for `seed`."""
    return synth.cluster_dets([8, 32, 64][seed % 3], [4, 8, 16][seed % 3], seed=100 + seed, quant=(33 if seed % 4 == 0 else None))


out = {}


def put(tag, d, is3d, hs):
    rows, keep = ref.wnms_4c(d, 0.1, 0.5, is3d, hs)
    out["rows_" + tag] = np.array(rows, np.float32).reshape(-1, 12)
    out["keep_" + tag] = np.array(keep, np.int32)


for seed in range(12):
    d = seed_dets(seed)
    out["dets_%d" % seed] = d
    for is3d in (False, True):
        for hs in (100, 10):
            put("%d_%d_%d" % (seed, int(is3d), hs), d, is3d, hs)
for K in (1, 2, 3):       # test_empty_and_tiny_vs_reference
    d = synth.cluster_dets(1, K, seed=K)
    out["dets_tiny%d" % K] = d
    put("tiny%d_0_100" % K, d, False, 100)
np.savez_compressed(os.path.join(HERE, "ref_wnms_cases.npz"), **out)
print("ref_wnms_cases.npz: %d arrays written to %s" % (len(out), HERE))
