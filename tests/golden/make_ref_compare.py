#!/usr/bin/env python3
"""Regenerates tests/golden/ref_compare_v1.json from the COMPILED REFERENCE (oracle/_ref/libawm_ref.so): what the reference
returns for the input of tests/test_oracle_golden.py::test_against_compiled_reference, so that the test pins the restatement
to the reference where oracle/_ref has not been built.  Run in the build container:

    make -C oracle ref && python tests/golden/make_ref_compare.py

Large arrays are kept as checksums of their bytes (-0.0 folded into 0.0, as np.array_equal sees them), small ones as values."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ref  # noqa: E402

PAY2 = "f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0"


def digest(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "sha256": hashlib.sha256((a + a.dtype.type(0)).tobytes()).hexdigest()}


def pkey(p):
    return [round(p["time"], 9), p["sync_index"], p["type"], p["block_type"], p["bits"]]


def main():
    rng = np.random.default_rng(99)                      # the draws of test_against_compiled_reference, in its order
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    x = rng.uniform(-1, 1, (56 * 44100 + 3, 1)).astype(np.float32)
    w = _ref.add(key, x, 1, PAY2)
    idx, quality, block = _ref.sync_search(key, w.reshape(-1, 1), 1)
    out = {"key": key.hex(), "mix_entries": digest(_ref.mix_entries(key)), "frame_mod": digest(_ref.frame_mod(key, PAY2, 1)),
           "add": digest(w),
           "sync_search": {"index": [int(v) for v in idx], "quality": [float(v) for v in quality], "block_type": [int(v) for v in block]},
           "get": [pkey(p) for p in _ref.get(key, w.reshape(-1, 1), 1)]}
    with open(os.path.join(HERE, "ref_compare_v1.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
