#!/usr/bin/env python3
"""Dump the raw output of every decode-GEMV matrix case to one .npz, so two
builds of the extension can be compared byte for byte.

Usage (on a GPU box, once per tree):
    python tools/dump_gemv_outputs.py --tree DIR --out FILE.npz

DIR's built extension is the one loaded.  The cases and inputs are those of
this file's own tree (tests/gemv_reference.py: matrix_cases, make_inputs,
run_case), so every DIR sees identical bytes.  Each array is the whole
sentinel-padded bf16 buffer as uint16 bits, keyed by the case id.  PRE_CASES
are not covered: MDI_GEMV_PRE is latched per process.
"""

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", required=True, help="tree whose build to load")
    ap.add_argument("--out", required=True, help=".npz to write")
    args = ap.parse_args()

    sys.path.insert(0, str(Path(args.tree).resolve()))
    from mdi_llm_amd.ops import require_hip_ops
    ops = require_hip_ops()
    print("extension:", ops.__file__)
    sys.path.insert(1, str(HERE / "tests"))
    import gemv_reference as R

    dumps = {}
    for case in R.matrix_cases():
        buf = R.run_case(ops, case, R.make_inputs(case), "cuda:0")
        torch.cuda.synchronize()
        assert case.id not in dumps, case.id
        dumps[case.id] = buf.cpu().view(torch.int16).numpy().view(np.uint16)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(args.out, **dumps)
    print(f"{len(dumps)} cases -> {args.out}")


if __name__ == "__main__":
    main()
