#!/usr/bin/env python3
"""Dump the raw results of every decode-attention test case to one .npz, so
two builds of the extension can be compared byte for byte.

Usage (on a GPU box, once per tree):
    python tools/dump_attn_outputs.py --tree DIR --out FILE.npz

DIR's built extension is the one loaded.  The cases and inputs are those of
this file's own tree, so every DIR sees identical bytes:
tests/test_attn_decode_matrix_gpu.py (CASES, run through its launch) and
tests/test_attn_proj_gpu.py (PARAMS, run through its launch).  Per case the
raw bits of the whole guard-padded `out` buffer, kpool, vpool, kscale and
vscale where present, and (attn_decode) part_o and part_ml are stored as
"<case id>/<array>".
"""

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent.parent


def bits(t):
    """Raw bytes of a tensor, whatever its dtype (NaN payloads included)."""
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().copy()


class Recorder:
    """Passes attn_decode through and keeps the tensors of the last call."""

    def __init__(self, ops):
        self.ops = ops

    def attn_decode(self, out, part_o, part_ml, qkv, kpool, vpool, *a,
                    kscale=None, vscale=None, **kw):
        self.ops.attn_decode(out, part_o, part_ml, qkv, kpool, vpool, *a,
                             kscale=kscale, vscale=vscale, **kw)
        # `out` is a view of the guard-padded buffer
        self.last = dict(out=out._base if out._base is not None else out,
                         kpool=kpool, vpool=vpool, kscale=kscale,
                         vscale=vscale, part_o=part_o, part_ml=part_ml)


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
    import test_attn_decode_matrix_gpu as D
    import test_attn_proj_gpu as P
    from attn_reference import make_case

    dumps = {}

    def put(cid, arrays):
        for name, t in arrays.items():
            if t is not None:
                key = f"{cid}/{name}"
                assert key not in dumps, key
                dumps[key] = bits(t)

    rec = Recorder(ops)
    for (spec, path, kv8), cid in zip(D.CASES, D.CASE_IDS):
        case = make_case(kv8=kv8, **spec.kw)
        D.launch(rec, case, spec.n_chunks,
                 path == "split" and spec.force_split,
                 spec.extra.get("n_batch", 0))
        torch.cuda.synchronize()
        put("decode-" + cid, rec.last)

    for geom, M, S, use_bias in P.PARAMS:
        case = make_case(**P.case_kw(geom, S))
        W, res, bias = P.proj_inputs(case, M, S)
        buf, kpool, vpool = P.launch(ops, case, M, W, res,
                                     bias if use_bias else None)[:3]
        put(f"proj-q{geom[0]}-kv{geom[1]}-h{geom[2]}-M{M}-S{S}-"
            f"{'bias' if use_bias else 'nobias'}",
            dict(out=buf, kpool=kpool, vpool=vpool))

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(args.out, **dumps)
    n_cases = len(D.CASES) + len(P.PARAMS)
    print(f"{n_cases} cases, {len(dumps)} arrays -> {args.out}")


if __name__ == "__main__":
    main()
