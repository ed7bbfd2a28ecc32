#!/usr/bin/env python3
"""A/B the fp4-fed M-tile GEMMs against what GroupDecodeEngine runs on bf16
weights for the same shape (Llama-3-8B): F.linear, addmm for the residual
shapes, two linears + swiglu_mul for the gate/up pair.  Both sides run
alternated in one process, warmed and event-timed; bytes/s are the weight
bytes each side has to read, computed from the shapes."""

import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from mdi_llm_amd.ops import require_hip_ops  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
SHAPES = [  # (name, K, M, kind)
    ("qkv", 4096, 6144, "linear"),
    ("proj", 4096, 4096, "residual"),
    ("gate+up", 4096, 14336, "pair"),
    ("down", 14336, 4096, "residual"),
    ("head", 4096, 128256, "linear"),
]


def timed(fn, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def ab(f_ref, f_new, iters=100, warmup=10, rounds=3):
    """Best of `rounds` alternated windows per side, seconds per call."""
    for _ in range(warmup):
        f_ref()
        f_new()
    t_ref = t_new = float("inf")
    for _ in range(rounds):
        t_ref = min(t_ref, timed(f_ref, iters))
        t_new = min(t_new, timed(f_new, iters))
    return t_ref, t_new


def mx_weight(ops, M, K):
    """Random packed bytes and scales (2^-9 .. 2^-1): timing needs the
    layout, not a quantized model."""
    q = torch.randint(0, 256, (M, -(-K // 32) * 16), device=DEV,
                      dtype=torch.uint8)
    s = torch.randint(118, 127, (M, ops.mxfp4_scale_row_bytes(K)),
                      device=DEV, dtype=torch.uint8)
    return q, s


def main():
    ops = require_hip_ops()
    print("| B | shape | K | M | bf16 us | bf16 TB/s | mxfp4 us | mxfp4 TB/s "
          "| speedup |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B in (16, 32, 64, 128):
        for name, K, M, kind in SHAPES:
            n_w = 2 if kind == "pair" else 1
            X = torch.randn(B, K, device=DEV, dtype=BF)
            W = [torch.randn(M, K, device=DEV, dtype=BF) * 0.02
                 for _ in range(n_w)]
            Q = [mx_weight(ops, M, K) for _ in range(n_w)]
            Y = torch.zeros(B, M, device=DEV, dtype=BF)
            res = torch.randn(B, M, device=DEV, dtype=BF)
            if kind == "linear":
                f_ref = lambda: F.linear(X, W[0])  # noqa: E731
                f_new = lambda: ops.mtile_gemm_mxfp4(  # noqa: E731
                    Y, Q[0][0], Q[0][1], X, None, None)
            elif kind == "residual":
                Wt = W[0].t()
                f_ref = lambda: torch.addmm(res, X, Wt)  # noqa: E731
                f_new = lambda: ops.mtile_gemm_mxfp4(  # noqa: E731
                    Y, Q[0][0], Q[0][1], X, None, res)
            else:
                def f_ref():
                    g, u = F.linear(X, W[0]), F.linear(X, W[1])
                    ops.swiglu_mul(u, g, u, False)

                f_new = lambda: ops.mtile_swiglu_mxfp4(  # noqa: E731
                    Y, Q[0][0], Q[0][1], Q[1][0], Q[1][1], X, False)
            t_ref, t_new = ab(f_ref, f_new)
            by_ref = n_w * M * K * 2
            by_new = n_w * sum(t.numel() for t in Q[0])
            print(f"| {B} | {name} | {K} | {M} | {t_ref * 1e6:.1f} | "
                  f"{by_ref / t_ref / 1e12:.2f} | {t_new * 1e6:.1f} | "
                  f"{by_new / t_new / 1e12:.2f} | {t_ref / t_new:.2f}x |",
                  flush=True)
            del W, Q


if __name__ == "__main__":
    main()
