"""OCP MXFP4 weight format (CPU): quantize_mxfp4 / dequantize_mxfp4 against
a plain fp64 construction of the OCP rule, the slab quantizer, and the CLI
flag."""

import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from mdi_llm_amd.ops.engine import (dequantize_mxfp4, mxfp4_scale_row_bytes,
                                    quantize_mxfp4, quantize_mxfp4_slab)

ROOT = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
GRID = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


def ocp_reference(w: torch.Tensor) -> torch.Tensor:
    """fp64 [M, K]: every block of 32 k scaled by 2^(floor(log2 amax) - 2)
    (clamped to e8m0, 1 for an all-zero block), elements to the nearest
    e2m1 magnitude, a tie to the one with the even mantissa (even index of
    GRID), above 6 to 6."""
    M, K = w.shape
    out = torch.zeros(M, K, dtype=torch.float64)
    for m in range(M):
        for k0 in range(0, K, 32):
            blk = w[m, k0:k0 + 32].double()
            amax = float(blk.abs().max())
            e = 0 if amax == 0 else math.floor(math.log2(amax)) - 2
            scale = 2.0 ** max(-127, min(127, e))
            a = (blk.abs() / scale).clamp(max=6.0)
            d = (a[:, None] - GRID[None]).abs()
            # nearest; of two equally near, the even index
            d = d + torch.tensor([0, 1e-9] * 4, dtype=torch.float64)[None]
            out[m, k0:k0 + 32] = torch.sign(blk) * GRID[d.argmin(1)] * scale
    return out


def _cases():
    torch.manual_seed(41)
    rnd = (torch.randn(5, 96) * 0.07).to(BF)
    pad = torch.randn(3, 40).to(BF)               # K = 40: one padded block
    zero = torch.randn(2, 64).to(BF)
    zero[0, 32:] = 0.0                            # an all-zero block
    six = (torch.rand(2, 32) * 6 * 2.0 ** -5).to(BF)
    six[:, 7] = 6 * 2.0 ** -5                     # amax exactly 6 * 2^e
    six[1, 9] = -5 * 2.0 ** -5                    # tie between 4 and 6
    above = (torch.rand(2, 32) * 0.25).to(BF)
    above[:, 3] = 0.25 * (1 + 2.0 ** -7)          # amax just above 2^-2
    return {"random": rnd, "pad40": pad, "zero_block": zero, "amax6": six,
            "above_pow2": above}


@pytest.mark.parametrize("name", list(_cases()))
def test_matches_ocp_rule(name):
    w = _cases()[name]
    M, K = w.shape
    packed, scales = quantize_mxfp4(w)
    assert packed.dtype == torch.uint8 and packed.is_contiguous()
    assert tuple(packed.shape) == (M, -(-K // 32) * 16)
    assert scales.dtype == torch.uint8
    assert tuple(scales.shape) == (M, mxfp4_scale_row_bytes(K))
    deq = dequantize_mxfp4(packed, scales, K)
    assert deq.dtype == torch.float32 and tuple(deq.shape) == (M, K)
    assert torch.equal(deq.double(), ocp_reference(w))
    # e2m1 times a power of two: nothing is lost in bf16
    assert torch.equal(deq.to(BF).float(), deq)


def test_slab_equals_per_expert_calls():
    torch.manual_seed(42)
    slab = (torch.randn(3, 6, 72) * 0.1).to(BF)
    q, s = quantize_mxfp4_slab(slab)
    for e in range(3):
        qe, se = quantize_mxfp4(slab[e])
        assert torch.equal(q[e], qe) and torch.equal(s[e], se)


@pytest.mark.parametrize("cli", ["sample.py", "starter.py", "chat.py"])
def test_cli_accepts_mxfp4(cli):
    # argparse validates --weights before --help exits: an unknown choice
    # would end with status 2 instead of printing the help
    r = subprocess.run(
        [sys.executable, str(ROOT / cli), "--weights", "mxfp4", "--help"],
        capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "mxfp4" in r.stdout
