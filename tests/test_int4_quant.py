"""int4 group-quantized weight format (CPU): quantize_int4_groupwise /
dequantize_int4 round trip, padding, degenerate groups, and the CLI flag."""

import subprocess
import sys
from pathlib import Path

import pytest
import torch

from mdi_llm_amd.ops.engine import dequantize_int4, quantize_int4_groupwise

ROOT = Path(__file__).resolve().parent.parent


def _bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """One bf16 unit in the last place of |v| (8 significand bits)."""
    _, e = torch.frexp(v.float().abs())  # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float32),
                       torch.ldexp(torch.ones_like(e, dtype=torch.float32),
                                   e - 8))


@pytest.mark.parametrize("M,K", [(8, 256), (5, 688), (3, 128)])
def test_round_trip(M, K):
    torch.manual_seed(M * 1000 + K)
    w = (torch.randn(M, K) * 0.05 + 0.01).to(torch.bfloat16)
    packed, qp = quantize_int4_groupwise(w)
    Kp = -(-K // 128) * 128
    assert packed.dtype == torch.uint8 and packed.is_contiguous()
    assert tuple(packed.shape) == (M, Kp // 2)
    assert qp.dtype == torch.bfloat16 and qp.is_contiguous()
    assert tuple(qp.shape) == (M, Kp // 128, 2)

    deq = dequantize_int4(packed, qp, K)
    assert deq.dtype == torch.float32 and tuple(deq.shape) == (M, K)
    scale = qp[..., 0].float().repeat_interleave(128, dim=1)[:, :K]
    zero = qp[..., 1].repeat_interleave(128, dim=1)[:, :K]
    bound = scale / 2 + _bf16_ulp(zero)
    err = (deq - w.float()).abs()
    assert bool((err <= bound).all()), float((err - bound).max())

    # the padded tail carries no information: whatever its nibbles hold,
    # the first K columns dequantize the same
    if Kp != K:
        scrambled = packed.clone()
        scrambled.view(M, Kp // 8, 4)[:, K // 8:] = 0xFF
        assert torch.equal(dequantize_int4(scrambled, qp, K), deq)
        # and it takes no part in the last group's range
        last = w[:, (Kp - 128):].float()
        assert torch.allclose(qp[:, -1, 1].float(),
                              last.amin(dim=1).to(torch.bfloat16).float())


def test_matches_format_definition():
    """Nibble value = round((w - zero) / scale) against the stored bf16
    parameters, at the documented position inside each 32-bit word."""
    torch.manual_seed(3)
    w = torch.randn(2, 256).to(torch.bfloat16)
    packed, qp = quantize_int4_groupwise(w)
    s = qp[..., 0].float().repeat_interleave(128, dim=1)
    z = qp[..., 1].float().repeat_interleave(128, dim=1)
    nib = ((w.float() - z) / s).round().clamp(0, 15).to(torch.int64)
    n = nib.view(2, 32, 8)
    word = (n[..., 0] | n[..., 2] << 4 | n[..., 4] << 8 | n[..., 6] << 12
            | n[..., 1] << 16 | n[..., 3] << 20 | n[..., 5] << 24
            | n[..., 7] << 28)
    b = packed.view(2, 32, 4).to(torch.int64)
    got = b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | b[..., 3] << 24
    assert torch.equal(got, word)


def test_degenerate_groups():
    w = torch.randn(4, 256).to(torch.bfloat16)
    w[0, :128] = 0.375          # constant group
    w[1] = 0.0                  # all-zero row
    w[2, 128:] = -2.5           # negative constant group
    packed, qp = quantize_int4_groupwise(w)
    assert bool(torch.isfinite(qp.float()).all())
    deq = dequantize_int4(packed, qp, 256)
    assert bool(torch.isfinite(deq).all())
    assert torch.equal(deq[0, :128], torch.full((128,), 0.375))
    assert torch.equal(deq[1], torch.zeros(256))
    assert torch.equal(deq[2, 128:], torch.full((128,), -2.5))


@pytest.mark.parametrize("cli", ["sample.py", "starter.py", "chat.py"])
def test_cli_accepts_int4(cli):
    # argparse validates --weights before --help exits: an unknown choice
    # would end with status 2 instead of printing the help
    r = subprocess.run(
        [sys.executable, str(ROOT / cli), "--weights", "int4", "--help"],
        capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "int4" in r.stdout
