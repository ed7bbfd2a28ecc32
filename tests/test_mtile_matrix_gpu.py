"""GPU: mtile_gemm against the fp64 reference X W^T (+bias) (+res) under
the GEMV bound of gemv_reference.py (no tolerance is set here).

The matrix runs every batch instantiation (B 16/32/64/128 with KC
512/512/256/128) at K = 2, 4 and 6 chunks — the depths at which the second
slot of the two-deep W ring is the last one, is reloaded once, and is
reloaded twice — at M = 16 (one block), 48 and 272, with the four bias/res
combinations.  Rows of X and W are independent draws, so a wrong batch row
inside a 16-tile, two swapped 8-element groups or a lost quarter-chunk land
far outside the bound (test_prefill_reference_cpu.py shows that on the
CPU).  Y is the [:B*M] view of a sentinel-padded buffer.
"""

import pytest
import torch

import gemv_reference as G
import prefill_reference as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
SENTINEL = G.SENTINEL
CASES = {c.id: c for c in P.mtile_matrix()}


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _d(t):
    return None if t is None else t.to(DEV)


def _ybuf(B, M):
    n = B * M
    buf = torch.full((n + G.PAD_ROWS,), SENTINEL, dtype=BF, device=DEV)
    return buf, buf[:n].view(B, M)


@pytest.mark.parametrize("cid", list(CASES))
def test_mtile_matrix(ops, cid):
    case = CASES[cid]
    inp = P.make_mtile_inputs(case)
    r = P.mtile_reference(inp)
    buf, Y = _ybuf(case.B, case.M)
    ops.mtile_gemm(Y, _d(inp.W), _d(inp.X), _d(inp.bias), _d(inp.res))
    torch.cuda.synchronize()
    host = buf.cpu()
    n = case.B * case.M
    ok, worst = P.mtile_error_ok(host[:n].view(case.B, case.M), r, case.K)
    print(f"MTILE_RATIO {cid} {worst:.4f}")
    assert bool((host[n:].float() == SENTINEL).all()), "wrote past Y"
    assert not bool((host[:n].float() == SENTINEL).any()), \
        "an element of Y was never written"
    assert ok, f"{cid}: err/bound {worst:.3g}"


# ---------------------------------------------------------------------------
# refusals: shapes without an instantiation and mis-sized arguments raise
# before any launch (Y keeps its sentinel)
def _t(*shape):
    return torch.ones(*shape, dtype=BF, device=DEV)


def _refusals():
    B, K, M = 16, 1024, 32

    def shape(**kw):
        a = dict(dict(B=B, K=K, M=M), **kw)
        return lambda Y: (Y, _t(a["M"], a["K"]), _t(a["B"], a["K"]), None,
                          None)

    W, X = _t(M, K), _t(B, K)
    return {
        "B-8": (8, M, shape(B=8)),
        "K-one-chunk": (B, M, shape(K=512)),
        "K-three-chunks": (B, M, shape(K=1536)),
        "M-24": (B, 24, shape(M=24)),
        "bias-size": (B, M, lambda Y: (Y, W, X, _t(M + 16), None)),
        "bias-dtype": (B, M, lambda Y: (Y, W, X, _t(M).float(), None)),
        "res-size": (B, M, lambda Y: (Y, W, X, None, _t(B + 1, M))),
        "res-dtype": (B, M, lambda Y: (Y, W, X, None, _t(B, M).float())),
        "res-strided": (B, M, lambda Y: (Y, W, X, None,
                                         _t(B, 2 * M)[:, :M])),
        "bias-device": (B, M, lambda Y: (Y, W, X, _t(M).cpu(), None)),
        "W-3d": (B, M, lambda Y: (Y, W.view(2, M // 2, K), X, None, None)),
        "X-1d": (B, M, lambda Y: (Y, W, X.flatten(), None, None)),
        "W-strided": (B, M, lambda Y: (Y, _t(M, 2 * K)[:, :K], X, None,
                                       None)),
    }


REFUSALS = ["B-8", "K-one-chunk", "K-three-chunks", "M-24", "bias-size",
            "bias-dtype", "res-size", "res-dtype", "res-strided",
            "bias-device", "W-3d", "X-1d", "W-strided"]


@pytest.mark.parametrize("which", REFUSALS)
def test_mtile_refuses_before_launch(ops, which):
    table = _refusals()
    assert set(table) == set(REFUSALS)
    B, M, args = table[which]
    buf, Y = _ybuf(B, M)
    with pytest.raises(RuntimeError):
        ops.mtile_gemm(*args(Y))
    torch.cuda.synchronize()
    assert bool((buf.float() == SENTINEL).all()), "something was launched"
