"""Fused attention + output projection (ops.attn_proj, the opt-in
MDI_FUSE_ATTN_PROJ=1 path) against an fp64 reference.

Reference: res + bias + W @ bf16(y), y from the shared attention reference,
all in fp64.  Tolerance per output row m:

    2^-8 |ref_m|  +  2^-9 sum_k |W_mk bf16(y)_k|                (the GEMV)
      +  sum_k |W_mk| (2^-8 |y_k| + 2^-9 A_k)                   (attention)

i.e. the bf16 rounding of the result, fp32 accumulation relative to the
dot product's own condition number, and the attention bound of
attn_reference propagated through |W|.

Every call gets a freshly zeroed hand-off scratch: re-using one at the same
(slot, pos) is documented as unsupported.  The kernel's spin is bounded and
writes NaN on a timeout, which fails the comparison like any wrong value.
"""

import itertools
import math

import pytest
import torch

from attn_reference import make_case, pick_probes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64

GEOMS = [(4, 2, 128), (1, 2, 64), (8, 1, 128), (2, 2, 256)]
PARAMS = list(itertools.product(GEOMS, (64, 200), (1, 17, 300),
                                (False, True)))


def case_kw(geom, S):
    qpk, n_kv, hs = geom
    pos = S - 1
    return dict(qpk=qpk, n_kv=n_kv, hs=hs, pos=pos, max_seq=512,
                probes=pick_probes(S, [0, 15, 16, pos - 1, pos]), kv8=False,
                seed=900 + 10 * GEOMS.index(geom) + (S % 7))


def case_kwargs():
    """make_case arguments of every attention input used below (the CPU
    suite checks their probe precondition)."""
    return [case_kw(g, S) for g in GEOMS for S in (1, 17, 300)]


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _i32(v):
    return torch.tensor(v, device=DEV, dtype=torch.int32)


def proj_inputs(case, M, S):
    """W, res, bias of one case (CPU, bf16)."""
    K = case.n_head * case.hs
    gen = torch.Generator().manual_seed(1000 + M + S)
    W = (torch.randn(M, K, generator=gen) / math.sqrt(K)).to(torch.bfloat16)
    res = torch.randn(M, generator=gen).to(torch.bfloat16)
    bias = torch.randn(M, generator=gen).to(torch.bfloat16)
    return W, res, bias


def launch(ops, case, M, W, res, bias):
    """Run attn_proj on device copies with a freshly zeroed scratch; bias
    may be None.  Returns (guard-padded out buffer, kpool, vpool, qkv, cos,
    sin, pos, slot), all on the device."""
    K = case.n_head * case.hs
    buf = torch.full((M + GUARD,), 12352.0, device=DEV, dtype=torch.bfloat16)
    kpool, vpool = case.kpool.to(DEV), case.vpool.to(DEV)
    qkv = case.qkv.to(DEV).reshape(-1).contiguous()
    cos, sin = case.cos.to(DEV), case.sin.to(DEV)
    pos, slot = _i32(case.pos), _i32(case.slot)
    gran = torch.zeros(K // 2 + 16, device=DEV, dtype=torch.int32)
    ops.attn_proj(buf[:M], qkv, kpool, vpool, cos, sin, pos, slot,
                  case.layer, case.scale, W.to(DEV),
                  None if bias is None else bias.to(DEV), res.to(DEV), gran)
    torch.cuda.synchronize()
    return buf, kpool, vpool, qkv, cos, sin, pos, slot


@pytest.mark.parametrize(
    "geom,M,S,use_bias", PARAMS,
    ids=[f"q{g[0]}-kv{g[1]}-h{g[2]}-M{M}-S{S}-{'bias' if b else 'nobias'}"
         for g, M, S, b in PARAMS])
def test_attn_proj(ops, geom, M, S, use_bias):
    case = make_case(**case_kw(geom, S))
    ref = case.reference()
    assert case.probes_ok(ref), case.probe_weights(ref)
    K = case.n_head * case.hs
    W, res, bias = proj_inputs(case, M, S)

    y = ref.out.reshape(K)
    A = ref.A.reshape(K)
    yb = y.to(torch.bfloat16).double()
    Wd = W.double()
    want = res.double() + Wd @ yb
    if use_bias:
        want = want + bias.double()
    tol = (2.0 ** -8 * want.abs() + 2.0 ** -9 * (Wd.abs() @ yb.abs())
           + Wd.abs() @ (2.0 ** -8 * y.abs() + 2.0 ** -9 * A))

    tail = torch.full((GUARD,), 12352.0, device=DEV, dtype=torch.bfloat16)
    buf, kpool, vpool, qkv, cos, sin, pos, slot = launch(
        ops, case, M, W, res, bias if use_bias else None)

    got = buf[:M].cpu().double()
    err = (got - want).abs()
    ratio = float((err / tol).max()) if bool(torch.isfinite(got).all()) \
        else math.inf
    print(f"ATTN_RATIO attn_proj fused bf16 q{geom[0]}-h{geom[2]}-M{M}-S{S} "
          f"{ratio:.4f}")
    assert bool((err <= tol).all()), f"|got-ref|/bound = {ratio:.3f}"
    assert torch.equal(buf[M:], tail), "out written past M"
    assert torch.equal(qkv.cpu().view(-1), case.qkv.view(-1))

    # the append and the untouched rows are those of attn_decode
    kpool2, vpool2 = case.kpool.to(DEV), case.vpool.to(DEV)
    out2 = torch.empty(K, device=DEV, dtype=torch.bfloat16)
    n_chunks = 8
    part_o = torch.zeros(K * n_chunks, device=DEV)
    part_ml = torch.zeros(case.n_head * n_chunks * 2, device=DEV)
    ops.attn_decode(out2, part_o, part_ml, qkv, kpool2, vpool2, cos, sin,
                    pos, slot, case.layer, n_chunks, case.scale)
    torch.cuda.synchronize()
    assert torch.equal(kpool, kpool2) and torch.equal(vpool, vpool2)
    idx = (case.slot[0], case.layer, slice(None), case.pos[0])
    for after, before in ((kpool, case.kpool), (vpool, case.vpool)):
        a = after.cpu()
        a[idx] = before[idx]
        assert torch.equal(a, before), "a row other than the append changed"


def test_attn_proj_refuses_long_max_seq(ops):
    """max_seq=8192 has no fused instantiation: the binding raises and
    launches nothing."""
    case = make_case(qpk=1, n_kv=2, hs=64, pos=16, max_seq=8192,
                     probes=[0, 16], n_slots=2, seed=990)
    K, M = case.n_head * case.hs, 64
    out = torch.full((M,), 12352.0, device=DEV, dtype=torch.bfloat16)
    kpool, vpool = case.kpool.to(DEV), case.vpool.to(DEV)
    W = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    gran = torch.zeros(K // 2 + 16, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        ops.attn_proj(out, case.qkv.to(DEV).reshape(-1), kpool, vpool,
                      case.cos.to(DEV), case.sin.to(DEV), _i32(case.pos),
                      _i32(case.slot), case.layer, case.scale, W, None,
                      torch.zeros(M, device=DEV, dtype=torch.bfloat16), gran)
    torch.cuda.synchronize()
    assert bool((out == 12352.0).all())
    assert int(gran.abs().sum()) == 0
    assert torch.equal(kpool.cpu(), case.kpool)
    assert torch.equal(vpool.cpu(), case.vpool)
