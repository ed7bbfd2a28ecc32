"""GPU: the grouped-MoE kernels against the fp64 references and derived
bounds of tests/moe_reference.py (its docstring has the rounding points, the
bounds and the mutants; tests/test_moe_reference_cpu.py shows on these exact
inputs that every mutant leaves the bound).

  * expert GEMMs: all 16 moe_group_gemm_kernel instantiations (RB 16/32/64/
    128 x swiglu/down x bf16/fp8) at 1, 2, 3, 3 ragged, 4 and 5 ragged
    K-chunks, M = 48 (three row tiles), two routings;
  * one-hot sweeps that pin the ring slots, both X buffers and every lane's
    fragment offset by equality;
  * the three routers against route_ref, tie rule included, and against
    each other bit for bit;
  * combine, gather and act row kernels.

Every output is a view into a sentinel-filled buffer with padding rows
behind it.  Out of contract and not tested: logits below -1e30 and NaN
(moe_token_topk pads idle lanes with -1e30)."""

import pytest
import torch

import gemv_reference as R
import moe_reference as MR
import test_group_moe_gpu as G
import test_moe_prefill_gpu as P

pytestmark = pytest.mark.gpu

DEV = G.DEV
BF = torch.bfloat16
F64 = torch.float64
SENT = R.SENTINEL          # exact in bf16 and fp32, never a result
PAD = R.PAD_ROWS


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def sentinel_rows(rows, width, dtype):
    buf = torch.full((rows + PAD, width), SENT, device=DEV, dtype=dtype)
    return buf, buf[:rows]


def assert_rows_written(buf, rows, skipped=()):
    """Padding rows and `skipped` rows keep the sentinel; no other row
    holds one."""
    b = buf.float().cpu()
    assert bool((b[rows:] == SENT).all()), "a padding row was written"
    keep = torch.zeros(rows, dtype=torch.bool)
    keep[list(skipped)] = True
    assert bool((b[:rows][keep] == SENT).all()), "an unowned row was written"
    assert not bool((b[:rows][~keep] == SENT).any()), "an owned row is stale"


def dev_routing(rt: MR.Routing):
    i32 = dict(device=DEV, dtype=torch.int32)
    return dict(count=rt.count.to(**i32), offset=rt.offset.to(**i32),
                perm=rt.perm.to(**i32), inv=rt.inv.to(**i32),
                escale=rt.escale.reshape(-1).float().to(DEV))


def slab_args(s: MR.Slab):
    if s.fmt == "bf16":
        return (s.w.to(DEV),)
    return (s.q.to(DEV), s.scale.to(DEV))


def launch_gemm(ops, op, fmt, Wa, Wb, X, d, k, n_tokens):
    """One launch into a fresh sentinel buffer; Wa/Wb are slab_args."""
    rows = n_tokens * k
    M = Wa[0].size(1)
    if op == "swiglu":
        buf, out = sentinel_rows(rows, M, BF)
        fn = ops.moe_group_swiglu if fmt == "bf16" else ops.moe_group_swiglu_fp8
        fn(out, *Wa, *Wb, X, d["count"], d["offset"], d["perm"], d["escale"],
           k)
    else:
        buf, out = sentinel_rows(rows, M, torch.float32)
        fn = ops.moe_group_down if fmt == "bf16" else ops.moe_group_down_fp8
        fn(out, *Wa, X, d["count"], d["offset"], n_tokens)
    return buf


# ---------------------------------------------------------------------------
# 1. expert GEMMs at every chunk count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", MR.gemm_cases(), ids=lambda c: c.id)
def test_expert_gemm(ops, case):
    inp = MR.make_gemm_inputs(case)
    rt = MR.gemm_routing(inp.logits)
    ref = MR.gemm_reference(case, inp, rt)
    rows = case.B * MR.TOP_K
    assert int(rt.count.sum()) == rows == ref.ref.size(0)
    d = dev_routing(rt)
    Wa = slab_args(inp.Wa)
    Wb = slab_args(inp.Wb) if inp.Wb is not None else None
    X = inp.X.to(DEV)

    buf = launch_gemm(ops, case.op, case.fmt, Wa, Wb, X, d, MR.TOP_K, case.B)
    assert_rows_written(buf, rows)
    q = MR.ratio(buf[:rows], ref)
    worst = float(q.max())
    s, m = divmod(int(q.argmax()), MR.M_ROWS)
    print(f"MARGIN {case.op} RB{case.RB} {case.fmt} nch{case.label} "
          f"{case.routing}: err/bound {worst:.3f} at row {s} col {m}")
    assert worst <= 1.0, (case.id, s, m, float(buf[s, m]),
                          float(ref.ref[s, m]))
    # a second launch is bit-identical
    again = launch_gemm(ops, case.op, case.fmt, Wa, Wb, X, d, MR.TOP_K,
                        case.B)
    assert torch.equal(again, buf)


# ---------------------------------------------------------------------------
# 2. exact ring order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("RB", [16, 32, 64, 128])
def test_one_hot_ring_order_exact(ops, RB):
    """All tokens on expert 1, k = 1, token b one-hot at (b + shift) % K,
    K = 3*KC + 32 (four chunks, the last ragged): every sum is one term, so
    D[b, m] must EQUAL W[1, m, pos_b] (times the power-of-two row scale),
    and the fp8 SwiGLU must equal the bf16 SwiGLU on the dequantized slabs
    bit for bit.  The sweep visits every k, so every ring slot, both X
    buffers and every lane's fragment offset are pinned.  The bf16 SwiGLU
    itself is held to the single-term fp64 value under gemv_bound with
    K = 0 (adding zeros is exact); neighbouring weights are 10 % apart."""
    B, K, n_e, M, k = MR.B_OF_RB[RB], MR.one_hot_K(RB), MR.N_E, MR.M_ROWS, 1
    assert MR.rb_of(B) == RB and MR.n_chunks(K, RB) == 4
    rt = MR.gemm_routing(G.all_to_one_logits(B, n_e), k)
    assert rt.count.tolist() == [0, B, 0] and bool((rt.escale == 1).all())
    d = dev_routing(rt)

    wg, wu, wd = (MR.exact_bf16_slab(n_e, M, K, salt).to(DEV)
                  for salt in (5, 977, 1409))
    s8 = [MR.exact_fp8_slab(n_e, M, K, step) for step in (17, 29, 41)]
    deq = [s.dequant_bf16() for s in s8]
    for s, dq in zip(s8, deq):
        assert torch.equal(dq.float(), R.fp8_decode(s.q) * s.scale[..., None])
    g8, u8, d8 = (slab_args(s) for s in s8)
    gd, ud, dd = (dq.to(DEV) for dq in deq)
    wg64, wu64 = wg[1].to(F64), wu[1].to(F64)

    def down(fmt, W, X):
        return launch_gemm(ops, "down", fmt, W, None, X, d, k, B)

    def swiglu(fmt, Wa, Wb, X):
        return launch_gemm(ops, "swiglu", fmt, Wa, Wb, X, d, k, B)

    hit = torch.zeros(K, dtype=torch.bool)
    n_launch = 0
    for shift in range(0, K, B):
        pos = ((torch.arange(B) + shift) % K)
        hit[pos] = True
        pd = pos.to(DEV)
        X = MR.one_hot_tokens(B, K, shift).to(DEV)
        where = (RB, shift)

        D = down("bf16", (wd,), X)
        assert torch.equal(D[:B], wd[1][:, pd].T.float()), where
        D8 = down("fp8", d8, X)
        assert torch.equal(D8[:B], dd[1][:, pd].T.float()), where
        assert bool((D[B:] == SENT).all()) and bool((D8[B:] == SENT).all())

        act8 = swiglu("fp8", g8, u8, X)
        act = swiglu("bf16", (gd,), (ud,), X)
        assert torch.equal(act8, act), where
        assert bool((act[B:].float() == SENT).all())

        actw = swiglu("bf16", (wg,), (wu,), X)[:B].to(F64)
        g, u = wg64[:, pd].T, wu64[:, pd].T
        a = R.activation(g, 3)
        bound = R.gemv_bound(a * u, R.ACT_LIP * g.abs() * u.abs()
                             + a.abs() * u.abs(), 0)
        assert bool(torch.isfinite(actw).all()), where
        assert bool(((actw - a * u).abs() <= bound).all()), where
        n_launch += 1
    assert bool(hit.all()) and n_launch == -(-K // B) <= 98

    # teeth: a slab with chunks 1 and 2 exchanged, tokens inside chunk 1
    shift = MR.KC_OF_RB[RB]
    pd = ((torch.arange(B) + shift) % K).to(DEV)
    X = MR.one_hot_tokens(B, K, shift).to(DEV)
    for fmt, W, dense in (("bf16", (wd,), wd),
                          ("fp8", d8, dd)):
        sw = (MR.swap_chunks_1_2(W[0], RB).contiguous(),) + W[1:]
        got = down(fmt, sw, X)[:B]
        assert not torch.equal(got, dense[1][:, pd].T.float()), (RB, fmt)
        assert torch.equal(
            got, MR.swap_chunks_1_2(dense, RB)[1][:, pd].T.float()), (RB, fmt)


# ---------------------------------------------------------------------------
# 3. routers
# ---------------------------------------------------------------------------
def gate_rows(ops, logits, k, rows):
    """moe_gate_topk, one launch per listed row, into slices of one pair of
    sentinel-filled buffers."""
    B = logits.size(0)
    eidx = torch.full((B * k + 8,), -7, device=DEV, dtype=torch.int32)
    escale = torch.full((B * k + 8,), -7.0, device=DEV)
    lg = logits.to(DEV).contiguous()
    for b in rows:
        ops.moe_gate_topk(eidx[b * k:(b + 1) * k], escale[b * k:(b + 1) * k],
                          lg[b], k)
    return eidx, escale


def check_router(r, rt: MR.Routing, where):
    """Index outputs by equality, escale under ESCALE_RTOL + the smallest
    normal fp32."""
    for name in ("eidx", "count", "offset", "perm", "inv"):
        want = getattr(rt, name).reshape(-1)
        assert torch.equal(r[name].cpu().long(), want), (where, name)
    assert MR.escale_ok(r["escale"], rt.escale, G.ESCALE_RTOL), where
    rel = ((r["escale"].cpu().double() - rt.escale.reshape(-1)).abs()
           / rt.escale.reshape(-1).clamp_min(MR.FP32_TINY)).max()
    print(f"router {where}: max rel escale err={float(rel):.3g}")


@pytest.mark.parametrize("case", MR.router_cases(), ids=lambda c: c.id)
def test_routers(ops, case):
    logits, k = case.logits, case.k
    B = logits.size(0)
    rt = MR.route_ref(logits, k)
    rg = G.route(ops, logits, k)
    check_router(rg, rt, "group " + case.id)
    rp = P.route_prefill(ops, logits, k)
    for name in rg:   # bit for bit, escale included, tied logits too
        assert torch.equal(rp[name], rg[name]), ("prefill", case.id, name)
    eidx, escale = gate_rows(ops, logits, k, range(B))
    assert torch.equal(eidx[:B * k], rg["eidx"]), ("gate", case.id)
    assert torch.equal(escale[:B * k], rg["escale"]), ("gate", case.id)
    assert bool((eidx[B * k:] == -7).all())
    assert bool((escale[B * k:] == -7.0).all())


@pytest.mark.parametrize("case", MR.prefill_edge_cases(), ids=lambda c: c.id)
def test_prefill_router_segment_edges(ops, case):
    """T*k around the MOE_SEG = 1024 boundaries, n_e = 5 (the (n_e+3)/4
    grid has idle waves), logits full of ties."""
    logits, k = case.logits, case.k
    T = logits.size(0)
    rp = P.route_prefill(ops, logits, k)
    check_router(rp, MR.route_ref(logits, k), "prefill " + case.id)
    assert P.same(rp, P.route_prefill(ops, logits, k))
    # the single-sample router on the tokens next to each segment boundary
    rows = sorted({0, T - 1} | {t for f in (1023, 1024, 2047, 2048)
                                for t in (f // k,) if t < T})
    eidx, escale = gate_rows(ops, logits, k, rows)
    for t in rows:
        sl = slice(t * k, (t + 1) * k)
        assert torch.equal(eidx[sl], rp["eidx"][sl]), (case.id, t)
        assert torch.equal(escale[sl], rp["escale"][sl]), (case.id, t)


# ---------------------------------------------------------------------------
# 4. combine and row kernels
# ---------------------------------------------------------------------------
SHAPES = [(k, w, n) for k in (1, 2, 8) for w in (8, 2048, 2056)
          for n in (1, 128)]


def row_inputs(k, width, n, seed):
    g = torch.Generator().manual_seed(seed + 1000 * k + width + n)
    res = torch.randn(n, width, generator=g).to(BF)
    D = torch.randn(n * k, width, generator=g)
    inv = torch.randperm(n * k, generator=g).to(torch.int32)
    return g, res, D, inv


@pytest.mark.parametrize("k,width,n", SHAPES)
def test_group_combine(ops, k, width, n):
    _, res, D, inv = row_inputs(k, width, n, 1)
    if n * k > 1:
        inv[n * k // 2] = -1                       # skipped
    ref = MR.combine_ref(res, D, inv, k)
    buf, out = sentinel_rows(n, width, BF)
    resd, Dd, invd = res.to(DEV), D.to(DEV), inv.to(DEV)
    ops.moe_group_combine(out, resd, Dd, invd, k)
    assert_rows_written(buf, n)
    worst = float(MR.ratio(out, ref).max())
    print(f"MARGIN group_combine k{k} w{width} B{n}: err/bound {worst:.3f}")
    assert worst <= 1.0
    alias = resd.clone()
    ops.moe_group_combine(alias, alias, Dd, invd, k)
    assert torch.equal(alias, out)


@pytest.mark.parametrize("k,width,n", SHAPES)
def test_prefill_combine(ops, k, width, n):
    _, res, D, inv = row_inputs(k, width, n, 2)
    D = D.to(BF)
    if n * k > 1:
        inv[n * k // 2] = -1
    ref = MR.combine_ref(res, D, inv, k)
    buf, out = sentinel_rows(n, width, BF)
    resd, Dd, invd = res.to(DEV), D.to(DEV), inv.to(DEV)
    ops.moe_prefill_combine(out, resd, Dd, invd, k)
    assert_rows_written(buf, n)
    worst = float(MR.ratio(out, ref).max())
    print(f"MARGIN prefill_combine k{k} w{width} T{n}: err/bound {worst:.3f}")
    assert worst <= 1.0
    alias = resd.clone()
    ops.moe_prefill_combine(alias, alias, Dd, invd, k)
    assert torch.equal(alias, out)


@pytest.mark.parametrize("k,width,n", SHAPES)
def test_prefill_gather(ops, k, width, n):
    g, hn, _, perm = row_inputs(k, width, n, 3)
    skipped = []
    if n * k > 1:
        perm[n * k // 2] = -1                      # row left untouched
        skipped = [n * k // 2]
    buf, XG = sentinel_rows(n * k, width, BF)
    ops.moe_prefill_gather(XG, hn.to(DEV), perm.to(DEV), k)
    assert_rows_written(buf, n * k, skipped)
    live = perm >= 0
    want = hn[perm[live].long() // k]
    assert torch.equal(XG.cpu()[live], want)


@pytest.mark.parametrize("k,width,n", SHAPES)
def test_prefill_act(ops, k, width, n):
    g, _, _, perm = row_inputs(k, width, n, 4)
    rows = n * k
    Gt = (torch.randn(rows, width, generator=g) * 2).to(BF)
    U = torch.randn(rows, width, generator=g).to(BF)
    es = torch.rand(rows, generator=g) + 0.05
    skipped = []
    if rows > 1:
        perm[rows // 2] = -1
        skipped = [rows // 2]
    ref = MR.prefill_act_ref(Gt, U, es, perm)
    buf, ACT = sentinel_rows(rows, width, BF)
    ops.moe_prefill_act(ACT, Gt.to(DEV), U.to(DEV), es.to(DEV),
                        perm.to(DEV))
    assert_rows_written(buf, rows, skipped)
    live = perm >= 0
    q = MR.ratio(ACT, ref)[live]
    worst = float(q.max())
    print(f"MARGIN prefill_act k{k} w{width} T{n}: err/bound {worst:.3f}")
    assert worst <= 1.0
