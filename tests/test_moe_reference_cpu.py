"""CPU: the grouped-MoE reference and its bounds (tests/moe_reference.py) on
the exact inputs of tests/test_moe_matrix_gpu.py — route_ref against
torch.topk and the layout of test_group_moe_gpu, every mutant outside the
bound in every case it applies to, an fp32 evaluation of the same formula
inside it, and the tie cases really tied where they claim."""

import pytest
import torch

import gemv_reference as R
import moe_reference as MR
import test_group_moe_gpu as G

F64 = MR.F64
CASES = MR.gemm_cases()


# ---------------------------------------------------------------------------
# routing
@pytest.mark.parametrize("B,n_e,k", [(1, 4, 2), (17, 8, 2), (128, 64, 8),
                                     (5, 5, 5)])
def test_route_ref_equals_topk_without_ties(B, n_e, k):
    logits = G.tie_free_logits(B, n_e, seed=B)
    G.assert_distinct(logits)
    rt = MR.route_ref(logits, k)
    top = torch.topk(logits.float(), k, dim=1)
    assert torch.equal(rt.eidx, top.indices)
    assert torch.allclose(rt.escale, torch.softmax(top.values.double(), 1),
                          rtol=1e-14, atol=0)
    # tie-free: the tie rule cannot matter
    assert torch.equal(MR.route_ref(logits, k, ties_high=True).eidx, rt.eidx)
    for got, want in zip(rt[2:], G.cpu_layout(top.indices.reshape(-1), n_e)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("case", MR.router_cases() + MR.prefill_edge_cases(),
                         ids=lambda c: c.id)
def test_route_ref_lowest_index_among_equals(case):
    lg, k = case.logits.double(), case.k
    B, n_e = lg.shape
    rt = MR.route_ref(case.logits, k)
    assert float(lg.min()) > -1e30 and bool(torch.isfinite(lg).all())
    for b in range(B):
        picked = rt.eidx[b].tolist()
        assert len(set(picked)) == k
        vals = lg[b, picked]
        assert bool((vals[1:] <= vals[:-1]).all())          # by value
        rest = [i for i in range(n_e) if i not in picked]
        for j, i in enumerate(picked):
            # nothing left out beats a pick, and an equal one left out or
            # picked later has a higher index
            assert all(lg[b, r] < lg[b, i] or
                       (lg[b, r] == lg[b, i] and r > i) for r in rest)
            assert all(lg[b, o] < lg[b, i] or o > i for o in picked[j + 1:])
    for got, want in zip(rt[2:], G.cpu_layout(rt.eidx.reshape(-1), n_e)):
        assert torch.equal(got, want)
    assert torch.allclose(rt.escale.sum(1), torch.ones(B, dtype=F64))

    srt = lg.sort(dim=1, descending=True).values
    if case.tie == "all":
        assert bool((lg == lg[:, :1]).all())
        assert rt.eidx.tolist() == [list(range(k))] * B
    if case.tie == "across":    # the tie straddles the k-th/(k+1)-th place
        assert bool((srt[:, k - 1] == srt[:, k]).all())
        assert k == 1 or bool((srt[:, k - 2] > srt[:, k - 1]).all())
    if case.tie == "inside":
        assert bool((srt[:, 0] == srt[:, 1]).all())
    if case.tie == "top_idx":
        assert n_e & (n_e - 1) != 0
        assert bool((lg[:, n_e - 2:] == srt[:, :1]).all())
        assert bool((lg[:, :n_e - 2] < srt[:, :1]).all())
        assert rt.eidx[0].tolist()[:2] == [n_e - 2, n_e - 1][:k]
    if case.tie in ("all", "across") and k < n_e or (
            case.tie == "top_idx" and k == 1):
        # mutant (f): highest index first picks other experts
        hi = MR.route_ref(case.logits, k, ties_high=True)
        assert not torch.equal(hi.eidx.sort(1).values, rt.eidx.sort(1).values)
    if case.tie == "inside":    # same set, other order
        hi = MR.route_ref(case.logits, k, ties_high=True)
        assert not torch.equal(hi.eidx, rt.eidx)


def test_lattice_cases_hold_straddling_ties():
    """The random lattice cases (the ones the three routers are compared
    on at every B and at the prefill segment edges) contain rows whose
    k-th and (k+1)-th logits are equal wherever n_e > 4."""
    n = 0
    for case in MR.router_cases() + MR.prefill_edge_cases():
        n_e = case.logits.size(1)
        if case.tie or not case.id.startswith(("lattice", "edge")):
            continue
        if n_e <= 4 or case.k >= n_e or case.logits.size(0) < 8:
            continue    # one row alone need not tie
        srt = case.logits.double().sort(dim=1, descending=True).values
        assert bool((srt[:, case.k - 1] == srt[:, case.k]).any()), case.id
        n += 1
    assert n >= 10


def test_router_case_table_covers_the_issue():
    cs = MR.router_cases()
    shapes = {(c.logits.size(1), c.k) for c in cs}
    for n_e in (1, 2, 5, 33, 63, 64):
        for k in (1, 2, 3, 8):
            assert (k > n_e) or (n_e, k) in shapes
    assert any(c.k == c.logits.size(1) for c in cs)
    assert {c.logits.size(0) for c in cs} >= {1, 63, 64, 65, 128}
    assert {c.tie for c in cs} == {"", "all", "across", "inside", "top_idx"}
    assert sorted(T * k for T, k in MR.PREFILL_EDGES) == [
        1023, 1024, 1025, 1026, 2048, 2049]
    assert (342, 3) in MR.PREFILL_EDGES and 1024 % 3 != 0


# ---------------------------------------------------------------------------
# expert GEMMs
def test_case_table_launches_every_instantiation_at_every_chunk_count():
    seen = {}
    for c in CASES:
        assert MR.rb_of(c.B) == c.RB
        seen.setdefault((c.RB, c.op, c.fmt), set()).add(c.nch)
        assert c.K % 32 == 0 and MR.M_ROWS % 16 == 0 and MR.M_ROWS // 16 == 3
    assert len(seen) == 16
    assert all(v == {1, 2, 3, 4, 5} for v in seen.values())
    for RB in MR.KC_OF_RB:
        KC = MR.KC_OF_RB[RB]
        assert [K for _, _, K in MR.k_table(RB)] == [
            KC, 2 * KC, 3 * KC, 2 * KC + 32, 4 * KC, 4 * KC + KC // 4 + 32]
    assert max(c.K for c in CASES) == 4 * 512 + 128 + 32


@pytest.mark.parametrize("B", sorted(MR.B_OF_RB.values()))
def test_routings_fill_and_starve(B):
    full = MR.route_ref(MR.routing_logits(B, "full"), MR.TOP_K)
    assert full.count.tolist()[0] == B - 1 and int(full.count.min()) > 0
    st = MR.route_ref(MR.routing_logits(B, "starved"), MR.TOP_K)
    assert st.count.tolist() == [B, 0, B]
    for rt, kind in ((full, "full"), (st, "starved")):
        G.assert_distinct(MR.routing_logits(B, kind))
        assert bool((rt.escale[:, 0] - rt.escale[:, 1] > 0.1).all())
        assert rt.eidx[:, 0].unique().numel() > 1   # rank order varies


@pytest.fixture(scope="module")
def evaluated():
    """(inputs, routing, fp64 reference) per case, computed once."""
    cache = {}

    def get(case):
        if case.id not in cache:
            inp = MR.make_gemm_inputs(case)
            rt = MR.gemm_routing(inp.logits)
            cache[case.id] = (inp, rt, MR.gemm_reference(case, inp, rt))
        return cache[case.id]

    return get


@pytest.mark.parametrize("case", CASES[::7], ids=lambda c: c.id)
def test_batched_reference_is_the_gemv_reference(evaluated, case):
    """group_swiglu_ref / group_down_ref row by row against
    gemv_swiglu_ref / gemv_ref of (token row, expert, escale)."""
    inp, rt, ref = evaluated(case)
    rows = rt.perm.numel()
    for s in sorted({0, 1, rows // 2, rows - 1}):
        e = int((rt.offset[1:] > s).nonzero()[0])
        f = int(rt.perm[s])
        if case.op == "swiglu":
            r = R.gemv_swiglu_ref(inp.Wa.expert(e), inp.Wb.expert(e),
                                  inp.X[f // MR.TOP_K],
                                  escale=float(rt.escale.reshape(-1)[f]))
            want = R.gemv_bound(r.ref, r.A, case.K, r.extra)
        else:
            r = R.gemv_ref(inp.Wa.expert(e), inp.X[s])
            want = (R.gemv_bound(r.ref, r.A, case.K, r.extra)
                    - R.REL_TERM * r.ref.abs() + R.ACC_UNIT * r.ref.abs())
        assert r.n_fragile == 0
        assert torch.allclose(ref.ref[s], r.ref, rtol=1e-11, atol=1e-13)
        assert torch.allclose(ref.A[s], r.A, rtol=1e-11, atol=0)
        assert torch.allclose(ref.bound[s], want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_mutants_leave_the_bound_and_fp32_stays_inside(evaluated, case):
    inp, rt, ref = evaluated(case)
    assert int(rt.count.sum()) == ref.ref.size(0)        # every row is owned
    assert bool((ref.bound > 0).all()) and bool(torch.isfinite(ref.ref).all())

    # the same formula in fp32, split-K in the kernel's order and plain,
    # with the kernel's output rounding: inside the bound everywhere
    for split in (True, False):
        emu = MR.gemm_reference(case, inp, rt, dtype=torch.float32,
                                split=split).ref
        if case.op == "swiglu":
            emu = emu.to(torch.bfloat16)
        worst = float(MR.ratio(emu, ref).max())
        assert worst <= 1.0, (case.id, split, worst)

    tried = 0
    for mut in MR.MUTANTS:
        if not MR.applies(mut, case):
            continue
        bad = MR.gemm_reference(case, inp, rt, mut=mut).ref
        if case.op == "swiglu":    # as the kernel would store it
            bad = bad.to(torch.bfloat16)
        assert float(MR.ratio(bad, ref).max()) > 1.0, (case.id, mut)
        tried += 1
    assert tried >= 2


# ---------------------------------------------------------------------------
# combine and the row kernels
@pytest.mark.parametrize("k", [1, 2, 8])
def test_combine_ref_and_bound(k):
    g = torch.Generator().manual_seed(k)
    B, E = 5, 16
    res = torch.randn(B, E, generator=g).to(torch.bfloat16)
    D = torch.randn(B * k, E, generator=g)
    inv = torch.randperm(B * k, generator=g)
    inv[1] = -1
    r = MR.combine_ref(res, D, inv, k)
    want = res.double().clone()
    for b in range(B):
        for j in range(k):
            s = int(inv[b * k + j])
            if s >= 0:
                want[b] += D[s].double()
    assert torch.equal(r.ref, want)
    # fp32 sum in rank order, one bf16 rounding: inside; the skipped entry
    # added anyway, or a rank dropped: outside
    acc = res.float().clone()
    full = res.float().clone()
    iv = inv.view(B, k)
    for j in range(k):
        ok = (iv[:, j] >= 0)[:, None]
        acc = acc + torch.where(ok, D[iv[:, j].clamp_min(0)],
                                torch.zeros(()))
        full = full + D[iv[:, j].clamp_min(0)]
    assert float(MR.ratio(acc.to(torch.bfloat16), r).max()) <= 1.0
    assert float(MR.ratio(full.to(torch.bfloat16), r).max()) > 1.0
    assert float(MR.ratio((acc - D[iv[:, k - 1].clamp_min(0)])
                          .to(torch.bfloat16), r).max()) > 1.0


def test_prefill_act_ref_and_bound():
    g = torch.Generator().manual_seed(3)
    n, I = 6, 16
    Gt = (torch.randn(n, I, generator=g) * 2).to(torch.bfloat16)
    U = torch.randn(n, I, generator=g).to(torch.bfloat16)
    es = torch.rand(n, generator=g) + 0.1
    perm = torch.randperm(n, generator=g)
    r = MR.prefill_act_ref(Gt, U, es, perm)
    want = (torch.nn.functional.silu(Gt.double()) * U.double()
            * es.double()[perm][:, None])
    assert torch.allclose(r.ref, want, rtol=1e-14, atol=0)
    emu = (torch.nn.functional.silu(Gt.float()) * U.float()
           * es[perm][:, None]).to(torch.bfloat16)
    assert float(MR.ratio(emu, r).max()) <= 1.0
    bad = (torch.nn.functional.silu(Gt.float()) * U.float()
           * es[:, None]).to(torch.bfloat16)           # escale[s], not [perm]
    assert float(MR.ratio(bad, r).max()) > 1.0


# ---------------------------------------------------------------------------
# exact one-hot slabs
@pytest.mark.parametrize("RB", sorted(MR.KC_OF_RB))
def test_exact_slabs(RB):
    K, n_e, M = MR.one_hot_K(RB), 2, MR.M_ROWS
    assert K == 3 * MR.KC_OF_RB[RB] + 32 and MR.n_chunks(K, RB) == 4
    assert -(-K // MR.B_OF_RB[RB]) <= 98
    w = MR.exact_bf16_slab(n_e, M, K, salt=5).float()
    assert bool(torch.isfinite(w).all())
    for m in (0, M - 1):
        assert w[1, m].unique().numel() == K
    rel = (w[..., 1:].abs() / w[..., :-1].abs())
    assert bool(((rel > 1.1) | (rel < 1 / 1.1)).all())
    assert not torch.equal(MR.swap_chunks_1_2(w, RB), w)
    s8 = MR.exact_fp8_slab(n_e, M, K, 17)
    deq = R.fp8_decode(s8.q) * s8.scale[..., None]
    assert torch.equal(s8.dequant_bf16().float(), deq)
    assert bool((deq[..., 1:] != deq[..., :-1]).all())
    # every position of the swapped chunks holds another value
    sw = MR.swap_chunks_1_2(deq, RB)
    KC = MR.KC_OF_RB[RB]
    assert bool((sw[..., KC:KC + 32] != deq[..., KC:KC + 32]).any(-1).all())
