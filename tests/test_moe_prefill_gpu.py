"""GPU: HIP prefill for MoE stages — the any-length router
(moe_route_prefill), the row kernels of the expert-major path
(moe_prefill_gather / moe_prefill_act / moe_prefill_combine), the MoE MLP
half of DecodeEngine.prefill_hidden on both of its paths, and the engine on
nano-moe-gpu against the torch stage forward.

Helpers, logits, tolerance and the fp32 reference come from
test_group_moe_gpu (imported, not copied); the layout convention is the one
stated there."""

from types import SimpleNamespace

import pytest
import torch

import test_group_moe_gpu as G

pytestmark = pytest.mark.gpu

DEV = G.DEV
BF = torch.bfloat16
SENTINEL = G.SENTINEL
ULP = dict(rtol=2.0 ** -7, atol=0.0)  # one bf16 ulp, see test_combine
E, I, N_E, K = 256, 224, 4, 2          # nano-moe-gpu sized

# Chosen with the torch model alone: a CPU run over seeds 0..63 of exactly
# the schedule of the engine tests below (model seed s, prompt seed s+1, 24
# prompt tokens + one greedy decode step, bf16 stage against the fp32 one).
# Among the seeds whose top-2 logit gap exceeds 0.1 both after the prompt
# and after the decode step, seed 1 has the largest minimum gap between the
# k-th and (k+1)-th gate logit: 0.0216, against a largest bf16 gate-logit
# deviation of 0.0039; top-2 gaps 0.225 / 0.258 against logit deviations of
# 0.008 / 0.006.
ENGINE_SEED = 1
PROMPT_T = 24


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def route_prefill(ops, logits, k):
    T, n_e = logits.shape
    i32 = dict(device=DEV, dtype=torch.int32)
    r = dict(
        eidx=torch.full((T * k,), -1, **i32),
        escale=torch.full((T * k,), -1.0, device=DEV),
        count=torch.full((n_e,), -1, **i32),
        offset=torch.full((n_e + 1,), -1, **i32),
        perm=torch.full((T * k,), -1, **i32),
        inv=torch.full((T * k,), -1, **i32),
    )
    ops.moe_route_prefill(r["eidx"], r["escale"], r["count"], r["offset"],
                          r["perm"], r["inv"], logits.to(DEV).contiguous(), k)
    return r


def check_router_prefill(ops, logits, k):
    """G.check_router's assertions on moe_route_prefill."""
    G.assert_distinct(logits)
    T, n_e = logits.shape
    r = route_prefill(ops, logits, k)
    top = torch.topk(logits.float(), k, dim=1)
    assert torch.equal(r["eidx"].cpu().view(T, k).long(), top.indices)
    ref_scale = torch.softmax(top.values, dim=1)
    got = r["escale"].cpu().view(T, k)
    err = ((got - ref_scale).abs() / ref_scale).max()
    print(f"prefill router T={T} n_e={n_e} k={k}: max rel escale "
          f"err={float(err):.3g}")
    assert torch.allclose(got, ref_scale, rtol=G.ESCALE_RTOL, atol=0.0)
    count, offset, perm, inv = G.cpu_layout(top.indices.reshape(-1), n_e)
    assert torch.equal(r["count"].cpu().long(), count)
    assert torch.equal(r["offset"].cpu().long(), offset)
    assert torch.equal(r["perm"].cpu().long(), perm)
    assert torch.equal(r["inv"].cpu().long(), inv)
    return r


def same(r1, r2):
    return all(torch.equal(r1[n], r2[n]) for n in r1)


# ---------------------------------------------------------------------------
# 1. router
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_e,k", [(1, 4, 2), (129, 4, 2), (300, 8, 2),
                                     (1000, 64, 8)])
def test_router_exact(ops, T, n_e, k):
    logits = G.tie_free_logits(T, n_e, seed=100 + T)
    r = check_router_prefill(ops, logits, k)
    # determinism: a second launch is bit-identical
    assert same(r, route_prefill(ops, logits, k))


def test_router_all_to_one(ops):
    r = check_router_prefill(ops, G.all_to_one_logits(300, 4), 1)
    assert r["count"].cpu().tolist() == [0, 300, 0, 0]


def test_router_same_two(ops):
    r = check_router_prefill(ops, G.same_two_logits(300, 8), 2)
    assert r["count"].cpu().tolist() == [0, 300, 0, 300, 0, 0, 0, 0]


def test_router_starved(ops):
    r = check_router_prefill(ops, G.one_starved_logits(300, 4, seed=3), 2)
    cnt = r["count"].cpu().tolist()
    assert cnt[2] == 0 and sum(cnt) == 600


@pytest.mark.parametrize("T,n_e,k", [(5, 8, 2), (128, 64, 8)])
def test_router_agrees_with_group_router(ops, T, n_e, k):
    """All six outputs equal moe_route_group's bit for bit (escale too: the
    per-token step is one shared device function)."""
    logits = G.tie_free_logits(T, n_e, seed=700 + T)
    rp, rg = route_prefill(ops, logits, k), G.route(ops, logits, k)
    for name in rp:
        assert torch.equal(rp[name], rg[name]), name


def test_router_largest_size(ops):
    """T*k at the cap of 65536 pairs: 64 segments per expert.  The layout
    reference is a stable sort of the pairs by expert (ascending f inside an
    expert), which is what G.cpu_layout builds pair by pair."""
    T, n_e, k = 32768, 8, 2
    g = torch.Generator().manual_seed(5)
    vals = (torch.arange(n_e, dtype=torch.float32) - n_e // 2) * 0.25
    logits = vals[torch.rand(T, n_e, generator=g).argsort(dim=1)].to(BF)
    G.assert_distinct(logits)
    r = route_prefill(ops, logits, k)
    top = torch.topk(logits.float(), k, dim=1)
    e = top.indices.reshape(-1)
    assert torch.equal(r["eidx"].cpu().long(), e)
    count = torch.bincount(e, minlength=n_e)
    perm = torch.argsort(e, stable=True)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    assert torch.equal(r["count"].cpu().long(), count)
    assert r["offset"].cpu().tolist() == [0] + count.cumsum(0).tolist()
    assert torch.equal(r["perm"].cpu().long(), perm)
    assert torch.equal(r["inv"].cpu().long(), inv)
    assert same(r, route_prefill(ops, logits, k))


def test_router_refuses_bad_arguments(ops):
    def call(T, n_e, k, dtype=BF, n_out=None):
        n = T * k if n_out is None else n_out
        i32 = dict(device=DEV, dtype=torch.int32)
        ops.moe_route_prefill(
            torch.zeros(n, **i32), torch.zeros(n, device=DEV),
            torch.zeros(n_e, **i32), torch.zeros(n_e + 1, **i32),
            torch.zeros(n, **i32), torch.zeros(n, **i32),
            torch.zeros(T, n_e, device=DEV, dtype=dtype), k)

    call(3, 4, 2)  # the well-formed call passes
    with pytest.raises(RuntimeError, match="bf16"):
        call(3, 4, 2, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="65536"):
        call(32769, 4, 2)
    with pytest.raises(RuntimeError, match="n_e <= 64"):
        call(3, 65, 2)
    with pytest.raises(RuntimeError, match="k <= min"):
        call(3, 16, 9)
    with pytest.raises(RuntimeError, match="k <= min"):
        call(3, 4, 5)
    with pytest.raises(RuntimeError, match="perm"):
        ops.moe_route_prefill(
            torch.zeros(6, device=DEV, dtype=torch.int32),
            torch.zeros(6, device=DEV),
            torch.zeros(4, device=DEV, dtype=torch.int32),
            torch.zeros(5, device=DEV, dtype=torch.int32),
            torch.zeros(5, device=DEV, dtype=torch.int32),
            torch.zeros(6, device=DEV, dtype=torch.int32),
            torch.zeros(3, 4, device=DEV, dtype=BF), 2)


# ---------------------------------------------------------------------------
# 2. row kernels
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def routed(ops):
    """One routing of 300 tokens shared by the row-kernel tests."""
    return route_prefill(ops, G.tie_free_logits(300, N_E, seed=11), K)


@pytest.mark.parametrize("width", [E, 2056])  # 2056: a second, ragged block
def test_gather(ops, routed, width):
    T = 300
    hn = G.mk(T, width, gen=torch.Generator().manual_seed(12))
    XG = torch.full((T * K, width), SENTINEL, device=DEV, dtype=BF)
    ops.moe_prefill_gather(XG, hn, routed["perm"], K)
    assert torch.equal(XG, hn[routed["perm"].long() // K])


@pytest.mark.parametrize("width", [E, 2056])
def test_combine(ops, routed, width):
    """The fp32 rank-ordered sum is evaluated far below half a bf16 ulp, so
    the kernel's bf16 is the correctly rounded value or its neighbour:
    relative error at most one ulp, 2^-7."""
    T = 300
    g = torch.Generator().manual_seed(13)
    res, D = G.mk(T, width, gen=g), G.mk(T * K, width, gen=g)
    inv = routed["inv"].long().view(T, K)
    ref = res.float()
    for j in range(K):
        ref = ref + D.float()[inv[:, j]]
    out = torch.empty_like(res)
    ops.moe_prefill_combine(out, res, D, routed["inv"], K)
    assert torch.allclose(out.float(), ref, **ULP)
    aliased = res.clone()
    ops.moe_prefill_combine(aliased, aliased, D, routed["inv"], K)
    assert torch.equal(aliased, out)


@pytest.mark.parametrize("width", [I, 2056])
def test_act(ops, routed, width):
    g = torch.Generator().manual_seed(14)
    n = 300 * K
    Gt, U = G.mk(n, width, gen=g), G.mk(n, width, gen=g)
    scale = routed["escale"][routed["perm"].long()]
    ref = torch.nn.functional.silu(Gt.float()) * U.float() * scale[:, None]
    ACT = torch.empty_like(Gt)
    ops.moe_prefill_act(ACT, Gt, U, routed["escale"], routed["perm"])
    assert torch.allclose(ACT.float(), ref, **ULP)


def test_row_kernels_refuse_bad_shapes(ops, routed):
    n = 300 * K
    with pytest.raises(RuntimeError, match="E % 8"):
        ops.moe_prefill_gather(
            torch.zeros(n, 100, device=DEV, dtype=BF),
            torch.zeros(300, 100, device=DEV, dtype=BF), routed["perm"], K)
    with pytest.raises(RuntimeError, match="fp32|bf16"):
        ops.moe_prefill_combine(
            torch.zeros(300, E, device=DEV, dtype=BF),
            torch.zeros(300, E, device=DEV, dtype=BF),
            torch.zeros(n, E, device=DEV), routed["inv"], K)
    with pytest.raises(RuntimeError, match="ACT"):
        ops.moe_prefill_act(
            torch.zeros(n - 1, I, device=DEV, dtype=BF),
            torch.zeros(n, I, device=DEV, dtype=BF),
            torch.zeros(n, I, device=DEV, dtype=BF), routed["escale"],
            routed["perm"])


# ---------------------------------------------------------------------------
# 3. the MoE MLP half of the prefill, both paths
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    """A DecodeEngine on nano-moe-gpu; the MLP-half tests hand it their own
    expert slabs."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, m = G._build(seed=0)
    assert (cfg.n_embd, cfg.intermediate_size, cfg.n_expert,
            cfg.n_expert_per_token) == (E, I, N_E, K)
    stage = G._starter(cfg, m, 1)
    return DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)


@pytest.fixture(scope="module")
def slabs():
    import math

    g = torch.Generator().manual_seed(1000 + E + I + N_E)
    Wg = G.mk(N_E, I, E, scale=1 / math.sqrt(E), gen=g)
    Wu = G.mk(N_E, I, E, scale=1 / math.sqrt(E), gen=g)
    Wd = G.mk(N_E, E, I, scale=1 / math.sqrt(I), gen=g)
    return Wg, Wu, Wd


def run_half(engine, slabs, r, X, res, group_max):
    """moe_prefill_experts on the path group_max selects; ACT/D pre-filled
    with a sentinel (D fp32 on the grouped path, bf16 on the other)."""
    Wg, Wu, Wd = slabs
    T = X.size(0)
    grouped = T <= min(group_max, 128)
    w = SimpleNamespace(fc1_w=Wg, fc2_w=Wu, mlp_proj_w=Wd)
    ACT = torch.full((T * K, I), SENTINEL, device=DEV, dtype=BF)
    D = torch.full((T * K, E), SENTINEL, device=DEV,
                   dtype=torch.float32 if grouped else BF)
    out = torch.empty_like(res)
    engine.moe_prefill_group_max = group_max
    engine.moe_prefill_experts(out, res, X, w, r, ACT=ACT, D=D)
    return ACT, D, out


@pytest.fixture(scope="module")
def half_case(ops):
    cache = {}

    def get(T):
        if T not in cache:
            g = torch.Generator().manual_seed(300 + T)
            X, res = G.mk(T, E, gen=g), G.mk(T, E, gen=g)
            logits = G.tie_free_logits(T, N_E, seed=200 + T)
            cache[T] = (X, res, logits, route_prefill(ops, logits, K))
        return cache[T]

    return get


@pytest.mark.parametrize("group_max", [128, 0])
@pytest.mark.parametrize("T", [3, 128, 129, 300])
def test_mlp_half(engine, slabs, half_case, T, group_max):
    Wg, Wu, Wd = slabs
    X, res, logits, r = half_case(T)
    ACT, D, out = run_half(engine, slabs, r, X, res, group_max)
    assert D.dtype == (torch.float32 if T <= group_max else BF)
    act_ref, d_ref, out_ref = G.reference(r, logits, X, res, Wg, Wu, Wd, K,
                                          ACT)
    for name, got, ref in (("ACT", ACT, act_ref), ("D", D, d_ref),
                           ("out", out, out_ref)):
        err = (got.float() - ref).abs().max()
        print(f"{name} T={T} group_max={group_max}: max|err|="
              f"{float(err):.4g} (max|ref|={float(ref.abs().max()):.3g})")
        assert torch.allclose(got.float(), ref, **G.TOL), (name, float(err))
    # teeth: the neighbouring expert's slabs must fail the same tolerance
    act_rot, d_rot, out_rot = G.reference(r, logits, X, res, Wg, Wu, Wd, K,
                                          ACT, rot=1)
    assert not torch.allclose(ACT.float(), act_rot, **G.TOL)
    assert not torch.allclose(D.float(), d_rot, **G.TOL)
    assert not torch.allclose(out.float(), out_rot, **G.TOL)


def test_mlp_half_paths_agree(engine, slabs, half_case):
    """The two paths round to bf16 in different places (D is fp32 on the
    grouped one), so they agree within G.TOL, not bit for bit."""
    X, res, _, r = half_case(128)
    _, _, out_g = run_half(engine, slabs, r, X, res, 128)
    _, _, out_e = run_half(engine, slabs, r, X, res, 0)
    err = (out_g.float() - out_e.float()).abs().max()
    print(f"grouped vs expert-major at T=128: max|diff|={float(err):.4g}")
    assert torch.allclose(out_g.float(), out_e.float(), **G.TOL)


@pytest.mark.parametrize("T,group_max", [(33, 128), (300, 0)])
def test_rows_past_the_layout_keep_sentinel(engine, slabs, half_case, ops, T,
                                            group_max):
    """Rows of ACT and D at and beyond offset[n_e] are never written.  A
    complete routing has none, so the last two rows are cut off the layout:
    offset[n_e] and the last expert's count drop by two, and the two pairs
    lose their perm / inv entries."""
    X, res = half_case(300)[0][:T].contiguous(), half_case(300)[1][:T]
    res = res.contiguous()
    r = route_prefill(ops, G.tie_free_logits(T, N_E, seed=400 + T), K)
    n = T * K
    assert int(r["count"][N_E - 1]) > 2
    full_ACT, full_D, _ = run_half(engine, slabs, r, X, res, group_max)
    assert not bool((full_ACT.float() == SENTINEL).any())
    assert not bool((full_D.float() == SENTINEL).any())

    cut = {name: t.clone() for name, t in r.items()}
    lost = cut["perm"][n - 2:].long()
    cut["inv"][lost] = -1
    cut["perm"][n - 2:] = -1
    cut["count"][N_E - 1] -= 2
    cut["offset"][N_E] -= 2
    ACT, D, out = run_half(engine, slabs, cut, X, res, group_max)
    assert bool((ACT[n - 2:].float() == SENTINEL).all())
    assert bool((D[n - 2:].float() == SENTINEL).all())
    # the other experts' rows are what the full launch wrote, bit for bit
    # (the shortened expert's GEMM has another row count, so the library may
    # pick another kernel for it: those rows only within G.TOL)
    lo = int(r["offset"][N_E - 1])
    assert torch.equal(ACT[:lo], full_ACT[:lo])
    assert torch.equal(D[:lo], full_D[:lo])
    assert torch.allclose(D[lo:n - 2].float(), full_D[lo:n - 2].float(),
                          **G.TOL)
    # and the two tokens that lost a pair sum only the rank they kept
    inv = cut["inv"].long().view(T, K)
    ref = res.float()
    for j in range(K):
        ok = inv[:, j] >= 0
        ref[ok] += D.float()[inv[ok, j]]
    assert int((inv < 0).sum()) == 2
    assert torch.allclose(out.float(), ref, **ULP)


# ---------------------------------------------------------------------------
# 4. engine: nano-moe-gpu, a prompt of 24 tokens
# ---------------------------------------------------------------------------
def _stage(cfg, m, dtype, n_slots):
    from mdi_llm_amd.models.stages import StarterStage

    st = StarterStage(cfg, cfg.n_layer).to(device=DEV, dtype=dtype)
    st.load_state_dict(m.state_dict())
    st.eval()
    st.set_kv_cache(n_slots)
    return st


@pytest.fixture(scope="module")
def refs():
    """The fp32 truth and the bf16 torch stage (the yardstick) on the
    prompt and on one greedy decode step, computed once."""
    with torch.inference_mode():
        cfg, m = G._build(seed=ENGINE_SEED)
        g = torch.Generator().manual_seed(ENGINE_SEED + 1)
        prompt = torch.randint(0, 511, (PROMPT_T,), generator=g).to(DEV)
        out = dict(cfg=cfg, m=m, prompt=prompt)
        for name, dtype in (("truth", torch.float32), ("torch", BF)):
            st = _stage(cfg, m, dtype, 1)
            gate = []
            hooks = [b.mlp.gate.register_forward_hook(
                lambda _m, _i, o: gate.append(o.float().clone()))
                for b in st.transformer.h]
            x = st.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
            for h in hooks:
                h.remove()
            logits0 = st.forward_tail(x).view(-1).float()
            tok = int(logits0.argmax())
            st.kv_pool.seq_len[0] = PROMPT_T
            x1 = st.forward_head(torch.tensor([[tok]], device=DEV), slot=0,
                                 input_pos=PROMPT_T)
            out[name] = dict(
                x=x[0].float(), gate=[t.view(-1, cfg.n_expert) for t in gate],
                logits0=logits0, tok=tok,
                logits1=st.forward_tail(x1).view(-1).float(),
                k=st.kv_pool.k[0, :, :, :PROMPT_T].float().clone(),
                v=st.kv_pool.v[0, :, :, :PROMPT_T].float().clone())
        return out


def test_reference_preconditions(refs):
    """On the references alone: no near-tied routing and no near-tied
    greedy pick, so that an honest bf16 pipeline cannot legitimately flip
    either.  Measured on MI355X: minimum gate gap 0.0216 against a largest
    bf16 gate deviation of 0.0039; top-2 gaps 0.225 / 0.258 against logit
    deviations of 0.0080 / 0.0059."""
    t, b = refs["truth"], refs["torch"]
    k = refs["cfg"].n_expert_per_token
    assert len(t["gate"]) == len(b["gate"]) == refs["cfg"].n_layer
    min_gap, max_dev = float("inf"), 0.0
    for tg, bg in zip(t["gate"], b["gate"]):
        srt = tg.sort(dim=1, descending=True).values
        gap = srt[:, k - 1] - srt[:, k]              # per token
        dev = float((bg - tg).abs().max())
        min_gap, max_dev = min(min_gap, float(gap.min())), max(max_dev, dev)
        assert bool((gap > dev).all()), (
            "precondition: routing near-tied in the fp32 truth",
            float(gap.min()), dev)
    print(f"min gate gap={min_gap:.4g}, max bf16 gate deviation={max_dev:.4g}")
    assert t["tok"] == b["tok"]
    for name in ("logits0", "logits1"):
        top = t[name].sort(descending=True).values
        gap = float(top[0] - top[1])
        dev = float((b[name] - t[name]).abs().max())
        print(f"{name}: top-2 gap={gap:.4g}, bf16 logit deviation={dev:.4g}")
        # the HIP path may sit twice as far from the truth as the yardstick
        assert gap > 2 * 2 * dev, (name, gap, dev)
    assert int(b["logits1"].argmax()) == int(t["logits1"].argmax())


@pytest.mark.parametrize("group_max", [128, 0])
@torch.inference_mode()
def test_engine_prefill(refs, group_max):
    """HIP prefill of the prompt on either MoE path: the final hidden stays
    below twice the bf16 torch stage's distance to the fp32 truth (the
    project's margin for the same bf16 pipeline with another fp32
    association), the KV pool matches the torch stage within 0.03
    (test_hip_prefill_matches_torch's figure), one greedy decode step off
    the HIP-filled cache picks the torch stage's token, and a continuation
    at pos0=16 lands where the one-shot prefill does.

    Measured on MI355X (also in profiles/moe_prefill.md): hidden distance
    0.00572 (grouped) / 0.00565 (expert-major) against 0.00646 for the
    torch stage; KV max|diff| 0.0078; continuation KV bit-identical, last
    hidden 0.00580 / 0.00561 against 0.00687."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, m, prompt = refs["cfg"], refs["m"], refs["prompt"]
    t, b = refs["truth"], refs["torch"]
    stage = _stage(cfg, m, BF, 2)
    eng = DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)
    assert eng.supports_hip_prefill
    eng.moe_prefill_group_max = group_max

    x_hip = eng.prefill_prompt(prompt, slot=0, pos0=0).float()
    d_hip, d_ref = G._rel(x_hip, t["x"]), G._rel(b["x"], t["x"])
    print(f"group_max={group_max}: hidden rel to fp32 truth: hip="
          f"{d_hip:.5f} torch bf16={d_ref:.5f}")
    assert d_hip < 2 * d_ref, (d_hip, d_ref)

    pool = stage.kv_pool
    kd = (pool.k[0, :, :, :PROMPT_T].float() - b["k"]).abs().max()
    vd = (pool.v[0, :, :, :PROMPT_T].float() - b["v"]).abs().max()
    print(f"group_max={group_max}: KV max|diff| k={float(kd):.4g} "
          f"v={float(vd):.4g}")
    assert kd < 0.03 and vd < 0.03, (float(kd), float(vd))

    # continuation: 16 tokens, then 8 more at pos0=16, in slot 1
    eng.prefill_prompt(prompt[:16], slot=1, pos0=0)
    x_c = eng.prefill_prompt(prompt[16:], slot=1, pos0=16).float()
    kc = (pool.k[1, :, :, 16:PROMPT_T].float()
          - pool.k[0, :, :, 16:PROMPT_T].float()).abs().max()
    vc = (pool.v[1, :, :, 16:PROMPT_T].float()
          - pool.v[0, :, :, 16:PROMPT_T].float()).abs().max()
    c_hip = G._rel(x_c[-1], t["x"][-1])
    c_ref = G._rel(b["x"][-1], t["x"][-1])
    print(f"group_max={group_max}: continuation KV max|diff| k="
          f"{float(kc):.4g} v={float(vc):.4g}; last hidden rel hip="
          f"{c_hip:.5f} torch bf16={c_ref:.5f}")
    assert kc < 0.03 and vc < 0.03, (float(kc), float(vc))
    assert c_hip < 2 * c_ref, (c_hip, c_ref)

    # greedy decode step off the HIP-prefilled cache (slot 0)
    eng.set_slot_pos(0, PROMPT_T)
    tok = torch.tensor([b["tok"]], device=DEV, dtype=torch.int32)
    logits = eng.tail(eng.decode_step_head(tok, slot=0)).float()
    assert int(logits.argmax()) == int(b["logits1"].argmax())


@torch.inference_mode()
def test_runner_prefills_moe_on_hip(refs):
    """The runner's prefill branches on supports_hip_prefill: on a MoE
    stage it now returns what the engine's prefill returns."""
    from mdi_llm_amd.parallel.runner import make_runner

    cfg, m, prompt = refs["cfg"], refs["m"], refs["prompt"]
    stage = _stage(cfg, m, BF, 1)
    runner = make_runner(stage, 1, torch.device(DEV), use_graphs=False)
    assert runner.backend == "hip" and runner.engine.supports_hip_prefill
    x = runner.prefill_head(prompt, 0)
    x2 = runner.engine.prefill_prompt(prompt, 0, 0)
    assert torch.equal(x.view(-1), x2.view(-1))
    assert int(runner.engine.pos_table[0]) == PROMPT_T
