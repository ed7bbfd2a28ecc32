"""GPU: grouped MoE decode on MXFP4 expert slabs.  moe_group_swiglu_mxfp4 /
moe_group_down_mxfp4 against the fp32 reference of test_group_moe_gpu on the
dequantized slabs (quantization error is not in the budget), the fp4 decode
bit for bit against the bf16 kernels, group independence and untouched rows,
and GroupDecodeEngine with MDI_WEIGHT_DTYPE=mxfp4 on a MoE stage.

Geometry under test: B <= 16 runs KC = 1024, larger groups KC = 512; an
expert with more than 64 tokens (B = 128, same_two) takes two column passes."""

import copy
import math

import pytest
import torch

import test_group_moe_gpu as G
from mdi_llm_amd.ops.engine import (dequantize_mxfp4, quantize_mxfp4,
                                    quantize_mxfp4_slab)

pytestmark = pytest.mark.gpu
DEV, BF, SENTINEL = G.DEV, torch.bfloat16, G.SENTINEL


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def deq(q, s, K):
    """The bf16 slab the packed one stands for (e2m1 * 2^e is exact)."""
    return torch.stack([dequantize_mxfp4(q[e], s[e], K)
                        for e in range(q.size(0))]).to(BF)


@pytest.fixture(scope="module")
def slabs():
    """(E, I, n_e) -> packed gate, up, down slabs [(q, s), ...] and their
    dequantized bf16 twins."""
    cache = {}

    def get(E, I, n_e):
        if (E, I, n_e) not in cache:
            g = torch.Generator().manual_seed(1000 + E + I + n_e)
            Q = [quantize_mxfp4_slab(G.mk(n_e, M, K, scale=1 / math.sqrt(K),
                                          gen=g))
                 for M, K in ((I, E), (I, E), (E, I))]
            cache[(E, I, n_e)] = Q, [deq(q, s, K) for (q, s), K
                                     in zip(Q, (E, E, I))]
        return cache[(E, I, n_e)]

    return get


def run_mx(ops, r, X, res, Q, k, count=None):
    """swiglu -> down -> combine on a routing `r`, ACT/D pre-filled with a
    sentinel (G.run_moe on the packed slabs)."""
    (gq, gs), (uq, us), (dq, ds) = Q
    B, E = X.shape
    cnt = r["count"] if count is None else count
    ACT = torch.full((B * k, gq.size(1)), SENTINEL, device=DEV, dtype=BF)
    D = torch.full((B * k, E), SENTINEL, device=DEV)
    out = torch.empty_like(res)
    ops.moe_group_swiglu_mxfp4(ACT, gq, gs, uq, us, X, cnt, r["offset"],
                               r["perm"], r["escale"], k)
    ops.moe_group_down_mxfp4(D, dq, ds, ACT, cnt, r["offset"], B)
    ops.moe_group_combine(out, res, D, r["inv"], k)
    return ACT, D, out


def close(a, b):
    return torch.allclose(a.float(), b, **G.TOL)


# ---------------------------------------------------------------------------
# 1. expert GEMMs against the reference on the dequantized slabs
# ---------------------------------------------------------------------------
CASES = [
    # (E, I, n_e, k, B, routing); K = 224 is 7 blocks: a partial super-step
    (256, 224, 4, 2, 1, "random"),
    (256, 224, 4, 2, 17, "random"),
    (256, 224, 4, 2, 33, "random"),
    (256, 224, 4, 2, 128, "same_two"),   # 128 tokens each: two column passes
    (256, 224, 4, 2, 17, "starved"),     # one expert with count 0
    (256, 224, 4, 1, 33, "all_to_one"),
    # ring reload at ci + 2 and a ragged last chunk in both forms:
    # K = 2080 / 3104 is 3 / 4 chunks of 1024 (B = 3), 5 / 7 of 512 (B = 17)
    (2080, 3104, 2, 2, 3, "random"),
    (2080, 3104, 2, 2, 17, "random"),
]


@pytest.mark.parametrize("E,I,n_e,k,B,routing", CASES)
def test_expert_gemms_mxfp4(ops, slabs, E, I, n_e, k, B, routing):
    Q, W = slabs(E, I, n_e)
    g = torch.Generator().manual_seed(300 + B)
    X, res = G.mk(B, E, gen=g), G.mk(B, E, gen=g)
    logits = G.case_logits(B, n_e, routing)
    G.assert_distinct(logits)
    r = G.route(ops, logits, k)
    cnt = r["count"].cpu().tolist()
    assert routing != "same_two" or cnt == [0, B, 0, B]
    assert routing != "starved" or cnt[2] == 0

    ACT, D, out = run_mx(ops, r, X, res, Q, k)
    ref = G.reference(r, logits, X, res, *W, k, ACT)
    for name, got, want in zip(("ACT", "D", "out"), (ACT, D, out), ref):
        err = float((got.float() - want).abs().max())
        print(f"{name} E={E} I={I} B={B} {routing}: max|err|={err:.4g} "
              f"(max|ref|={float(want.abs().max()):.3g})")
        assert close(got, want), (name, err)

    # teeth: the neighbouring expert's slabs, and every block scale read as
    # 2^0, must fail the same tolerance
    flat = [deq(q, torch.full_like(s, 127), K)
            for (q, s), K in zip(Q, (E, E, I))]
    for bad in (G.reference(r, logits, X, res, *W, k, ACT, rot=1),
                G.reference(r, logits, X, res, *flat, k, ACT)):
        assert not close(ACT, bad[0]) and not close(D, bad[1])

    # determinism: a second launch is bit-identical
    for a, b in zip((ACT, D, out), run_mx(ops, r, X, res, Q, k)):
        assert torch.equal(a, b)


def test_down_mxfp4_scale_index_wraps(ops):
    """K = 8256 is 258 blocks: the scale index crosses the 256-block wrap of
    the stored layout (17 chunks of 512)."""
    n_e, M, K, B = 2, 32, 8256, 17
    g = torch.Generator().manual_seed(77)
    q, s = quantize_mxfp4_slab(G.mk(n_e, M, K, scale=1 / math.sqrt(K), gen=g))
    ACT = G.mk(B, K, gen=g)
    r = G.route(ops, G.case_logits(B, n_e, "random"), 1)
    assert min(r["count"].cpu().tolist()) > 0
    D = torch.full((B, M), SENTINEL, device=DEV)
    ops.moe_group_down_mxfp4(D, q, s, ACT, r["count"], r["offset"], B)
    ex = torch.repeat_interleave(torch.arange(n_e, device=DEV),
                                 r["count"].long())

    def ref(W, rot=0):
        return torch.einsum("sk,smk->sm", ACT.float(),
                            W.float()[(ex + rot) % n_e])

    print(f"down K={K}: max|err|={float((D - ref(deq(q, s, K))).abs().max())}")
    assert close(D, ref(deq(q, s, K)))
    assert not close(D, ref(deq(q, s, K), rot=1))
    assert not close(D, ref(deq(q, torch.full_like(s, 127), K)))


def test_shape_guards_mxfp4(ops):
    """K % 32 != 0 and a mis-shaped scale tensor are refused by both ops."""
    n_e, k, B, M = 4, 2, 3, 256
    r = G.route(ops, G.tie_free_logits(B, n_e, seed=1), k)
    ACT = torch.zeros(B * k, M, device=DEV, dtype=BF)
    D = torch.zeros(B * k, M, device=DEV)
    u8 = dict(device=DEV, dtype=torch.uint8)
    for K, nsb, msg in ((208, 28, "K % 32"), (224, 24, "scales")):
        q = torch.zeros(n_e, M, (K + 31) // 32 * 16, **u8)
        s = torch.full((n_e, M, nsb), 127, **u8)
        X = torch.zeros(B, K, device=DEV, dtype=BF)
        with pytest.raises(RuntimeError, match=msg):
            ops.moe_group_swiglu_mxfp4(ACT, q, s, q, s, X, r["count"],
                                       r["offset"], r["perm"], r["escale"], k)
        with pytest.raises(RuntimeError, match=msg):
            ops.moe_group_down_mxfp4(D, q, s, X.repeat(k, 1), r["count"],
                                     r["offset"], B)


# ---------------------------------------------------------------------------
# 2. the fp4 decode is exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 64, 128])
def test_one_hot_matches_bf16_kernels(ops, B):
    """All 16 e2m1 codes varying along k and rows, block scales 2^-7..2^3:
    the dequantized value is exact in bf16 and a one-hot token makes every
    dot product a single term, so the mxfp4 kernels must equal the bf16
    kernels on the dequantized slabs bit for bit (gate, silu input and up
    included).  A slab with the nibbles of every byte swapped must not."""
    n_e, M, K, k = 4, 256, 256, 1
    e_, m_, k_ = (torch.arange(n)[sh] for n, sh in (
        (n_e, (slice(None), None, None)), (M, (None, slice(None), None)),
        (K, (None, None, slice(None)))))

    def slab(step):
        code = ((m_ * 3 + step * k_ + 11 * e_) % 16).to(torch.uint8)
        q = (code[..., 0::2] | (code[..., 1::2] << 4)).contiguous()
        s = torch.full((n_e, M, 32), 127, dtype=torch.uint8)
        # K / 32 = 8 blocks <= 64: block c's scale is byte 0 of dword c
        s[..., 0::4] = (120 + (m_ + k_[..., :8] * step + e_) % 11).to(
            torch.uint8)
        d = deq(q, s, K)
        assert d.float().unique().numel() > 40
        return q.to(DEV), s.to(DEV), d.to(DEV)

    gq, gs, gd = slab(5)
    uq, us, ud = slab(7)
    dq, ds, dd = slab(9)
    r = G.route(ops, G.all_to_one_logits(B, n_e), k)
    rt = (r["count"], r["offset"], r["perm"], r["escale"], k)
    for shift in range(0, K, B):
        X = torch.zeros(B, K, dtype=BF)
        X[torch.arange(B), (torch.arange(B) + shift) % K] = 1.0
        X = X.to(DEV)
        a4, a, bad = (torch.full((B, M), SENTINEL, device=DEV, dtype=BF)
                      for _ in range(3))
        ops.moe_group_swiglu_mxfp4(a4, gq, gs, uq, us, X, *rt)
        ops.moe_group_swiglu(a, gd, ud, X, *rt)
        assert torch.equal(a4, a), (B, shift)
        ops.moe_group_swiglu_mxfp4(bad, gq, gs, (uq >> 4) | (uq << 4), us, X,
                                   *rt)
        assert not torch.equal(bad, a)
        D4 = torch.full((B, M), SENTINEL, device=DEV)
        D = D4.clone()
        ops.moe_group_down_mxfp4(D4, dq, ds, X, r["count"], r["offset"], B)
        ops.moe_group_down(D, dd, X, r["count"], r["offset"], B)
        assert torch.equal(D4, D), (B, shift)


# ---------------------------------------------------------------------------
# 3. group independence and untouched rows
# ---------------------------------------------------------------------------
def test_group_independence_and_untouched_rows(ops, slabs):
    E, I, n_e, k, B = 256, 224, 4, 2, 33
    Q, _ = slabs(E, I, n_e)
    g = torch.Generator().manual_seed(500 + B)
    X, res = G.mk(B, E, gen=g), G.mk(B, E, gen=g)
    logits = G.tie_free_logits(B, n_e, seed=600 + B)
    p = torch.randperm(B, generator=g)
    assert not torch.equal(p, torch.arange(B))
    pd = p.to(DEV)
    r1, r2 = G.route(ops, logits, k), G.route(ops, logits[p], k)
    ACT1, D1, out1 = run_mx(ops, r1, X, res, Q, k)
    ACT2, D2, out2 = run_mx(ops, r2, X[pd].contiguous(),
                            res[pd].contiguous(), Q, k)
    assert torch.equal(out2, out1[pd])
    inv1, inv2 = (r["inv"].long().view(B, k) for r in (r1, r2))
    for j in range(k):
        assert torch.equal(ACT2[inv2[:, j]], ACT1[inv1[pd, j]])
        assert torch.equal(D2[inv2[:, j]], D1[inv1[pd, j]])

    # one live expert's count set to 0, another's shortened by 2: exactly
    # those rows keep the sentinel, all others equal the full launch
    cnt, off = r1["count"].cpu(), r1["offset"].cpu()
    assert not bool((ACT1.float() == SENTINEL).any() or (D1 == SENTINEL).any())
    live = [e for e in range(n_e) if int(cnt[e]) > 2]
    dead, short = live[0], live[-1]
    assert dead != short
    doctored = cnt.clone()
    doctored[dead] = 0
    doctored[short] -= 2
    ACT, D, _ = run_mx(ops, r1, X, res, Q, k, count=doctored.to(DEV))
    mask = torch.zeros(B * k, dtype=torch.bool)
    mask[int(off[dead]):int(off[dead + 1])] = True
    mask[int(off[short + 1]) - 2:int(off[short + 1])] = True
    mask = mask.to(DEV)
    assert bool((ACT[mask].float() == SENTINEL).all())
    assert bool((D[mask] == SENTINEL).all())
    assert torch.equal(ACT[~mask], ACT1[~mask])
    assert torch.equal(D[~mask], D1[~mask])


# ---------------------------------------------------------------------------
# 4. engine
# ---------------------------------------------------------------------------
# Chosen with the torch models alone, on the CPU: of seeds 0..63 the one with
# the largest minimum k-th/(k+1)-th gate-logit gap over this schedule (bf16
# model and the model holding the dequantized experts): seed 40, gap 0.0246.
ENGINE_SEED = 40


class _RouteSpy:
    """Stands in for the ops module of a GroupDecodeEngine and records the
    gate logits [B, n_e] each MoE layer hands to the router."""

    def __init__(self, real):
        self._real, self.logits = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def moe_route_group(self, *a):
        self.logits.append(a[6].float().clone())
        return self._real.moe_route_group(*a)


def test_group_engine_moe_mxfp4(monkeypatch):
    """Construction (warning, flags, one packed copy shared with the single-
    sample engine), graph vs eager over 8 teacher-forced greedy steps, and
    the distance to the torch model holding the dequantized experts against
    twice the bf16 grouped engine's distance to the bf16 torch model (the
    factor of test_mxfp4_gpu / test_moe_fp8_gpu), with routing off any tie.
    Measured on MI355X: see profiles/group_moe_mxfp4.md."""
    from mdi_llm_amd.ops.engine import DecodeEngine
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    B, gkw = len(G.PROMPT_LENS), dict(n_chunks=8, use_graphs=False)
    cfg, m = G._build(seed=ENGINE_SEED)
    _, mq = G._build(seed=ENGINE_SEED)
    k = cfg.n_expert_per_token
    sg, se, sb = (G._starter(cfg, m, B) for _ in range(3))
    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "mxfp4")
    with pytest.warns(UserWarning, match="mxfp4 applies to the expert GEMMs; "
                      "only the dense GEMMs"):
        eng_g = GroupDecodeEngine(sg, sg.kv_pool, B, n_chunks=8)
    eng_e = GroupDecodeEngine(se, se.kv_pool, B, **gkw)
    eng1 = DecodeEngine(se, se.kv_pool, **gkw)
    monkeypatch.delenv("MDI_WEIGHT_DTYPE")
    eng_b = GroupDecodeEngine(sb, sb.kv_pool, B, **gkw)
    assert eng_e.moe_mxfp4 and not eng_e.mxfp4 and not eng_b.moe_mxfp4
    w0 = eng_e.blocks[0]
    assert w0.fc1_wmx.dim() == 3 and w0.fc1_wmx.dtype == torch.uint8
    assert not hasattr(w0, "attn_wmx")
    for w1, wg in zip(eng1.blocks, eng_e.blocks):
        for n in ("fc1", "fc2", "mlp_proj"):
            for suf in ("_wmx", "_smx"):
                assert getattr(w1, n + suf).data_ptr() == \
                    getattr(wg, n + suf).data_ptr(), n + suf

    with torch.inference_mode():
        eng_g.ensure_graphs(0.0, 0, 0)  # greedy; before prefill
        toks, pos = [], []
        for mm in (m, mq):
            mm.set_kv_cache(B)
        for s, p in enumerate(G._prompts(ENGINE_SEED + 1)):
            m(p.view(1, -1), input_pos=0, slot=s)
            ref = mq(p.view(1, -1), input_pos=0, slot=s)
            toks.append(int(ref[0, -1].float().argmax()))
            pos.append(p.numel())
            for st, eng in ((sg, eng_g), (se, eng_e), (sb, eng_b)):
                st.forward_head(p.view(1, -1), slot=s, input_pos=0)
                eng.set_slot_pos(s, p.numel())
        sd = copy.deepcopy(mq.state_dict())  # the experts, dequantized
        for name in [n for n in sd if ".mlp.experts." in n]:
            sd[name] = dequantize_mxfp4(*quantize_mxfp4(sd[name]),
                                        sd[name].size(1)).to(BF)
        mq.load_state_dict(sd)
        gates = {id(mm): [] for mm in (m, mq)}
        for mm in (m, mq):
            for blk in mm.transformer.h:
                blk.mlp.gate.register_forward_hook(
                    lambda _m, _i, out, L=gates[id(mm)]: L.append(
                        out.float().view(-1).clone()))
        eng_e.ops, eng_b.ops = _RouteSpy(eng_e.ops), _RouteSpy(eng_b.ops)

        slots = torch.arange(B, device=DEV, dtype=torch.int32)
        worst, min_gap, max_dev = 0.0, float("inf"), 0.0
        for step in range(G.N_STEPS):
            out = []
            for eng in (eng_g, eng_e, eng_b):
                eng.token_table.copy_(torch.tensor(toks, dtype=torch.int32))
                eng.set_group(slots)
            eng_g.standalone_step()
            got = eng_g.token_table.clone()
            for eng in (eng_e, eng_b):
                eng.ops.logits.clear()
                eng.head_step()
                eng._tail_seq()
                out.append(eng.LOGITS.float().clone())
            # the graph's greedy pick is a maximum of the eager logits
            picked = out[0].gather(1, got.long().view(B, 1)).view(B)
            assert torch.equal(picked, out[0].max(dim=1).values), (step, got)
            for s in range(B):
                t = torch.tensor([[toks[s]]], device=DEV)
                refs = []
                for mm, eng in ((mq, eng_e), (m, eng_b)):
                    gates[id(mm)].clear()
                    refs.append(mm(t, input_pos=pos[s], slot=s)[0, -1].float())
                    assert len(gates[id(mm)]) == len(eng.ops.logits)
                    for tg, eg in zip(gates[id(mm)], eng.ops.logits):
                        srt = tg.sort(descending=True).values
                        gap = float(srt[k - 1] - srt[k])
                        dev = float((eg[s] - tg).abs().max())
                        min_gap, max_dev = min(min_gap, gap), max(max_dev, dev)
                        assert gap > dev, ("precondition: routing near-tied "
                                           "in the torch reference", step, s)
                rel, base = G._rel(out[0][s], refs[0]), G._rel(out[1][s],
                                                               refs[1])
                worst = max(worst, rel / base)
                print(f"step {step} slot {s}: mxfp4 rel={rel:.5f} "
                      f"bf16 base={base:.5f}")
                assert rel <= 2 * base, (step, s, rel, base)
                toks[s] = int(refs[0].argmax())
                pos[s] += 1
        print(f"worst rel/base={worst:.3f}; min gate gap={min_gap:.4g}, "
              f"max engine gate deviation={max_dev:.4g}")
