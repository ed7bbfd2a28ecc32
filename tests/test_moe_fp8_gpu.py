"""GPU: fp8 expert weights for MoE decode — the expert indirection of
gemv_fp8 / gemv_swiglu_fp8, the fp8-slab grouped expert GEMMs
(moe_group_swiglu_fp8 / moe_group_down_fp8), and both engines on
nano-moe-gpu with MDI_WEIGHT_DTYPE=fp8.

Helpers, cases, tolerance and the fp32 reference of the bf16 grouped
kernels come from test_group_moe_gpu (imported, not copied): the fp8
kernels are held to the same figures on the dequantized weights
decode(byte) * scale."""

import copy
import math

import pytest
import torch

import gemv_reference as R
import test_group_moe_gpu as G

pytestmark = pytest.mark.gpu

DEV = G.DEV
BF = torch.bfloat16
SENTINEL = G.SENTINEL
# Chosen with the torch model alone (CPU bf16 run of the schedule of
# test_engine_fp8_moe_logits_vs_torch with the dequantized weights loaded):
# the largest minimum gap between the k-th and (k+1)-th gate logit over
# seeds 0..63.
ENGINE_SEED = 40
PROMPT_LENS = G.PROMPT_LENS
N_STEPS = G.N_STEPS


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def quant_slab(slab):
    """bf16 [n_e,M,K] on DEV -> (fp8, scales, fp32 decode*scale, fp32
    decode alone)."""
    from mdi_llm_amd.ops.engine import quantize_fp8_slab

    q, s = quantize_fp8_slab(slab)
    raw = R.fp8_decode(q.view(torch.uint8))
    return q, s, raw * s[..., None], raw


def i32(vals):
    return torch.tensor(vals, device=DEV, dtype=torch.int32)


def f32(vals):
    return torch.tensor(vals, device=DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------
# 1. expert indirection of the single-sample GEMVs is exact
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gemv_slabs():
    cache = {}

    def get(M, K, n_e=4):
        if (M, K) not in cache:
            g = torch.Generator().manual_seed(2000 + M)
            a = quant_slab(G.mk(n_e, M, K, scale=1 / math.sqrt(K), gen=g))
            b = quant_slab(G.mk(n_e, M, K, scale=1 / math.sqrt(K), gen=g))
            cache[(M, K)] = (a, b, G.mk(K, gen=g), G.mk(M, gen=g))
        return cache[(M, K)]

    return get


@pytest.mark.parametrize("M,K", [(256, 224), (224, 256)])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("epilogue", [0, 1])
def test_gemv_fp8_indirection_exact(ops, gemv_slabs, M, K, rows, epilogue):
    (W8, S, _, _), _, x, res = gemv_slabs(M, K)
    n_e = W8.size(0)
    r = res if epilogue == 1 else None

    def direct(e):
        o = torch.full((M,), SENTINEL, device=DEV, dtype=BF)
        ops.gemv_fp8(o, W8[e].contiguous(), S[e].contiguous(), x, None, r,
                     epilogue, rows=rows)
        return o

    want = [direct(e) for e in range(n_e)]
    for e in range(n_e):
        o = torch.full((M,), SENTINEL, device=DEV, dtype=BF)
        ops.gemv_fp8(o, W8, S, x, None, r, epilogue, rows=rows,
                     eidx=i32([e]), estride=M * K)
        assert torch.equal(o, want[e]), e
        assert not torch.equal(o, want[(e + 1) % n_e]), e  # the teeth
    if epilogue == 1:  # the residual took part
        o = torch.full((M,), SENTINEL, device=DEV, dtype=BF)
        ops.gemv_fp8(o, W8, S, x, None, None, 0, rows=rows, eidx=i32([0]),
                     estride=M * K)
        assert not torch.equal(o, want[0])


@pytest.mark.parametrize("M,K", [(256, 224), (224, 256)])
def test_gemv_swiglu_fp8_indirection_exact(ops, gemv_slabs, M, K):
    (G8, GS, _, _), (U8, US, _, _), x, _ = gemv_slabs(M, K)
    n_e = G8.size(0)

    def run(*w, **kw):
        o = torch.full((M,), SENTINEL, device=DEV, dtype=BF)
        ops.gemv_swiglu_fp8(o, *w, x, False, **kw)
        return o

    want = [run(G8[e].contiguous(), GS[e].contiguous(), U8[e].contiguous(),
                US[e].contiguous()) for e in range(n_e)]
    for e in range(n_e):
        kw = dict(eidx=i32([e]), estride=M * K)
        o = run(G8, GS, U8, US, **kw)
        assert torch.equal(o, want[e]), e
        assert not torch.equal(o, want[(e + 1) % n_e]), e
        assert torch.equal(run(G8, GS, U8, US, escale=f32([1.0]), **kw), o)
        # halving is exact in bf16 away from the subnormals
        ref = o.float()
        assert bool(((ref == 0) | (ref.abs() >= 2.0 ** -120)).all())
        half = run(G8, GS, U8, US, escale=f32([0.5]), **kw)
        assert torch.equal(half.float(), ref * 0.5), e
    # escale also works without the indirection
    assert torch.equal(
        run(G8[1].contiguous(), GS[1].contiguous(), U8[1].contiguous(),
            US[1].contiguous(), escale=f32([0.5])).float(),
        want[1].float() * 0.5)


def test_gemv_fp8_indirection_guards(ops, gemv_slabs):
    M, K = 256, 224
    (W8, S, _, _), _, x, _ = gemv_slabs(M, K)
    o = torch.zeros(M, device=DEV, dtype=BF)
    e = i32([1])
    with pytest.raises(RuntimeError, match="int32"):
        ops.gemv_fp8(o, W8, S, x, None, None, 0, eidx=e.long(),
                     estride=M * K)
    with pytest.raises(RuntimeError, match="empty"):
        ops.gemv_fp8(o, W8, S, x, None, None, 0, eidx=e[:0], estride=M * K)
    with pytest.raises(RuntimeError, match="LayerNorm"):
        ops.gemv_fp8(o, W8, S, x, None, None, 0, x, None, 2, 1e-5, 1,
                     eidx=e, estride=M * K)
    with pytest.raises(RuntimeError, match="wscale"):
        ops.gemv_fp8(o, W8, S[0].contiguous(), x, None, None, 0, eidx=e,
                     estride=M * K)
    with pytest.raises(RuntimeError, match="estride"):
        ops.gemv_fp8(o, W8, S, x, None, None, 0, eidx=e, estride=K)
    with pytest.raises(RuntimeError, match="int32"):
        ops.gemv_swiglu_fp8(o, W8, S, W8, S, x, False, eidx=e.long(),
                            estride=M * K)
    with pytest.raises(RuntimeError, match="LayerNorm"):
        ops.gemv_swiglu_fp8(o, W8, S, W8, S, x, False, x, None, 2, 1e-5,
                            eidx=e, estride=M * K)


# ---------------------------------------------------------------------------
# 2. byte decode of the grouped kernels is exact
# ---------------------------------------------------------------------------
def one_hot_tokens(B, K, shift):
    X = torch.zeros(B, K, dtype=BF)
    X[torch.arange(B), (torch.arange(B) + shift) % K] = 1.0
    return X.to(DEV)


# B=64 is the 16-byte-load path at all 64 k positions; 16 and 128 reach the
# RB=16 instantiation and the 8-byte loads of RB=128
@pytest.mark.parametrize("B", [64, 16, 128])
def test_group_down_fp8_byte_decode_exact(ops, B):
    n_e, M, K, k = 4, 256, 64, 1
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7F == 0x7F] = 0          # the two NaN codes
    Wd = torch.full((n_e, M, K), 0x38, dtype=torch.uint8)   # 1.0 elsewhere
    Wd[1] = codes[:, None].expand(M, K)
    ds = torch.ones(n_e, M)
    ds[1] = 2.0 ** -(torch.arange(M) % 4).float()
    want = (R.fp8_decode(codes) * ds[1]).to(DEV)
    assert bool(torch.isfinite(want).all()) and want.unique().numel() > 200
    r = G.route(ops, G.all_to_one_logits(B, n_e), k)
    assert r["count"].cpu().tolist() == [0, B, 0, 0]
    Wd, ds = Wd.to(DEV), ds.to(DEV)
    for shift in range(0, K, min(B, K)):
        ACT = one_hot_tokens(B, K, shift)
        D = torch.full((B, M), SENTINEL, device=DEV)
        ops.moe_group_down_fp8(D, Wd, ds, ACT, r["count"], r["offset"], B)
        assert torch.equal(D, want[None, :].expand(B, M)), (B, shift)


@pytest.mark.parametrize("B", [64, 16, 128])
def test_group_fp8_one_hot_matches_bf16_kernels(ops, B):
    """Codes that differ along k, power-of-two row scales: decode * scale
    is exact in bf16, and a one-hot token makes every sum a single term,
    so the fp8 kernels must equal the bf16 kernels on the dequantized
    slabs bit for bit — gate, silu input and up included.  A slab with
    the lo/hi 16-bit halves of every word swapped must not."""
    n_e, M, K, k = 4, 256, 64, 1
    finite = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F],
                          dtype=torch.uint8)
    m_ = torch.arange(M)[:, None]
    k_ = torch.arange(K)[None, :]

    def slab(step):
        w = torch.stack([finite[(m_ * 3 + step * k_ + 11 * e) % 254]
                         for e in range(n_e)]).contiguous()
        s = (2.0 ** -(4 + (torch.arange(n_e * M) % 3))).float().view(n_e, M)
        deq = (R.fp8_decode(w) * s[..., None]).to(BF)
        assert torch.equal(deq.float(), R.fp8_decode(w) * s[..., None])
        return w.to(DEV), s.to(DEV), deq.to(DEV)

    g8, gs, gd = slab(17)
    u8, us, ud = slab(29)
    d8, dsc, dd = slab(41)
    r = G.route(ops, G.all_to_one_logits(B, n_e), k)
    for shift in range(0, K, min(B, K)):
        X = one_hot_tokens(B, K, shift)
        act8 = torch.full((B, M), SENTINEL, device=DEV, dtype=BF)
        act = act8.clone()
        ops.moe_group_swiglu_fp8(act8, g8, gs, u8, us, X, r["count"],
                                 r["offset"], r["perm"], r["escale"], k)
        ops.moe_group_swiglu(act, gd, ud, X, r["count"], r["offset"],
                             r["perm"], r["escale"], k)
        assert torch.equal(act8, act), (B, shift)
        assert act.float().unique().numel() > 100

        swapped = u8.view(n_e, M, K // 4, 2, 2).flip(3).reshape(n_e, M, K)
        bad = torch.full((B, M), SENTINEL, device=DEV, dtype=BF)
        ops.moe_group_swiglu_fp8(bad, g8, gs, swapped.contiguous(), us, X,
                                 r["count"], r["offset"], r["perm"],
                                 r["escale"], k)
        assert not torch.equal(bad, act)

        D8 = torch.full((B, M), SENTINEL, device=DEV)
        D = D8.clone()
        ops.moe_group_down_fp8(D8, d8, dsc, X, r["count"], r["offset"], B)
        ops.moe_group_down(D, dd, X, r["count"], r["offset"], B)
        assert torch.equal(D8, D), (B, shift)


# ---------------------------------------------------------------------------
# 3. expert GEMMs against the fp32 reference on the dequantized weights
# ---------------------------------------------------------------------------
GEMM_CASES = G.GEMM_CASES + [(256, 224, 4, 2, 128, "random")]  # RB=128


@pytest.fixture(scope="module")
def weights8():
    cache = {}

    def get(E, I, n_e):
        if (E, I, n_e) not in cache:
            g = torch.Generator().manual_seed(1000 + E + I + n_e)
            cache[(E, I, n_e)] = tuple(
                quant_slab(G.mk(*shape, scale=1 / math.sqrt(shape[2]),
                                gen=g))
                for shape in ((n_e, I, E), (n_e, I, E), (n_e, E, I)))
        return cache[(E, I, n_e)]

    return get


def run_moe8(ops, r, X, res, Wg, Wu, Wd, k, count=None):
    """G.run_moe on fp8 slabs: W* are quant_slab tuples."""
    B, E = X.shape
    I = Wg[0].size(1)
    cnt = r["count"] if count is None else count
    ACT = torch.full((B * k, I), SENTINEL, device=DEV, dtype=BF)
    D = torch.full((B * k, E), SENTINEL, device=DEV)
    out = torch.empty_like(res)
    ops.moe_group_swiglu_fp8(ACT, Wg[0], Wg[1], Wu[0], Wu[1], X, cnt,
                             r["offset"], r["perm"], r["escale"], k)
    ops.moe_group_down_fp8(D, Wd[0], Wd[1], ACT, cnt, r["offset"], B)
    ops.moe_group_combine(out, res, D, r["inv"], k)
    return ACT, D, out


@pytest.mark.parametrize("E,I,n_e,k,B,routing", GEMM_CASES)
def test_expert_gemms_fp8(ops, weights8, E, I, n_e, k, B, routing):
    Wg, Wu, Wd = weights8(E, I, n_e)
    g = torch.Generator().manual_seed(300 + B)
    X = G.mk(B, E, gen=g)
    res = G.mk(B, E, gen=g)
    logits = G.case_logits(B, n_e, routing)
    G.assert_distinct(logits)
    r = G.route(ops, logits, k)

    ACT, D, out = run_moe8(ops, r, X, res, Wg, Wu, Wd, k)
    refs = G.reference(r, logits, X, res, Wg[2], Wu[2], Wd[2], k, ACT)
    for name, got, ref in zip(("ACT", "D", "out"), (ACT, D, out), refs):
        err = (got.float() - ref).abs().max()
        print(f"fp8 {name} E={E} I={I} B={B} {routing}: max|err|="
              f"{float(err):.4g} (max|ref|={float(ref.abs().max()):.3g})")
        assert torch.allclose(got.float(), ref, **G.TOL), (name, float(err))

    # teeth: the neighbouring expert's slabs, and the row scales dropped
    act_rot, d_rot, _ = G.reference(r, logits, X, res, Wg[2], Wu[2], Wd[2],
                                    k, ACT, rot=1)
    assert not torch.allclose(ACT.float(), act_rot, **G.TOL)
    assert not torch.allclose(D.float(), d_rot, **G.TOL)
    act_raw, d_raw, _ = G.reference(r, logits, X, res, Wg[3], Wu[3], Wd[3],
                                    k, ACT)
    assert not torch.allclose(ACT.float(), act_raw, **G.TOL)
    assert not torch.allclose(D.float(), d_raw, **G.TOL)

    # determinism: a second launch is bit-identical
    ACT2, D2, out2 = run_moe8(ops, r, X, res, Wg, Wu, Wd, k)
    assert torch.equal(ACT, ACT2) and torch.equal(D, D2)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("B,routing", [(17, "random"), (33, "same_two")])
def test_untouched_rows_keep_sentinel_fp8(ops, weights8, B, routing):
    """As test_group_moe_gpu.test_untouched_rows_keep_sentinel."""
    E, I, n_e, k = 256, 224, 4, 2
    Wg, Wu, Wd = weights8(E, I, n_e)
    g = torch.Generator().manual_seed(400 + B)
    X = G.mk(B, E, gen=g)
    res = G.mk(B, E, gen=g)
    r = G.route(ops, G.case_logits(B, n_e, routing), k)
    cnt = r["count"].cpu()
    off = r["offset"].cpu()
    full_ACT, full_D, _ = run_moe8(ops, r, X, res, Wg, Wu, Wd, k)
    assert not bool((full_ACT.float() == SENTINEL).any())
    assert not bool((full_D == SENTINEL).any())

    live = [e for e in range(n_e) if int(cnt[e]) > 0]
    dead, short = live[0], live[-1]
    assert dead != short and int(cnt[short]) > 2
    doctored = cnt.clone()
    doctored[dead] = 0       # its rows must stay untouched
    doctored[short] -= 2     # its last two rows become padding rows
    ACT, D, _ = run_moe8(ops, r, X, res, Wg, Wu, Wd, k,
                         count=doctored.to(DEV))
    untouched = list(range(int(off[dead]), int(off[dead + 1])))
    untouched += [int(off[short + 1]) - 2, int(off[short + 1]) - 1]
    mask = torch.zeros(B * k, dtype=torch.bool)
    mask[untouched] = True
    mask = mask.to(DEV)
    assert bool((ACT[mask].float() == SENTINEL).all())
    assert bool((D[mask] == SENTINEL).all())
    assert torch.equal(ACT[~mask], full_ACT[~mask])
    assert torch.equal(D[~mask], full_D[~mask])


@pytest.mark.parametrize("B", [5, 33])
def test_group_independence_fp8(ops, weights8, B):
    """As test_group_moe_gpu.test_group_independence."""
    E, I, n_e, k = 256, 224, 4, 2
    Wg, Wu, Wd = weights8(E, I, n_e)
    g = torch.Generator().manual_seed(500 + B)
    X = G.mk(B, E, gen=g)
    res = G.mk(B, E, gen=g)
    logits = G.tie_free_logits(B, n_e, seed=600 + B)
    p = torch.randperm(B, generator=g)
    assert not torch.equal(p, torch.arange(B))

    r1 = G.route(ops, logits, k)
    ACT1, D1, out1 = run_moe8(ops, r1, X, res, Wg, Wu, Wd, k)
    r2 = G.route(ops, logits[p], k)
    pd = p.to(DEV)
    ACT2, D2, out2 = run_moe8(ops, r2, X[pd].contiguous(),
                              res[pd].contiguous(), Wg, Wu, Wd, k)
    assert torch.equal(out2, out1[pd])
    inv1 = r1["inv"].long().view(B, k)
    inv2 = r2["inv"].long().view(B, k)
    for j in range(k):
        assert torch.equal(ACT2[inv2[:, j]], ACT1[inv1[pd, j]])
        assert torch.equal(D2[inv2[:, j]], D1[inv1[pd, j]])


def test_shape_guards_fp8(ops):
    """K % 32 != 0 is refused instead of mis-launched."""
    n_e, k, B, E, I = 4, 2, 3, 256, 208
    r = G.route(ops, G.tie_free_logits(B, n_e, seed=1), k)
    W = torch.zeros(n_e, E, I, device=DEV, dtype=torch.uint8)
    s = torch.ones(n_e, E, device=DEV)
    ACT = torch.zeros(B * k, I, device=DEV, dtype=BF)
    D = torch.zeros(B * k, E, device=DEV)
    with pytest.raises(RuntimeError, match="K % 32"):
        ops.moe_group_down_fp8(D, W, s, ACT, r["count"], r["offset"], B)
    Wi = torch.zeros(n_e, I, E, device=DEV, dtype=torch.uint8)
    X = torch.zeros(B, E, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="scales"):
        ops.moe_group_swiglu_fp8(ACT, Wi, s, Wi, s, X, r["count"],
                                 r["offset"], r["perm"], r["escale"], k)


# ---------------------------------------------------------------------------
# engine helpers
# ---------------------------------------------------------------------------
def _deq(w):
    from mdi_llm_amd.ops.engine import quantize_fp8_rowwise

    q, s = quantize_fp8_rowwise(w)
    return (q.float() * s[:, None]).to(BF)


def dequantized_state(m, experts_only=False):
    """state_dict of `m` with every matrix the single-sample fp8 engine
    quantizes (block linears, expert linears, lm_head) replaced by
    decode(byte) * scale cast to bf16; the router weights stay as they
    are.  experts_only: what the grouped engine quantizes."""
    sd = copy.deepcopy(m.state_dict())
    for name, mod in m.named_modules():
        if not isinstance(mod, torch.nn.Linear) or name.endswith("mlp.gate"):
            continue
        if experts_only and ".mlp.experts." not in name:
            continue
        sd[name + ".weight"] = _deq(sd[name + ".weight"])
    return sd


def _cpu_prompts(seed):
    g = torch.Generator().manual_seed(seed)  # G._prompts, on the CPU
    return [torch.randint(0, 511, (n,), generator=g) for n in PROMPT_LENS]


class _Schedule:
    """Three prompts prefilled with the bf16 weights everywhere (the
    engines' prefill is bf16), then the torch model `m8` takes the
    dequantized weights and teacher-forces 8 greedy steps.
    experts_only: the grouped engine's reference (see dequantized_state)."""

    def __init__(self, seed=ENGINE_SEED, experts_only=False, dev=DEV):
        from mdi_llm_amd import GPT, ModelConfig

        torch.manual_seed(seed)  # G._build, on `dev`
        self.cfg = ModelConfig.from_name("nano-moe-gpu")
        self.m8 = GPT(self.cfg)
        self.m8.apply_init()
        self.m8 = self.m8.to(device=dev, dtype=BF).eval()
        self.B = len(PROMPT_LENS)
        self.m8.set_kv_cache(self.B)
        self.prompts = [p.to(dev) for p in _cpu_prompts(seed + 1)]
        self.toks, self.pos = [], []
        for s, p in enumerate(self.prompts):
            ref = self.m8(p.view(1, -1), input_pos=0, slot=s)
            self.toks.append(int(ref[0, -1].float().argmax()))
            self.pos.append(p.numel())
        self.bf16_state = copy.deepcopy(self.m8.state_dict())
        self.m8.load_state_dict(dequantized_state(self.m8, experts_only))
        self.gate = []
        self.hooks = [blk.mlp.gate.register_forward_hook(
            lambda _m, _i, out: self.gate.append(
                out.float().view(-1).clone()))
            for blk in self.m8.transformer.h]

    def starter(self):
        """A starter stage holding the bf16 weights, prompts prefilled."""
        from mdi_llm_amd.models.stages import StarterStage

        st = StarterStage(self.cfg, self.cfg.n_layer).to(device=DEV,
                                                         dtype=BF)
        st.load_state_dict(self.bf16_state)
        st.eval()
        st.set_kv_cache(self.B)
        for s, p in enumerate(self.prompts):
            st.forward_head(p.view(1, -1), slot=s, input_pos=0)
        return st

    def tok(self, s):
        return torch.tensor([self.toks[s]], device=self.prompts[0].device,
                            dtype=torch.int32)

    def min_gate_gap(self, k):
        """Smallest k-th/(k+1)-th gate-logit gap of the last ref()."""
        srt = torch.stack(self.gate).sort(dim=1, descending=True).values
        return float((srt[:, k - 1] - srt[:, k]).min())

    def ref(self, s):
        """m8's logits for slot s at its current position; fills .gate."""
        self.gate.clear()
        return self.m8(self.tok(s).view(1, 1).long(), input_pos=self.pos[s],
                       slot=s)[0, -1].float()

    def advance(self, s, ref):
        self.toks[s] = int(ref.argmax())
        self.pos[s] += 1


def _engine(monkeypatch, stage, weights, prompts=True, **kw):
    from mdi_llm_amd.ops.engine import DecodeEngine

    if weights == "bf16":
        monkeypatch.delenv("MDI_WEIGHT_DTYPE", raising=False)
    else:
        monkeypatch.setenv("MDI_WEIGHT_DTYPE", weights)
    eng = DecodeEngine(stage, stage.kv_pool, n_chunks=8, **kw)
    if prompts:
        for s, n in enumerate(PROMPT_LENS):
            eng.set_slot_pos(s, n)
    return eng


def _gate_margin(sch, spy, k):
    """(smallest k-th/(k+1)-th gate gap in the torch model, largest gate
    deviation of the engine) over the layers of the step just taken."""
    assert len(sch.gate) == len(spy.logits) == sch.cfg.n_layer
    gap, dev = float("inf"), 0.0
    for tg, eg in zip(sch.gate, spy.logits):
        srt = tg.sort(descending=True).values
        gap = min(gap, float(srt[k - 1] - srt[k]))
        dev = max(dev, float((eg.view(-1) - tg).abs().max()))
    return gap, dev


# ---------------------------------------------------------------------------
# 4. single-sample engine
# ---------------------------------------------------------------------------
@torch.inference_mode()
def test_engine_fp8_moe_logits_vs_torch(monkeypatch):
    """DecodeEngine in fp8 mode on a MoE stage against the torch GPT that
    holds the dequantized weights, at each of 8 teacher-forced greedy
    steps of three slots.  Bound: twice the bf16 engine's distance from
    the bf16 torch model at the same (step, slot) — the fp8 GEMVs add only
    fp32 reassociation to the same bf16 pipeline (the project's margin,
    tests/test_int4_gpu.py).

    Near-tied routing may legitimately flip, so at every checked (step,
    slot, layer) the gap between the k-th and (k+1)-th gate logit of the
    torch model must exceed the engine's gate-logit deviation there (the
    router weight stays bf16, so that deviation is the bf16 pipeline's).
    Measured on MI355X over the 24 (step, slot) pairs: fp8 engine vs the
    dequantized torch model mean 0.00823 / max 0.01009, bf16 engine vs the
    bf16 torch model mean 0.00760 / max 0.00859, worst ratio at one pair
    1.43; minimum gate gap 0.0415, largest gate deviation 0.0039."""
    cfg, m = G._build(seed=ENGINE_SEED)        # the bf16 torch model
    sch = _Schedule()
    B, k = sch.B, cfg.n_expert_per_token
    m.set_kv_cache(B)
    for s, p in enumerate(sch.prompts):
        m(p.view(1, -1), input_pos=0, slot=s)
    eng_b = _engine(monkeypatch, sch.starter(), "bf16", use_graphs=False)
    assert not eng_b.fp8
    st8 = sch.starter()
    eng8 = _engine(monkeypatch, st8, "fp8", use_graphs=False)
    assert eng8.fp8 and not eng8.int4
    w0 = eng8.blocks[0]
    assert w0.fc1_w8.dtype == torch.float8_e4m3fn
    assert w0.gate_w.dtype == BF and not hasattr(w0, "gate_w8")
    assert w0.gate_w.data_ptr() == \
        st8.transformer.h[0].mlp.gate.weight.data_ptr()
    spy = G._GateSpy(eng8.ops)
    eng8.ops = spy

    worst, min_gap, max_dev = 0.0, float("inf"), 0.0
    rels, bases = [], []
    for step in range(N_STEPS):
        for s in range(B):
            tok = sch.tok(s)
            ref_b = m(tok.view(1, 1).long(), input_pos=sch.pos[s],
                      slot=s)[0, -1].float()
            ref8 = sch.ref(s)
            got_b = eng_b.tail(eng_b.decode_step_head(tok, s)).float()
            base = G._rel(got_b.view(-1), ref_b)
            spy.logits.clear()
            got8 = eng8.tail(eng8.decode_step_head(tok, s)).float()
            gap, dev = _gate_margin(sch, spy, k)
            min_gap, max_dev = min(min_gap, gap), max(max_dev, dev)
            assert gap > dev, ("precondition: routing near-tied in the "
                               "torch reference", step, s, gap, dev)
            rel = G._rel(got8.view(-1), ref8)
            rels.append(rel)
            bases.append(base)
            worst = max(worst, rel / base)
            print(f"step {step} slot {s}: fp8 rel={rel:.5f} "
                  f"bf16 base={base:.5f}")
            assert rel < 2 * base, (step, s, rel, base)
            sch.advance(s, ref8)
    print(f"fp8 rel mean={sum(rels) / len(rels):.5f} max={max(rels):.5f}; "
          f"bf16 base mean={sum(bases) / len(bases):.5f} "
          f"max={max(bases):.5f}; worst rel/base={worst:.3f}; min gate "
          f"gap={min_gap:.4g}, max fp8-engine gate deviation={max_dev:.4g}")


def _moe_stage(seed):
    cfg, m = G._build(seed=seed)
    return cfg, m, G._starter(cfg, m, 1)


@torch.inference_mode()
def test_engine_fp8_moe_graph_matches_eager(monkeypatch):
    """The fused step graph in fp8 mode against eager stepping over 8
    greedy tokens: each graph pick is a maximum of the eager logits."""
    cfg, m = G._build(seed=ENGINE_SEED + 4)
    torch.manual_seed(ENGINE_SEED + 5)
    prompt = torch.randint(0, 511, (8,), device=DEV)
    t0 = 5

    sg = G._starter(cfg, m, 1)
    eng_g = _engine(monkeypatch, sg, "fp8", prompts=False, use_graphs=True)
    assert eng_g.fp8
    eng_g.ensure_fused_graphs(0.0, 0, 0)  # greedy; before prefill
    sg.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng_g.set_slot_pos(0, 8)
    eng_g.token_table[0] = t0

    se = G._starter(cfg, m, 1)
    eng_e = _engine(monkeypatch, se, "fp8", prompts=False, use_graphs=False)
    se.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng_e.set_slot_pos(0, 8)

    tok = t0
    for i in range(N_STEPS):
        eng_g.standalone_step(0)
        nxt = int(eng_g.token_table[0])
        x = eng_e.decode_step_head(
            torch.tensor([tok], device=DEV, dtype=torch.int32), 0)
        logits = eng_e.tail(x).float()
        assert float(logits[nxt]) == float(logits.max()), (
            i, nxt, int(logits.argmax()))
        tok = nxt
    assert bool(torch.isfinite(logits).all())


@torch.inference_mode()
def test_secondary_fp8_moe_graph_matches_eager(monkeypatch):
    from mdi_llm_amd.models.stages import SecondaryStage

    cfg, m = G._build(seed=ENGINE_SEED + 6)
    sd = {k_: v for k_, v in m.state_dict().items()
          if k_.startswith(("transformer.h.0.", "transformer.h.1."))}

    def secondary():
        st = SecondaryStage(cfg, 2).to(device=DEV, dtype=BF)
        st.load_state_dict(sd)
        st.eval()
        st.set_kv_cache(1)
        return st

    g = torch.Generator().manual_seed(ENGINE_SEED + 7)
    xp = G.mk(1, 8, cfg.n_embd, gen=g)
    xs = [G.mk(cfg.n_embd, gen=g) for _ in range(N_STEPS)]

    sg = secondary()
    eng_g = _engine(monkeypatch, sg, "fp8", prompts=False, use_graphs=True)
    assert eng_g.fp8 and not eng_g.is_starter
    eng_g.capture_graphs()  # before prefill: the warm-up scribbles caches
    assert eng_g._graph_blocks is not None
    sg(xp, slot=0, input_pos=0)
    eng_g.set_slot_pos(0, 8)

    se = secondary()
    eng_e = _engine(monkeypatch, se, "fp8", prompts=False, use_graphs=False)
    se(xp, slot=0, input_pos=0)
    eng_e.set_slot_pos(0, 8)

    for i, x in enumerate(xs):
        yg = eng_g.decode_step_mid(x.clone(), 0).clone()
        ye = eng_e.decode_step_mid(x.clone(), 0).clone()
        assert torch.equal(yg, ye), (
            i, float((yg.float() - ye.float()).abs().max()))
    assert bool(torch.isfinite(ye.float()).all())


# ---------------------------------------------------------------------------
# 5. grouped engine
# ---------------------------------------------------------------------------
def _group_engine(monkeypatch, stage, B, **kw):
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "fp8")
    with pytest.warns(UserWarning, match="only the dense GEMMs"):
        eng = GroupDecodeEngine(stage, stage.kv_pool, B, n_chunks=8, **kw)
    assert eng.moe and eng.moe_fp8 and not eng.fp8
    assert eng.blocks[0].fc1_w8.dtype == torch.float8_e4m3fn
    assert not hasattr(eng.blocks[0], "attn_w8")
    return eng


@torch.inference_mode()
def test_group_fp8_moe_graph_matches_eager(monkeypatch):
    """As test_group_moe_gpu.test_group_moe_graph_matches_eager with fp8
    expert slabs (B=3, prompt lengths 5, 9, 3)."""
    cfg, m = G._build(seed=ENGINE_SEED)
    B = len(PROMPT_LENS)
    m.set_kv_cache(B)
    sg, se = G._starter(cfg, m, B), G._starter(cfg, m, B)
    eng_g = _group_engine(monkeypatch, sg, B)
    eng_g.ensure_graphs(0.0, 0, 0)  # greedy; before prefill
    eng_e = _group_engine(monkeypatch, se, B, use_graphs=False)
    for s, p in enumerate(G._prompts(ENGINE_SEED + 1)):
        t0 = int(m(p.view(1, -1), input_pos=0, slot=s)[0, -1].float()
                 .argmax())
        for st, eng in ((sg, eng_g), (se, eng_e)):
            st.forward_head(p.view(1, -1), slot=s, input_pos=0)
            eng.set_slot_pos(s, p.numel())
            eng.token_table[s] = t0

    slots = torch.arange(B, device=DEV, dtype=torch.int32)
    for step in range(N_STEPS):
        eng_g.set_group(slots)
        eng_g.standalone_step()
        got = eng_g.token_table.clone()
        eng_e.set_group(slots)
        eng_e.head_step()
        eng_e._tail_seq()
        logits = eng_e.LOGITS.float()
        picked = logits.gather(1, got.long().view(B, 1)).view(B)
        assert torch.equal(picked, logits.max(dim=1).values), (
            step, got.tolist(), logits.argmax(dim=1).tolist())
        eng_e.token_table.copy_(got)
    assert bool(torch.isfinite(logits).all())


@torch.inference_mode()
def test_group_fp8_moe_logits_vs_torch(monkeypatch):
    """Per-slot logits of the grouped engine with fp8 expert slabs against
    the torch GPT holding the dequantized weights; yardstick: the single-
    sample fp8 engine at the same (step, slot), bound twice its distance.
    Each engine is measured against the torch model holding exactly the
    weights it computes with: the grouped engine quantizes the expert
    slabs only (its qkv, proj and lm_head GEMMs stay bf16), so its
    reference dequantizes the experts only; the single-sample engine's
    dequantizes every matrix.  Both references are teacher-forced with
    the same tokens, and a step counts only if neither routes near a tie
    (the precondition of the single-sample test, on both models)."""
    sch = _Schedule()
    schg = _Schedule(experts_only=True)
    assert schg.toks == sch.toks
    cfg, B, k = sch.cfg, sch.B, sch.cfg.n_expert_per_token
    sg = schg.starter()
    geng = _group_engine(monkeypatch, sg, B, use_graphs=False)
    for s, n in enumerate(PROMPT_LENS):
        geng.set_slot_pos(s, n)
    s1 = sch.starter()
    eng1 = _engine(monkeypatch, s1, "fp8", use_graphs=False)
    assert eng1.fp8
    spy = G._GateSpy(eng1.ops)
    eng1.ops = spy

    slots = torch.arange(B, device=DEV, dtype=torch.int32)
    worst = 0.0
    for step in range(N_STEPS):
        geng.token_table.copy_(torch.tensor(sch.toks, dtype=torch.int32))
        geng.set_group(slots)
        geng.head_step()
        geng._tail_seq()
        glogits = geng.LOGITS.float().clone()
        for s in range(B):
            tok = sch.tok(s)
            ref8 = sch.ref(s)
            schg.toks[s] = sch.toks[s]
            refg = schg.ref(s)
            spy.logits.clear()
            got1 = eng1.tail(eng1.decode_step_head(tok, s)).float()
            gap, dev = _gate_margin(sch, spy, k)
            gap = min(gap, schg.min_gate_gap(k))
            assert gap > dev, ("precondition: routing near-tied in the "
                               "torch reference", step, s, gap, dev)
            base = G._rel(got1.view(-1), ref8)
            rel = G._rel(glogits[s], refg)
            worst = max(worst, rel / base)
            print(f"step {step} slot {s}: grouped fp8 rel={rel:.5f} "
                  f"single-sample fp8 base={base:.5f}")
            assert rel < 2 * base, (step, s, rel, base)
            sch.advance(s, ref8)
            schg.pos[s] += 1
    print(f"worst grouped/single-sample ratio={worst:.3f}")


def test_engines_share_fp8_slabs(monkeypatch):
    """One stage, a grouped and a single-sample engine: one copy of the
    fp8 slabs (and of the bf16 ones).  Not under inference_mode: inference
    tensors track no version, so their slabs are never cached."""
    cfg, m = G._build(seed=ENGINE_SEED + 11)
    B = 2
    stage = G._starter(cfg, m, B)
    geng = _group_engine(monkeypatch, stage, B, use_graphs=False)
    eng = _engine(monkeypatch, stage, "fp8", prompts=False,
                  use_graphs=False)
    for w1, wg in zip(eng.blocks, geng.blocks):
        for name in ("fc1_w8", "fc1_s", "fc2_w8", "fc2_s", "mlp_proj_w8",
                     "mlp_proj_s", "fc1_w"):
            assert getattr(w1, name).data_ptr() == \
                getattr(wg, name).data_ptr(), name


@torch.inference_mode()
def test_group_dense_stage_still_ignores_fp8(monkeypatch):
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "fp8")
    cfg, m = G._build("nano-gpu", seed=ENGINE_SEED + 8)
    stage = G._starter(cfg, m, 2)
    with pytest.warns(UserWarning, match="ignores MDI_WEIGHT_DTYPE=fp8"):
        geng = GroupDecodeEngine(stage, stage.kv_pool, 2, n_chunks=8)
    assert not geng.fp8 and not geng.moe_fp8 and not geng.moe
    w0 = geng.blocks[0]
    assert not any(hasattr(w0, n) for n in ("fc1_w8", "attn_w8",
                                            "mlp_proj_w8"))


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def _build_cfg(seed, **over):
    from mdi_llm_amd import GPT, ModelConfig

    torch.manual_seed(seed)
    cfg = ModelConfig.from_name("nano-moe-gpu", **over)
    m = GPT(cfg)
    m.apply_init()
    m = m.to(device=DEV, dtype=BF)
    m.eval()
    return cfg, m


def test_fp8_moe_shape_refused(monkeypatch):
    """intermediate_size 232 is a multiple of 8 (the bf16 engine takes it)
    but not of the 16 fp8 bytes a lane loads."""
    from mdi_llm_amd.ops.engine import DecodeEngine, engine_supported

    cfg, m = _build_cfg(ENGINE_SEED + 9, intermediate_size=232)
    assert cfg.intermediate_size == 232 and engine_supported(cfg)
    stage = G._starter(cfg, m, 1)
    monkeypatch.delenv("MDI_WEIGHT_DTYPE", raising=False)
    DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)
    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "fp8")
    with pytest.raises(ValueError, match="232"):
        DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)


def test_int4_moe_still_refused(monkeypatch):
    from mdi_llm_amd.ops.engine import DecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    cfg, m = _build_cfg(ENGINE_SEED + 10)
    stage = G._starter(cfg, m, 1)
    with pytest.raises(ValueError, match="int4"):
        DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)
