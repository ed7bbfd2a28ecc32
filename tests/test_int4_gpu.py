"""GPU: int4 group-quantized decode weights — the gemv_int4 /
gemv_swiglu_int4 kernels against the exact dequantized reference, and the
DecodeEngine in MDI_WEIGHT_DTYPE=int4 mode (eager, hipGraph, secondary
stage, LayerNorm/GELU/parallel-residual config, refusals)."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=5e-2, rtol=5e-2)  # the fp8 GEMV tests' figure


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def mk(*shape, scale=1.0, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return (torch.randn(*shape, device=DEV) * scale).to(
        torch.bfloat16).contiguous()


def quant(W):
    from mdi_llm_amd.ops.engine import (dequantize_int4,
                                        quantize_int4_groupwise)

    packed, qp = quantize_int4_groupwise(W)
    return packed, qp, dequantize_int4(packed, qp, W.size(1))


def staged_x(x, g, b, norm_kind, eps=1e-5):
    """(bf16-rounded x as the kernel stages it, uniform post-dot scale)."""
    xf = x.float()
    if norm_kind == 0:
        return xf, 1.0
    if norm_kind == 1:
        xs = (xf * g.float()).to(torch.bfloat16).float()
        return xs, torch.rsqrt(xf.pow(2).mean() + eps)
    xn = torch.nn.functional.layer_norm(xf, (x.numel(),), g.float(),
                                        None if b is None else b.float(),
                                        eps)
    return xn.to(torch.bfloat16).float(), 1.0


# ---------------------------------------------------------------------------
# 1. gemv_int4 vs dequantize_int4(...) @ x in fp32
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gemv_case():
    cache = {}

    def get(M, K):
        if (M, K) not in cache:
            W = mk(M, K, scale=1.0 / math.sqrt(K), seed=60)
            x = mk(K, seed=61)
            packed, qp, deq = quant(W)
            cache[(M, K)] = (packed, qp, x, deq @ x.float())
        return cache[(M, K)]

    return get


@pytest.mark.parametrize("M,K,rows", [
    (176, 128, 0), (176, 128, 1), (176, 128, 2), (176, 128, 4),
    (64, 688, 0), (64, 688, 1), (64, 688, 2), (64, 688, 4),
    (4096, 4096, 0), (128256, 512, 0),
])
def test_gemv_int4(ops, gemv_case, M, K, rows):
    packed, qp, x, ref = gemv_case(M, K)
    out = torch.empty(M, device=DEV, dtype=torch.bfloat16)
    ops.gemv_int4(out, packed, qp, x, None, None, 0, rows=rows)
    err = (out.float() - ref).abs().max()
    print(f"gemv_int4 {M}x{K} rows={rows}: max|err|={float(err):.4g}")
    assert torch.allclose(out.float(), ref, **TOL), float(err)


@pytest.mark.parametrize("norm_kind", [0, 1, 2])
@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
def test_gemv_int4_epilogue_norm(ops, epilogue, norm_kind):
    M = K = 256
    W = mk(M, K, scale=1.0 / math.sqrt(K), seed=62)
    x = mk(K, seed=63)
    bias = mk(M, seed=64)
    res = mk(M, seed=65)
    g = mk(K, seed=66)
    b = mk(K, seed=67)
    packed, qp, deq = quant(W)
    out = torch.empty(M, device=DEV, dtype=torch.bfloat16)
    ops.gemv_int4(out, packed, qp, x, bias, res, epilogue,
                  g if norm_kind else None, b if norm_kind == 2 else None,
                  norm_kind, 1e-5, 1)
    xs, post = staged_x(x, g, b, norm_kind)
    ref = (deq @ xs) * post + bias.float()
    if epilogue == 1:
        ref = ref + res.float()
    elif epilogue == 2:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    elif epilogue == 3:
        ref = torch.nn.functional.silu(ref)
    err = (out.float() - ref).abs().max()
    print(f"epi={epilogue} norm={norm_kind}: max|err|={float(err):.4g}")
    assert torch.allclose(out.float(), ref, **TOL), float(err)


# ---------------------------------------------------------------------------
# 2. gemv_swiglu_int4
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(2048, 1024), (688, 256)])
@pytest.mark.parametrize("gelu_gate", [False, True])
def test_gemv_swiglu_int4(ops, M, K, gelu_gate):
    Wg = mk(M, K, scale=1.0 / math.sqrt(K), seed=70)
    Wu = mk(M, K, scale=1.0 / math.sqrt(K), seed=71)
    x = mk(K, seed=72)
    gp, gq, gdeq = quant(Wg)
    up, uq, udeq = quant(Wu)
    out = torch.empty(M, device=DEV, dtype=torch.bfloat16)
    ops.gemv_swiglu_int4(out, gp, gq, up, uq, x, gelu_gate)
    gg = gdeq @ x.float()
    uu = udeq @ x.float()
    act = (torch.nn.functional.gelu(gg, approximate="tanh") if gelu_gate
           else torch.nn.functional.silu(gg))
    ref = act * uu
    err = (out.float() - ref).abs().max()
    print(f"swiglu_int4 {M}x{K} gelu={gelu_gate}: max|err|={float(err):.4g}")
    assert torch.allclose(out.float(), ref, **TOL), float(err)


def test_gemv_swiglu_int4_fused_norm(ops):
    """padded K (688) through the fused RMSNorm staging."""
    M, K = 256, 688
    Wg = mk(M, K, scale=1.0 / math.sqrt(K), seed=73)
    Wu = mk(M, K, scale=1.0 / math.sqrt(K), seed=74)
    x = mk(K, seed=75)
    g = mk(K, seed=76)
    gp, gq, gdeq = quant(Wg)
    up, uq, udeq = quant(Wu)
    out = torch.empty(M, device=DEV, dtype=torch.bfloat16)
    ops.gemv_swiglu_int4(out, gp, gq, up, uq, x, False, g, None, 1, 1e-5)
    xs, post = staged_x(x, g, None, 1)
    ref = torch.nn.functional.silu((gdeq @ xs) * post) * ((udeq @ xs) * post)
    assert torch.allclose(out.float(), ref, **TOL), \
        float((out.float() - ref).abs().max())


# ---------------------------------------------------------------------------
# engine helpers
# ---------------------------------------------------------------------------
def _build(name="nano-gpu", seed=0):
    from mdi_llm_amd import GPT, ModelConfig

    torch.manual_seed(seed)
    cfg = ModelConfig.from_name(name)
    m = GPT(cfg)
    m.apply_init()
    m = m.to(device=DEV, dtype=torch.bfloat16)
    m.eval()
    return cfg, m


def _starter(cfg, m, n_slots=1):
    from mdi_llm_amd.models.stages import StarterStage

    stage = StarterStage(cfg, cfg.n_layer).to(device=DEV,
                                              dtype=torch.bfloat16)
    stage.load_state_dict(m.state_dict())
    stage.eval()
    stage.set_kv_cache(n_slots)
    return stage


def _dequantized_state(m):
    """state_dict of `m` with every matrix the int4 engine quantizes (all
    block linears + lm_head) replaced by dequant(quant(w)) cast to bf16."""
    sd = copy.deepcopy(m.state_dict())
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Linear):
            w = sd[name + ".weight"]
            sd[name + ".weight"] = quant(w)[2].to(torch.bfloat16)
    return sd


def _rel(logits, ref):
    # test_engine_fp8_mode's metric
    return float((logits - ref).abs().mean() / ref.abs().std())


@torch.inference_mode()
def _int4_logit_check(monkeypatch, name, seed):
    """Prefill 8 tokens with the torch stage, decode one token through the
    int4 engine; compare with the torch GPT holding the dequantized
    weights on the same (bf16-prefilled) KV cache."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, m = _build(name, seed=seed)
    stage = _starter(cfg, m)
    m.set_kv_cache(1)
    torch.manual_seed(seed + 1)
    prompt = torch.randint(0, 511, (8,), device=DEV)
    tok = torch.tensor([5], device=DEV, dtype=torch.int32)
    stage.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    m(prompt.view(1, -1), input_pos=0, slot=0)

    # base: the bf16 engine against the unmodified torch model (both
    # existing code) — the noise floor of the shared bf16 pipeline
    monkeypatch.delenv("MDI_WEIGHT_DTYPE", raising=False)
    eng = DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)
    assert not eng.int4 and not eng.fp8
    eng.set_slot_pos(0, 8)
    got = eng.tail(eng.decode_step_head(tok, 0)).float().clone()
    ref = m(tok.view(1, 1).long(), input_pos=8, slot=0)[0, -1].float()
    base = _rel(got, ref)

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    eng4 = DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)
    assert eng4.int4 and not eng4.fp8 and not eng4._fuse_attn_proj
    eng4.set_slot_pos(0, 8)  # redo position 8 on the same prefilled cache
    got4 = eng4.tail(eng4.decode_step_head(tok, 0)).float().clone()
    m.load_state_dict(_dequantized_state(m))
    ref4 = m(tok.view(1, 1).long(), input_pos=8, slot=0)[0, -1].float()
    rel = _rel(got4, ref4)
    print(f"{name}: int4 engine vs dequantized torch rel={rel:.5f}, "
          f"bf16 engine vs torch base={base:.5f}")
    return rel, base


# ---------------------------------------------------------------------------
# 3. engine, nano-gpu (intermediate_size 688 = 5*128 + 48: padded groups)
# ---------------------------------------------------------------------------
def test_engine_int4_eager(monkeypatch):
    rel, base = _int4_logit_check(monkeypatch, "nano-gpu", 80)
    assert rel < 0.2, rel
    # the int4 kernels add only fp32 reassociation on top of the same bf16
    # pipeline: allow twice the bf16 engine's own distance from torch
    # (measured on MI355X: base 0.00836, int4 0.00850; nano-neox-gpu
    # below: base 0.01022, int4 0.01127)
    assert rel < 2 * base, (rel, base)


# ---------------------------------------------------------------------------
# 5. LayerNorm + GptNeoxMLP (GELU epilogue) + parallel residual
# ---------------------------------------------------------------------------
def test_engine_int4_neox(monkeypatch):
    rel, base = _int4_logit_check(monkeypatch, "nano-neox-gpu", 82)
    assert rel < 0.2, rel
    assert rel < 2 * base, (rel, base)


# ---------------------------------------------------------------------------
# 4. hipGraph capture in int4 mode
# ---------------------------------------------------------------------------
@torch.inference_mode()
def test_engine_int4_fused_graph_matches_eager(monkeypatch):
    from mdi_llm_amd.ops.engine import DecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    cfg, m = _build(seed=84)
    torch.manual_seed(85)
    prompt = torch.randint(0, 511, (8,), device=DEV)
    t0 = 5

    sg = _starter(cfg, m)
    eng_g = DecodeEngine(sg, sg.kv_pool, n_chunks=8, use_graphs=True)
    assert eng_g.int4
    eng_g.ensure_fused_graphs(0.0, 0, 0)  # greedy; before prefill
    sg.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng_g.set_slot_pos(0, 8)
    eng_g.token_table[0] = t0

    se = _starter(cfg, m)
    eng_e = DecodeEngine(se, se.kv_pool, n_chunks=8, use_graphs=False)
    assert eng_e.int4
    se.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng_e.set_slot_pos(0, 8)

    tok = t0
    for i in range(16):
        eng_g.standalone_step(0)
        nxt = int(eng_g.token_table[0])
        # the eager engine steps the same token; the kernels are
        # deterministic, so the graph's greedy pick must be a maximum of
        # the eager logits
        x = eng_e.decode_step_head(
            torch.tensor([tok], device=DEV, dtype=torch.int32), 0)
        logits = eng_e.tail(x).float()
        assert float(logits[nxt]) == float(logits.max()), (
            i, nxt, int(logits.argmax()))
        tok = nxt


@torch.inference_mode()
def test_secondary_int4_graph_matches_eager(monkeypatch):
    from mdi_llm_amd.models.stages import SecondaryStage
    from mdi_llm_amd.ops.engine import DecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    cfg, m = _build(seed=86)
    sd = {k: v for k, v in m.state_dict().items()
          if k.startswith(("transformer.h.0.", "transformer.h.1."))}

    def secondary():
        st = SecondaryStage(cfg, 2).to(device=DEV, dtype=torch.bfloat16)
        st.load_state_dict(sd)
        st.eval()
        st.set_kv_cache(1)
        return st

    torch.manual_seed(87)
    xp = mk(1, 8, cfg.n_embd)
    xs = [mk(cfg.n_embd) for _ in range(16)]

    sg = secondary()
    eng_g = DecodeEngine(sg, sg.kv_pool, n_chunks=8, use_graphs=True)
    assert eng_g.int4 and not eng_g.is_starter
    eng_g.capture_graphs()  # before prefill: the warm-up scribbles caches
    assert eng_g._graph_blocks is not None
    sg(xp, slot=0, input_pos=0)
    eng_g.set_slot_pos(0, 8)

    se = secondary()
    eng_e = DecodeEngine(se, se.kv_pool, n_chunks=8, use_graphs=False)
    se(xp, slot=0, input_pos=0)
    eng_e.set_slot_pos(0, 8)

    for i, x in enumerate(xs):
        yg = eng_g.decode_step_mid(x.clone(), 0).clone()
        ye = eng_e.decode_step_mid(x.clone(), 0).clone()
        assert torch.equal(yg, ye), (i, float((yg.float()
                                               - ye.float()).abs().max()))
    assert bool(torch.isfinite(ye.float()).all())


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_int4_moe_refused(monkeypatch):
    from mdi_llm_amd.ops.engine import DecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    cfg, m = _build("nano-moe-gpu", seed=88)
    stage = _starter(cfg, m)
    with pytest.raises(ValueError, match="int4"):
        DecodeEngine(stage, stage.kv_pool, n_chunks=8, use_graphs=False)


@torch.inference_mode()
def test_group_engine_ignores_int4(monkeypatch):
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "int4")
    cfg, m = _build(seed=89)
    B = 2
    stage = _starter(cfg, m, n_slots=B)
    m.set_kv_cache(B)
    with pytest.warns(UserWarning, match="int4"):
        geng = GroupDecodeEngine(stage, stage.kv_pool, B, n_chunks=8)
    assert not geng.fp8 and not getattr(geng, "int4", False)
    assert not hasattr(geng.blocks[0], "attn_w4")
    geng.ensure_graphs(0.0, 0, 0)

    # still the bf16 path: one greedy step matches the torch model
    torch.manual_seed(90)
    ref = []
    for s, n in enumerate((5, 7)):
        p = torch.randint(0, 511, (n,), device=DEV)
        stage.forward_head(p.view(1, -1), slot=s, input_pos=0)
        t0 = int(m(p.view(1, -1), input_pos=0, slot=s)[0, -1].float()
                 .argmax())
        geng.set_slot_pos(s, n)
        geng.token_table[s] = t0
        logits = m(torch.tensor([[t0]], device=DEV), input_pos=n, slot=s)
        ref.append(int(logits[0, -1].float().argmax()))
    geng.set_group(torch.arange(B, device=DEV, dtype=torch.int32))
    geng.standalone_step()
    assert geng.token_table.cpu().tolist() == ref
