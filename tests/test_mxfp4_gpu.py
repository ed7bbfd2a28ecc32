"""GPU: OCP MXFP4 decode weights.  gemv_mxfp4 / gemv_swiglu_mxfp4 against
dequantize_mxfp4(...) in fp64 under gemv_reference's bound, the element and
scale placement by one-hot equality, the host guards, and DecodeEngine with
MDI_WEIGHT_DTYPE=mxfp4 (dense and MoE, eager and graph)."""

import copy
import itertools

import pytest
import torch

import gemv_reference as R
import test_group_moe_gpu as G
from mdi_llm_amd.ops.engine import (dequantize_mxfp4, quantize_mxfp4,
                                    quantize_mxfp4_slab)

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
KS = (32, 40, 2048 + 32, 8192 + 64)  # chunk, pad, past a stride, past four


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _rand(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF)


def _slab(M, K, seed):
    """3 expert slabs: (packed, scales) on the GPU, fp32 dequantized."""
    q, s = quantize_mxfp4_slab(_rand(3, M, K, seed=seed, scale=0.05))
    deq = torch.stack([dequantize_mxfp4(q[e], s[e], K) for e in range(3)])
    return q.to(DEV), s.to(DEV), deq


def _pick(q, s, deq, K, eidx):
    """Op arguments and reference weights: a plain matrix (slab 1) without
    eidx, else the stack, where an index past the last slab clamps."""
    if eidx is None:
        return q[1], s[1], R.Weights("bf16", K, w=deq[1]), {}
    kw = dict(eidx=torch.tensor([eidx], device=DEV, dtype=torch.int32),
              estride=q[0].numel())
    return q, s, R.Weights("bf16", K, w=deq[min(eidx, 2)]), kw


def test_one_hot_placement(ops):
    """Row p holds one nonzero per block, at position p, with the block's
    own exponent; x = 1 at one k returns column k exactly.  Blocks 0, 63 and
    64 are the first scale dword's byte 0 (two lanes) and byte 1."""
    K = 65 * 32
    b = torch.arange(65)
    val = (1 + 0.5 * (b % 2)) * (1 - 2 * (b % 3 == 0)) * 2.0 ** (b % 15 - 7)
    w = torch.zeros(32, 65, 32)
    w[torch.arange(32), :, torch.arange(32)] = val
    w = w.view(32, K).to(BF)
    q, s = quantize_mxfp4(w)
    assert torch.equal(dequantize_mxfp4(q, s, K), w.float())
    q, s = q.to(DEV), s.to(DEV)
    for blk, p in itertools.product((0, 63, 64), range(32)):
        x = torch.zeros(K, dtype=BF, device=DEV)
        x[blk * 32 + p] = 1.0
        buf = R.new_out_buffer(32, DEV)
        ops.gemv_mxfp4(buf[:32], q, s, x, None, None, 0)
        assert torch.equal(buf[:32].cpu(), w[:, blk * 32 + p]), (blk, p)


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("M", [1, 5, 67])
@pytest.mark.parametrize("K", KS)
def test_gemv_mxfp4(ops, K, M, rows):
    q, s, deq = _slab(M, K, seed=K + M)
    x = _rand(K, seed=K + 1)
    nw, nb = _rand(K, seed=3, scale=0.1, shift=1.0), _rand(K, seed=4)
    bias, res = _rand(M, seed=5), _rand(M, seed=6)
    worst = 0.0
    for (epi, b_, r_), norm, eidx in itertools.product(
            ((0, None, None), (0, bias, None), (1, None, res)), (0, 1, 2),
            (None, 2, 7)):
        if norm == 2 and eidx is not None:
            continue  # refused, see test_guards
        W, S, wt, kw = _pick(q, s, deq, K, eidx)
        n = (None, None) if norm == 0 else (nw, nb if norm == 2 else None)
        ref = R.gemv_ref(wt, x, b_, r_, epi, *n, norm)
        buf = R.new_out_buffer(M, DEV)
        d = [None if t is None else t.to(DEV) for t in (b_, r_, *n)]
        ops.gemv_mxfp4(buf[:M], W, S, x.to(DEV), d[0], d[1], epi, d[2], d[3],
                       norm, R.EPS, rows, **kw)
        ok, ratio, msg = R.check_out_buffer(buf, M, ref, K)
        assert ok, (epi, norm, eidx, msg)
        worst = max(worst, ratio)
    print(f"gemv_mxfp4 {M}x{K} rows={rows}: worst err/bound {worst:.3g}")


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("M", [1, 5, 67])
@pytest.mark.parametrize("K", KS)
def test_gemv_swiglu_mxfp4(ops, K, M, gelu):
    gq, gs, gdeq = _slab(M, K, seed=K + M)
    uq, us, udeq = _slab(M, K, seed=K + M + 7)
    x = _rand(K, seed=K + 2)
    nw, nb = _rand(K, seed=3, scale=0.1, shift=1.0), _rand(K, seed=4)
    esc = torch.tensor([0.375])
    for norm, eidx in itertools.product((0, 1, 2), (None, 2, 7)):
        if norm == 2 and eidx is not None:
            continue
        Wg, Sg, wg, kw = _pick(gq, gs, gdeq, K, eidx)
        Wu, Su, wu, _ = _pick(uq, us, udeq, K, eidx)
        if eidx is not None:
            kw["escale"] = esc.to(DEV)
        n = (None, None) if norm == 0 else (nw, nb if norm == 2 else None)
        ref = R.gemv_swiglu_ref(wg, wu, x, gelu, *n, norm,
                                escale=esc[0] if eidx is not None else None)
        buf = R.new_out_buffer(M, DEV)
        d = [None if t is None else t.to(DEV) for t in n]
        ops.gemv_swiglu_mxfp4(buf[:M], Wg, Sg, Wu, Su, x.to(DEV), gelu, *d,
                              norm, R.EPS, **kw)
        ok, _, msg = R.check_out_buffer(buf, M, ref, K)
        assert ok, (norm, eidx, msg)


def test_guards(ops):
    """Every refusal comes before a launch: out keeps its sentinel."""
    M, K = 5, 40
    q, s, _ = _slab(M, K, seed=9)
    x, nw = _rand(K, seed=1).to(DEV), _rand(K, seed=2).to(DEV)
    e2 = torch.tensor([2], device=DEV, dtype=torch.int32)
    buf = R.new_out_buffer(M, DEV)
    o = buf[:M]
    bad = [
        lambda: ops.gemv_mxfp4(o, q[1][:, :16].contiguous(), s[1], x, None,
                               None, 0),                     # packed width
        lambda: ops.gemv_mxfp4(o, q[1], s[1][:, :2].contiguous(), x, None,
                               None, 0),                     # scale size
        lambda: ops.gemv_mxfp4(o, q[1].to(torch.int8), s[1], x, None, None,
                               0),                           # not uint8
        lambda: ops.gemv_mxfp4(o, q, s, x, None, None, 0, nw, None, 2,
                               eidx=e2, estride=q[0].numel()),  # LayerNorm
        lambda: ops.gemv_mxfp4(o, q, s, x, None, None, 0, eidx=e2,
                               estride=M * K),               # estride
        lambda: ops.gemv_swiglu_mxfp4(o, q, s, q, s[:2].contiguous(), x,
                                      False, eidx=e2, estride=q[0].numel()),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
        torch.cuda.synchronize()
        assert bool((buf.float() == R.SENTINEL).all()), i


def _dequantized_state(m):
    """m's state with every matrix the engine quantizes replaced by its
    mxfp4-dequantized value; the router weight stays."""
    sd = copy.deepcopy(m.state_dict())
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Linear) and not name.endswith("mlp.gate"):
            w = sd[name + ".weight"]
            sd[name + ".weight"] = dequantize_mxfp4(
                *quantize_mxfp4(w), w.size(1)).to(BF)
    return sd


def _engine_distance(monkeypatch, name, weights, use_graphs):
    """Mean over 6 teacher-forced steps of mean|logits - ref| / std(ref)
    (tests/test_attn_mha80_gpu.py), after a bf16 prompt on both sides; ref
    is the torch model, holding the dequantized weights under mxfp4.  Also
    (smallest top-k gate gap of ref, largest gate deviation of the eager
    engine) for a MoE config."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    if weights == "bf16":
        monkeypatch.delenv("MDI_WEIGHT_DTYPE", raising=False)
    else:
        monkeypatch.setenv("MDI_WEIGHT_DTYPE", weights)
    # seed chosen with the dequantized torch model alone, on the CPU: its
    # smallest top-2 gate gap on this schedule is 0.076
    cfg, m = G._build(name, seed=1295)
    m.set_kv_cache(1)
    st = G._starter(cfg, m, 1)
    eng = DecodeEngine(st, st.kv_pool, use_graphs=use_graphs)
    assert eng.mxfp4 == (weights == "mxfp4") and not eng.fp8 and not eng.int4
    if use_graphs:
        eng.capture_graphs()  # before the prompt: warm-up writes the cache
    else:
        eng.ops = spy = G._GateSpy(eng.ops)
    prompt = torch.randint(
        0, 511, (9,), generator=torch.Generator().manual_seed(1296)).to(DEV)
    ref = m(prompt.view(1, -1), input_pos=0, slot=0)[0, -1].float()
    st.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng.set_slot_pos(0, prompt.numel())
    if weights == "mxfp4":
        m.load_state_dict(_dequantized_state(m))
    gates = []
    hooks = [blk.mlp.gate.register_forward_hook(
        lambda _m, _i, out: gates.append(out.float().view(-1).clone()))
        for blk in m.transformer.h if hasattr(blk.mlp, "gate")]
    ds, gap, dev = [], float("inf"), 0.0
    for i in range(6):
        tok = ref.argmax().view(1)
        ref = m(tok.view(1, 1), input_pos=prompt.numel() + i,
                slot=0)[0, -1].float()
        got = eng.tail(eng.decode_step_head(tok.to(torch.int32), 0))
        ds.append(float((got.float().view(-1) - ref).abs().mean()
                        / ref.std()))
        if hooks and not use_graphs:
            for tg, eg in zip(gates, spy.logits):
                srt = tg.sort(descending=True).values
                k = cfg.n_expert_per_token
                gap = min(gap, float(srt[k - 1] - srt[k]))
                dev = max(dev, float((eg.view(-1) - tg).abs().max()))
            spy.logits.clear()
        gates.clear()
    for h in hooks:
        h.remove()
    return eng, sum(ds) / len(ds), gap, dev


@pytest.mark.parametrize("use_graphs", [False, True])
@pytest.mark.parametrize("name", ["nano-gpu", "nano-moe-gpu"])
@torch.inference_mode()
def test_engine_mxfp4_logits_vs_torch(monkeypatch, name, use_graphs):
    """The mxfp4 engine against the dequantized torch model is at most twice
    as far as the bf16 engine is from the bf16 torch model on the same
    schedule (the factor of tests/test_moe_fp8_gpu.py).  MoE: routing must
    not sit on a near-tie, or an expert flip could hide in the distance."""
    eng, d4, gap, dev = _engine_distance(monkeypatch, name, "mxfp4",
                                         use_graphs)
    w0 = eng.blocks[0]
    assert w0.attn_wmx.dtype == torch.uint8 and eng.head_wmx.size(0) > 0
    if name == "nano-moe-gpu":
        assert w0.fc1_wmx.dim() == 3 and not hasattr(w0, "gate_wmx")
    _, db, _, _ = _engine_distance(monkeypatch, name, "bf16", use_graphs)
    print(f"MXFP4_ENGINE {name} graphs={use_graphs} d_mxfp4={d4:.5f} "
          f"d_bf16={db:.5f} gate gap={gap:.4g} dev={dev:.4g}")
    assert gap > dev
    assert d4 <= 2 * db


@torch.inference_mode()
def test_group_engine_ignores_mxfp4(monkeypatch):
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "mxfp4")
    cfg, m = G._build("nano-gpu", seed=1291)
    stage = G._starter(cfg, m, 2)
    with pytest.warns(UserWarning, match="mxfp4"):
        geng = GroupDecodeEngine(stage, stage.kv_pool, 2, n_chunks=8)
    assert not hasattr(geng.blocks[0], "attn_wmx")
