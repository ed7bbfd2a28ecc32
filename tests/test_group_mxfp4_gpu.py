"""GPU: grouped decode on MXFP4 weights.  mtile_gemm_mxfp4 and
mtile_swiglu_mxfp4 against fp64 references on dequantize_mxfp4(...) under the
bounds of gemv_reference.py (the convert is exact, so the bf16 bounds apply
as they stand), element and scale placement by one-hot equality, the
refusals, and GroupDecodeEngine with MDI_WEIGHT_DTYPE=mxfp4 at B=16.

Worst err/bound printed by test_gemm_vs_fp64 on MI355X: see
profiles/group_mxfp4.md."""

import pytest
import torch

import gemv_reference as R
import prefill_reference as P
import test_group_moe_gpu as G
import test_mxfp4_gpu as MX
from mdi_llm_amd.ops.engine import dequantize_mxfp4, quantize_mxfp4

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
# chunk length of the kernel per padded batch (MtileMx in decode_kernels.hip)
KC = {16: 1024, 32: 512, 64: 512, 128: 512}


def _two_chunks_one_block(B):
    return 2 * KC[min(rb for rb in KC if rb >= B)] + 32


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _ybuf(B, M):
    buf = torch.full((B * M + R.PAD_ROWS,), R.SENTINEL, dtype=BF, device=DEV)
    return buf, buf[:B * M].view(B, M)


def _quantized(w):
    """(packed, scales) on the GPU and the fp32 weights they stand for."""
    q, s = quantize_mxfp4(w)
    return q.to(DEV), s.to(DEV), dequantize_mxfp4(q, s, w.size(1))


def _d(t):
    return None if t is None else t.to(DEV)


def test_placement_exact(ops):
    """Row p holds one nonzero per block, at position p, with the block's
    own exponent; X row b is one-hot at k_b, so Y[b] is column k_b, bit for
    bit.  Blocks: the four sub-lanes of super-step 0 and the first of the
    next, both sides of a scale byte and of the 256-block period."""
    nb = 257
    K = nb * 32
    b = torch.arange(nb)
    val = (1 + 0.5 * (b % 2)) * (1 - 2 * (b % 3 == 0)) * 2.0 ** (b % 15 - 7)
    w = torch.zeros(32, nb, 32)
    w[torch.arange(32), :, torch.arange(32)] = val
    w = w.view(32, K).to(BF)
    q, s, deq = _quantized(w)
    assert torch.equal(deq, w.float())
    blocks = (0, 1, 3, 4, 63, 64, 255, 256)
    pos = (1, 30, 9, 18, 6, 27, 12, 23, 0, 31, 15, 16, 7, 8, 20, 29)
    ks = [blocks[i // 2] * 32 + p for i, p in enumerate(pos)]
    X = torch.zeros(16, K, dtype=BF)
    X[torch.arange(16), ks] = 1.0
    buf, Y = _ybuf(16, 32)
    ops.mtile_gemm_mxfp4(Y, q, s, X.to(DEV), None, None)
    assert torch.equal(Y.cpu(), w[:, ks].t())
    assert bool((buf[16 * 32:].float() == R.SENTINEL).all())


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias-res"])
@pytest.mark.parametrize("M", [16, 48])
@pytest.mark.parametrize("K", [32, 688, 8192 + 64, "2ch+1"])
@pytest.mark.parametrize("B", [5, 16, 32, 40, 64, 128])
def test_gemm_vs_fp64(ops, B, K, M, extras):
    _check_gemm(ops, B, _two_chunks_one_block(B) if K == "2ch+1" else K, M,
                extras)


@pytest.mark.parametrize("K", [24576 + 32, 28672, 32768])
@pytest.mark.parametrize("B", [32, 64, 128])
def test_gemm_large_k(ops, B, K):
    """Up to ops.MTILE_MXFP4_MAX_K; past 24576 the scale rows of two row
    tiles (RB >= 64) sit unpadded in LDS.  28672 is the 70B Llamas' down
    GEMM; M = 48 leaves the second row tile of the last block empty."""
    assert ops.MTILE_MXFP4_MAX_K == 32768
    _check_gemm(ops, B, K, 48, True)


def _check_gemm(ops, B, K, M, extras):
    case = P.MtileCase(B, K, M, extras, extras)
    inp = P.make_mtile_inputs(case)
    q, s, inp.W = _quantized(inp.W)
    r = P.mtile_reference(inp)
    buf, Y = _ybuf(B, M)
    ops.mtile_gemm_mxfp4(Y, q, s, _d(inp.X), _d(inp.bias), _d(inp.res))
    host = buf.cpu()
    ok, worst = P.mtile_error_ok(host[:B * M].view(B, M), r, K)
    print(f"MTILE_MXFP4_RATIO {case.id} {worst:.4f}")
    assert bool((host[B * M:].float() == R.SENTINEL).all()), "wrote past Y"
    assert not bool((host[:B * M].float() == R.SENTINEL).any()), \
        "an element of Y was never written"
    assert ok, f"{case.id}: err/bound {worst:.3g}"


@pytest.mark.parametrize("gelu", [False, True], ids=["silu", "gelu"])
@pytest.mark.parametrize("M", [16, 48])
@pytest.mark.parametrize("K", [688, "2ch+1"])
@pytest.mark.parametrize("B", [16, 64])
def test_swiglu_vs_fp64(ops, B, K, M, gelu):
    K = _two_chunks_one_block(B) if K == "2ch+1" else K
    inp = P.make_mtile_inputs(P.MtileCase(B, K, M, False, False))
    up = P.make_mtile_inputs(P.MtileCase(B, K, M, True, False)).W
    gq, gs, gdeq = _quantized(inp.W)
    uq, us, udeq = _quantized(up)
    wg, wu = R.Weights("bf16", K, w=gdeq), R.Weights("bf16", K, w=udeq)
    buf, ACT = _ybuf(B, M)
    ops.mtile_swiglu_mxfp4(ACT, gq, gs, uq, us, inp.X.to(DEV), gelu)
    host = buf.cpu()
    assert bool((host[B * M:].float() == R.SENTINEL).all()), "wrote past ACT"
    for b in range(B):
        ref = R.gemv_swiglu_ref(wg, wu, inp.X[b], gelu)
        row = torch.cat([host[b * M:(b + 1) * M], host[B * M:]])
        ok, _, msg = R.check_out_buffer(row, M, ref, K)
        assert ok, (b, msg)


@pytest.mark.parametrize("which", ["packed-width", "scale-size", "not-uint8",
                                   "M-24", "B-129", "K-36", "K-32800",
                                   "X-strided"])
def test_refuses_before_launch(ops, which):
    shape = {"M-24": (16, 64, 24), "B-129": (129, 64, 32),
             "K-36": (16, 36, 32), "K-32800": (64, 32800, 32)}
    B, K, M = shape.get(which, (16, 64, 32))
    q, s, _ = _quantized(torch.ones(M, K, dtype=BF))
    X = torch.ones(B, 2 * K, dtype=BF, device=DEV)
    X = X[:, :K] if which == "X-strided" else X[:, :K].contiguous()
    if which == "packed-width":
        q = q[:, :16].contiguous()
    if which == "scale-size":
        s = s[:, :4].contiguous()
    if which == "not-uint8":
        q = q.to(torch.int8)
    buf, Y = _ybuf(B, M)
    with pytest.raises(RuntimeError):
        ops.mtile_gemm_mxfp4(Y, q, s, X, None, None)
    torch.cuda.synchronize()
    assert bool((buf.float() == R.SENTINEL).all()), "something was launched"


# ---------------------------------------------------------------------------
# engine: nano-gpu at B=16 (K = 688 and M = 688 occur), distinct prompt lengths
B_ENG, N_STEPS, SEED = 16, 6, 1297


def _engines(monkeypatch, graphs):
    """(cfg, torch model, [(stage, GroupDecodeEngine)]), prompts run in bf16
    on every side, first tokens; one engine per entry of `graphs`."""
    from mdi_llm_amd.ops.group_engine import GroupDecodeEngine

    monkeypatch.setenv("MDI_WEIGHT_DTYPE", "mxfp4")
    cfg, m = G._build("nano-gpu", seed=SEED)
    m.set_kv_cache(B_ENG)
    pairs = []
    for use_graphs in graphs:
        st = G._starter(cfg, m, B_ENG)
        with pytest.warns(UserWarning, match="mtile_gemm_mxfp4"):
            eng = GroupDecodeEngine(st, st.kv_pool, B_ENG, n_chunks=8,
                                    use_graphs=use_graphs)
        assert eng.mxfp4 and eng.blocks[0].attn_wmx.dtype == torch.uint8
        if use_graphs:
            eng.ensure_graphs(0.0, 0, 0)  # greedy; before prefill
        pairs.append((st, eng))
    g = torch.Generator().manual_seed(SEED + 1)
    prompts = [torch.randint(0, 511, (3 + s,), generator=g).to(DEV)
               for s in range(B_ENG)]
    toks = []
    for s, p in enumerate(prompts):
        toks.append(int(m(p.view(1, -1), input_pos=0, slot=s)[0, -1].float()
                        .argmax()))
        for st, eng in pairs:
            st.forward_head(p.view(1, -1), slot=s, input_pos=0)
            eng.set_slot_pos(s, p.numel())
    return cfg, m, pairs, prompts, toks


@torch.inference_mode()
def test_group_mxfp4_logits_vs_torch(monkeypatch):
    """Per-slot eager logits against the torch model holding the dequantized
    weights, 6 teacher-forced steps.  Yardstick: DecodeEngine under mxfp4 on
    the same slot and step reads the same packed weights, so the grouped path
    differs only by fp32 reassociation and must stay below twice its distance
    (the factor of test_group_moe_logits_vs_torch)."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, m, [(_, geng)], prompts, toks = _engines(monkeypatch, [False])
    s1 = G._starter(cfg, m, B_ENG)
    eng1 = DecodeEngine(s1, s1.kv_pool, n_chunks=8, use_graphs=False)
    assert eng1.mxfp4
    for s, p in enumerate(prompts):
        s1.forward_head(p.view(1, -1), slot=s, input_pos=0)
        eng1.set_slot_pos(s, p.numel())
    m.load_state_dict(MX._dequantized_state(m))
    pos = [p.numel() for p in prompts]
    slots = torch.arange(B_ENG, device=DEV, dtype=torch.int32)
    worst = 0.0
    for step in range(N_STEPS):
        geng.token_table.copy_(torch.tensor(toks, dtype=torch.int32))
        geng.set_group(slots)
        geng.head_step()
        geng._tail_seq()
        glogits = geng.LOGITS.float().clone()
        for s in range(B_ENG):
            tok = torch.tensor([toks[s]], device=DEV, dtype=torch.int32)
            ref = m(tok.view(1, 1).long(), input_pos=pos[s],
                    slot=s)[0, -1].float()
            base = G._rel(eng1.tail(eng1.decode_step_head(tok, s)).float()
                          .view(-1), ref)
            rel = G._rel(glogits[s], ref)
            worst = max(worst, rel / base)
            assert rel < 2 * base, (step, s, rel, base)
            toks[s] = int(ref.argmax())
            pos[s] += 1
    print(f"GROUP_MXFP4 worst grouped/single-sample distance {worst:.3f}")


@torch.inference_mode()
def test_group_mxfp4_graph_matches_eager(monkeypatch):
    """The captured step against eager stepping over 6 greedy steps: the
    graph's pick is a maximum of the eager logits
    (test_group_moe_graph_matches_eager's criterion)."""
    _, _, [(_, eng_g), (_, eng_e)], _, toks = _engines(monkeypatch,
                                                       [True, False])
    for eng in (eng_g, eng_e):
        eng.token_table[:B_ENG] = torch.tensor(toks, dtype=torch.int32)
    slots = torch.arange(B_ENG, device=DEV, dtype=torch.int32)
    for step in range(N_STEPS):
        eng_g.set_group(slots)
        eng_g.standalone_step()
        got = eng_g.token_table.clone()
        eng_e.set_group(slots)
        eng_e.head_step()
        eng_e._tail_seq()
        logits = eng_e.LOGITS.float()
        picked = logits.gather(1, got.long().view(B_ENG, 1)).view(B_ENG)
        assert torch.equal(picked, logits.max(dim=1).values), (
            step, got.tolist(), logits.argmax(dim=1).tolist())
        eng_e.token_table.copy_(got)
    assert bool(torch.isfinite(logits).all())
