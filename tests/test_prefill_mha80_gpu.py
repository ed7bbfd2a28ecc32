"""GPU: HIP prefill for head size 80 and for the LayerNorm / parallel-
residual family.  prefill_attn at hs 80, qpk 1 against the fp64 reference
of prefill_reference.py under its derived bf16-P bound C_V2 (no tolerance is
set here); layernorm over rows against its own one-row calls; the engine
prefill against the torch stage in fp32, bounded by twice the distance of
the bf16 torch stage (the path these configs ran before).

Prints PREFILL_RATIO / PREFILL_D lines; profiles/prefill_mha80.md keeps the
figures of one run.
"""

import pytest
import torch

import prefill_reference as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def _matrix():
    spec = [(f"qtile-T{T}", dict(T=T, pos0=0)) for T in (1, 15, 16, 17, 33)]
    spec += [(f"chunk-S{S}-T{T}", dict(T=T, pos0=S - T))
             for S in (63, 64, 65, 129) for T in (1, 17)]
    spec += [(f"full-pos{p}", dict(T=17, pos0=p)) for p in (47, 48, 63, 64)]
    # 130 rows: blocks of four q tiles with four causal bounds, and a last
    # block with one live wave
    spec += [(f"multi-T130-pos{p}", dict(T=130, pos0=p)) for p in (0, 60)]
    spec += [(f"mode-{m}", dict(T=60, pos0=240, mode=m))
             for m in ("ascending", "descending", "outlier")]
    return {f"mha80-{n}-{'fp8' if kv8 else 'bf16'}": dict(kv8=kv8, **kw)
            for kv8 in (False, True) for n, kw in spec}


MATRIX = _matrix()


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


@pytest.mark.parametrize("name", list(MATRIX))
def test_prefill_mha80_matrix(ops, name):
    case = P.make_prefill_case(name=name, qpk=1, hs=80, **MATRIX[name])
    ref = case.reference()
    assert case.probes_ok(ref), (case.probe_weights(ref),
                                 case.leak_margins())
    buf, dev = P.run_prefill(ops, case, DEV)
    torch.cuda.synchronize()
    ok, ratio, msg = P.check_prefill(case, ref, buf, dev, P.C_V2)
    print(f"PREFILL_RATIO {name} {ratio:.4f}")
    assert ok, f"{name}: {msg}"


def test_head80_gqa_is_refused(ops):
    case = P.make_prefill_case(name="mha80-qpk2", qpk=2, hs=80, T=4, pos0=0)
    with pytest.raises(RuntimeError, match="unsupported head_size 80"):
        P.run_prefill(ops, case, DEV)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows,n", [(1, 256), (3, 320), (17, 2560)])
def test_layernorm_rows(ops, rows, n, bias):
    gen = torch.Generator().manual_seed(rows * n + bias)
    x = (torch.randn(rows, n, generator=gen) * 2 + 0.5).to(BF).to(DEV)
    w = torch.randn(n, generator=gen).to(BF).to(DEV)
    b = torch.randn(n, generator=gen).to(BF).to(DEV) if bias else None
    buf = torch.full((rows * n + P.PAD,), P.SENTINEL, dtype=BF, device=DEV)
    ops.layernorm(buf[:rows * n].view(rows, n), x, w, b, 1e-5)
    for r in range(rows):
        one = torch.empty(n, dtype=BF, device=DEV)
        ops.layernorm(one, x[r], w, b, 1e-5)
        assert torch.equal(buf[r * n:(r + 1) * n], one), r
    assert bool((buf[rows * n:].float() == P.SENTINEL).all())


# ---------------------------------------------------------------------------
NEOX80 = dict(n_embd=320)
ENGINE_CONFIGS = {
    "neox-head64": {},
    "neox-head80": NEOX80,
    "phi-block-head80": dict(n_embd=320, shared_attention_norm=True,
                             gelu_approximate="tanh", lm_head_bias=True),
    "sequential-learned-pos": dict(parallel_residual=False,
                                   rotary_percentage=0.0,
                                   pos_embedding="learned"),
}
T_PROMPT = 40


def _d(x, truth):
    """mean|x - truth| / std(truth), the metric of profiles/attn_mha80.md."""
    return float((x.float() - truth).abs().mean() / truth.std())


def _stages(name, over, seed):
    """(cfg, [bf16 engine stage, bf16 torch stage, fp32 torch stage]) on one
    set of bf16 weights, two cache slots each."""
    from mdi_llm_amd import GPT, ModelConfig
    from mdi_llm_amd.models.stages import StarterStage

    cfg = ModelConfig.from_name(name, **over)
    torch.manual_seed(seed)
    m = GPT(cfg)
    m.apply_init()
    m = m.to(device=DEV, dtype=BF)
    out = []
    for dtype in (BF, BF, torch.float32):
        st = StarterStage(cfg, cfg.n_layer).to(device=DEV, dtype=dtype)
        st.load_state_dict(m.state_dict())
        st.eval()
        st.set_kv_cache(2)
        out.append(st)
    return cfg, out


@torch.inference_mode()
@pytest.mark.parametrize("which", list(ENGINE_CONFIGS))
def test_engine_prefill_family(which):
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, (st, ref, truth) = _stages("nano-neox-gpu", ENGINE_CONFIGS[which],
                                    seed=4080)
    eng = DecodeEngine(st, st.kv_pool, n_chunks=8, use_graphs=False)
    assert eng.supports_hip_prefill
    prompt = torch.randint(0, 511, (T_PROMPT,), device=DEV)
    x_t = truth.forward_head(prompt.view(1, -1), slot=0, input_pos=0)[0]
    x_b = ref.forward_head(prompt.view(1, -1), slot=0, input_pos=0)[0]
    x_h = eng.prefill_prompt(prompt, slot=0, pos0=0)
    eng.prefill_prompt(prompt[:16], slot=1, pos0=0)
    x_s = eng.prefill_prompt(prompt[16:], slot=1, pos0=16)
    d_hip, d_split, d_torch = _d(x_h, x_t), _d(x_s, x_t[16:]), _d(x_b, x_t)
    print(f"PREFILL_D {which} hip {d_hip:.5f} split {d_split:.5f} "
          f"torch-bf16 {d_torch:.5f}")
    assert d_hip <= 2 * d_torch
    assert d_split <= 2 * _d(x_b[16:], x_t[16:])
    for nm in ("k", "v"):
        rows = [getattr(s.kv_pool, nm)[0, :, :, :T_PROMPT]
                for s in (st, ref, truth)]
        d_pool, d_pool_torch = _d(rows[0], rows[2]), _d(rows[1], rows[2])
        print(f"PREFILL_D {which} pool-{nm} hip {d_pool:.5f} torch-bf16 "
              f"{d_pool_torch:.5f}")
        assert d_pool <= 2 * d_pool_torch

    # a greedy decode step off the HIP-filled cache: torch-on-torch's argmax
    eng.set_slot_pos(0, T_PROMPT)
    tok = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    l_hip = eng.tail(eng.decode_step_head(tok, slot=0))
    ref.kv_pool.seq_len[0] = T_PROMPT
    l_ref = ref.forward_tail(ref.forward_head(tok.long().view(1, 1), slot=0,
                                              input_pos=T_PROMPT))
    assert int(l_hip.float().argmax()) == int(l_ref.view(-1).float().argmax())


def _fp8_kv_distance(name, over):
    """d of the prefill output under an fp8 KV cache; also checks that the
    cache is fp8 and that one decode step off it is finite."""
    from mdi_llm_amd.ops.engine import DecodeEngine

    cfg, (st, _, truth) = _stages(name, over, seed=4081)
    eng = DecodeEngine(st, st.kv_pool, n_chunks=8, use_graphs=False)
    assert eng.kv8 and st.kv_pool.k.dtype == torch.uint8 \
        and st.kv_pool.v.dtype == torch.uint8
    prompt = torch.randint(0, 511, (T_PROMPT,), device=DEV)
    x_t = truth.forward_head(prompt.view(1, -1), slot=0, input_pos=0)[0]
    x_h = eng.prefill_prompt(prompt, slot=0, pos0=0)
    eng.set_slot_pos(0, T_PROMPT)
    tok = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    logits = eng.tail(eng.decode_step_head(tok, slot=0))
    assert bool(torch.isfinite(logits.float()).all())
    return _d(x_h, x_t)


@torch.inference_mode()
def test_engine_fp8_kv_head80(monkeypatch):
    """MDI_KV_DTYPE=fp8 now takes effect on the head-80 config; its distance
    to the fp32 truth is held against nano-gpu's, whose path is unchanged."""
    monkeypatch.setenv("MDI_KV_DTYPE", "fp8")
    d80 = _fp8_kv_distance("nano-neox-gpu", NEOX80)
    d_base = _fp8_kv_distance("nano-gpu", {})
    print(f"PREFILL_D fp8-kv neox-head80 {d80:.5f} nano-gpu {d_base:.5f}")
    assert d80 <= 2 * d_base
