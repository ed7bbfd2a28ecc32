"""Decode attention for head size 80 (q_per_kv == 1): attn_mha_block_kernel
and attn_mha_split_kernel + attn_combine_kernel against the fp64 reference
of attn_reference, through the checks of test_attn_decode_matrix_gpu's
run_and_check (error bound, appended row, untouched pools, guard elements,
raw qkv, which path ran).  The s_edge sizes sit round the 32-key tile and
the 128-key round of four waves."""

import pytest
import torch

from attn_reference import keys_per_chunk, make_case, pick_probes
from test_attn_decode_matrix_gpu import (DEV, Spec, _i32, _single, ops,  # noqa: F401
                                         run_and_check)

BF = torch.bfloat16


def _mha(name, family, n_kv, S, max_seq, cand, seed, rope_ne=32, **kw):
    return _single(name, family, 1, n_kv, 80, S, max_seq, cand, seed=seed,
                   rope_ne=rope_ne, **kw)


def _specs():
    out = []
    for i, ne in enumerate((0, 20, 32, 80)):
        out.append(_mha(f"geom-rope{ne}", "geom", 3, 83, 128,
                        [0, 15, 16, 64, -1], 901 + i, rope_ne=ne))
    for i, (S, max_seq) in enumerate(((1, 128), (31, 128), (32, 128),
                                      (33, 128), (127, 128), (128, 128),
                                      (129, 512), (257, 512))):
        out.append(_mha(f"s_edge-S{S}", "s_edge", 2, S, max_seq,
                        [0, 31, 32, 127, 128, -1], 920 + i,
                        paths=("block",)))
    for i, (n_chunks, S, max_seq) in enumerate(((4, 1, 128), (4, 33, 128),
                                                (4, 65, 128), (16, 257, 512),
                                                (256, 4096, 4096))):
        kpc = keys_per_chunk(S, n_chunks)
        own = ((S - 1) // kpc) * kpc  # first key of the chunk owning pos
        out.append(_mha(f"chunk_edge-c{n_chunks}-S{S}", "chunk_edge", 2, S,
                        max_seq, [0, kpc - 1, kpc, own, -1], 940 + i,
                        n_chunks=n_chunks, paths=("split",)))
    for i, mode in enumerate(("ascending", "descending", "outlier")):
        out.append(_mha(f"mode-{mode}", "mode", 2, 300, 512, [0, 150, -1],
                        960 + i, n_chunks=16, mode=mode))
    pos = (0, 37, 127)
    out.append(Spec("batched-B3", "batched",
                    dict(qpk=1, n_kv=2, hs=80, rope_ne=32, pos=list(pos),
                         slot=[2, 0, 1], max_seq=128, seed=970,
                         probes=[pick_probes(p + 1, [0, 15, 16, p - 1, p])
                                 for p in pos]),
                    8, extra=dict(n_batch=3)))
    out.append(_mha("implicit-maxseq8192", "implicit", 2, 300, 8192,
                    [0, 15, 16, -1], 980, n_chunks=32, paths=("split",),
                    force_split=False))
    return out


CASES = [(s, path, kv8) for s in _specs() for path in s.paths
         for kv8 in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize(
    "spec,path,kv8", CASES,
    ids=[f"{s.name}-{p}-{'fp8' if k else 'bf16'}" for s, p, k in CASES])
def test_attn_mha80(ops, spec, path, kv8):  # noqa: F811
    run_and_check(ops, spec, path, kv8)


@pytest.mark.gpu
def test_attn_mha80_gqa_refused_launches_nothing(ops):  # noqa: F811
    """Head size 80 has kernels for q_per_kv == 1 only."""
    case = make_case(qpk=2, n_kv=2, hs=80, pos=82, max_seq=128,
                     probes=[0, 82], seed=990)
    n = case.n_head * case.hs
    out = torch.full((n,), 12352.0, device=DEV, dtype=BF)
    kpool, vpool = case.kpool.to(DEV), case.vpool.to(DEV)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        ops.attn_decode(out, torch.zeros(n * 8, device=DEV),
                        torch.zeros(case.n_head * 16, device=DEV),
                        case.qkv.to(DEV).reshape(-1), kpool, vpool,
                        case.cos.to(DEV), case.sin.to(DEV), _i32(case.pos),
                        _i32(case.slot), case.layer, 8, case.scale)
    torch.cuda.synchronize()
    assert bool((out == 12352.0).all())
    assert torch.equal(kpool.cpu(), case.kpool)
    assert torch.equal(vpool.cpu(), case.vpool)


def _engine_distance(block_size, use_graphs, **over):
    """Mean over 6 teacher-forced decode steps of mean|logits - ref| /
    std(ref), DecodeEngine against the torch model, after a torch prompt."""
    from mdi_llm_amd import GPT, ModelConfig
    from mdi_llm_amd.models.stages import StarterStage
    from mdi_llm_amd.ops.engine import DecodeEngine, engine_supported
    from mdi_llm_amd.parallel.runner import make_runner

    cfg = ModelConfig.from_name("nano-neox-gpu", block_size=block_size,
                                **over)
    assert engine_supported(cfg)
    torch.manual_seed(1180)
    m = GPT(cfg)
    m.apply_init()
    m = m.to(device=DEV, dtype=BF).eval()
    m.set_kv_cache(1)
    st = StarterStage(cfg, cfg.n_layer).to(device=DEV, dtype=BF)
    st.load_state_dict(m.state_dict())
    st.eval()
    assert make_runner(st, 1, torch.device(DEV)).backend == "hip"
    st.set_kv_cache(1)
    eng = DecodeEngine(st, st.kv_pool, use_graphs=use_graphs)
    if use_graphs:
        eng.capture_graphs()  # before the prompt: warm-up writes the cache
    prompt = torch.randint(0, 511, (9,), device=DEV)
    ref = m(prompt.view(1, -1), input_pos=0, slot=0)[0, -1].float()
    st.forward_head(prompt.view(1, -1), slot=0, input_pos=0)
    eng.set_slot_pos(0, prompt.numel())
    ds = []
    for i in range(6):
        tok = ref.argmax().view(1)
        ref = m(tok.view(1, 1), input_pos=prompt.numel() + i,
                slot=0)[0, -1].float()
        got = eng.tail(eng.decode_step_head(tok.to(torch.int32), 0))
        ds.append(float((got.float().view(-1) - ref).abs().mean()
                        / ref.std()))
    return cfg, sum(ds) / len(ds)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graphs", [False, True])
@pytest.mark.parametrize("block_size", [256, 8192])  # block / split route
@torch.inference_mode()
def test_engine_head80_logits_vs_torch(block_size, use_graphs):
    """nano-neox-gpu widened to n_embd=320 (head size 80, rope_n_elem 20,
    LayerNorm, parallel residual, biases) on DecodeEngine.  The bound is
    twice the distance of the unmodified head-64 config on the existing
    kernels, same schedule (the factor of tests/test_moe_fp8_gpu.py).  The
    two are different models, so the steps are not paired: each distance
    is the mean over the six steps."""
    cfg, d80 = _engine_distance(block_size, use_graphs, n_embd=320)
    assert cfg.head_size == 80 and cfg.rope_n_elem == 20
    _, d64 = _engine_distance(block_size, use_graphs)
    print(f"MHA80_ENGINE block_size={block_size} graphs={use_graphs} "
          f"d80={d80:.5f} d64={d64:.5f}")
    assert d80 <= 2 * d64


def test_registry_head80_models_supported():
    from mdi_llm_amd import ModelConfig
    from mdi_llm_amd.ops.engine import engine_supported

    for name in ("phi-2", "pythia-2.8b", "stablelm-3b-4e1t", "stable-code-3b",
                 "RedPajama-INCITE-Base-3B-v1"):
        cfg = ModelConfig.from_name(name)
        assert cfg.head_size == 80 and engine_supported(cfg), name
    assert not engine_supported(ModelConfig.from_name("falcon-7b"))
    gqa = ModelConfig.from_name("phi-2", n_query_groups=16)
    assert gqa.head_size == 80 and gqa.q_per_kv == 2
    assert not engine_supported(gqa)
