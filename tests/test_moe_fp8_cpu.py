"""CPU: fp8 expert slabs for MoE decode — the slab quantizer against
quantize_fp8_rowwise, and how _BlockWeights.quantize_fp8 attaches, shares
and refreshes the slabs on a nano-moe-gpu block."""

import torch


def _block(seed=0):
    from mdi_llm_amd import ModelConfig
    from mdi_llm_amd.models.model import Block

    torch.manual_seed(seed)
    cfg = ModelConfig.from_name("nano-moe-gpu")
    blk = Block(cfg, 0).to(torch.bfloat16)
    return cfg, blk


def _bits(t):
    return t.view(torch.uint8)


def test_slab_quantizer_matches_rowwise():
    from mdi_llm_amd.ops.engine import (quantize_fp8_rowwise,
                                        quantize_fp8_slab)

    torch.manual_seed(1)
    n_e, M, K = 4, 224, 256
    slab = (torch.randn(n_e, M, K) / 16).to(torch.bfloat16)
    slab[1, 3] = 0  # an all-zero row takes the clamped scale
    slab[2] *= 37.0  # experts must not share a scale
    q, s = quantize_fp8_slab(slab)
    assert q.dtype == torch.float8_e4m3fn and q.shape == (n_e, M, K)
    assert s.dtype == torch.float32 and s.shape == (n_e, M)
    assert q.is_contiguous() and s.is_contiguous()
    for e in range(n_e):
        qe, se = quantize_fp8_rowwise(slab[e])
        assert torch.equal(_bits(q[e]), _bits(qe)), e
        assert torch.equal(s[e], se), e
    assert not torch.equal(s[2], s[0])


def test_block_weights_attach_share_and_refresh():
    from mdi_llm_amd.ops.engine import _BlockWeights, quantize_fp8_rowwise

    cfg, blk = _block()
    w = _BlockWeights(blk, cfg)
    w.quantize_fp8(cfg)
    n_e, E, I = cfg.n_expert, cfg.n_embd, cfg.intermediate_size
    for name, shape in (("fc1", (n_e, I, E)), ("fc2", (n_e, I, E)),
                        ("mlp_proj", (n_e, E, I))):
        q, s = getattr(w, name + "_w8"), getattr(w, name + "_s")
        assert q.dtype == torch.float8_e4m3fn and q.shape == shape
        assert s.shape == shape[:2]
    assert hasattr(w, "attn_w8") and hasattr(w, "proj_w8")
    # the router weight has no fp8 twin and is the module's bf16 weight
    assert not hasattr(w, "gate_w8") and not hasattr(w, "gate_s")
    assert w.gate_w.dtype == torch.bfloat16
    assert torch.equal(w.gate_w, blk.mlp.gate.weight)
    # the bf16 slabs stay
    assert w.fc1_w.dtype == torch.bfloat16 and w.fc1_w.shape == (n_e, I, E)
    qe, se = quantize_fp8_rowwise(blk.mlp.experts[2].proj.weight.detach())
    assert torch.equal(_bits(w.mlp_proj_w8[2]), _bits(qe))
    assert torch.equal(w.mlp_proj_s[2], se)

    # a second _BlockWeights on the same block shares the storage
    w2 = _BlockWeights(blk, cfg)
    w2.quantize_fp8(cfg)
    for name in ("fc1_w8", "fc1_s", "fc2_w8", "fc2_s", "mlp_proj_w8",
                 "mlp_proj_s", "fc1_w"):
        assert getattr(w2, name).data_ptr() == getattr(w, name).data_ptr()

    # replaced weights are stacked and quantized afresh
    old = _bits(w.fc1_w8).clone()
    sd = {k: v * 0.5 if "experts.1.fc_1" in k else v
          for k, v in blk.state_dict().items()}
    sd["mlp.experts.0.fc_1.weight"] = torch.randn(I, E).to(torch.bfloat16)
    blk.load_state_dict(sd)
    w3 = _BlockWeights(blk, cfg)
    w3.quantize_fp8(cfg)
    q0, s0 = quantize_fp8_rowwise(blk.mlp.experts[0].fc_1.weight.detach())
    assert torch.equal(_bits(w3.fc1_w8[0]), _bits(q0))
    assert torch.equal(w3.fc1_s[0], s0)
    assert not torch.equal(_bits(w3.fc1_w8[0]), old[0])
    # scaling a row by 0.5 keeps its codes and halves its scale
    assert torch.equal(_bits(w3.fc1_w8[1]), old[1])
    assert torch.equal(w3.fc1_s[1], w.fc1_s[1] * 0.5)
    assert w3.fc1_w8.data_ptr() == blk.mlp._hip_expert_slabs_fp8[1][0] \
        .data_ptr()
