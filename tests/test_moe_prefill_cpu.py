"""CPU: which configs take the HIP prefill path (moe_prefill_supported and
the dense rule it sits beside)."""

from mdi_llm_amd import ModelConfig
from mdi_llm_amd.ops.engine import (hip_prefill_supported,
                                    moe_prefill_supported)


def test_moe_prefill_supported():
    assert moe_prefill_supported(ModelConfig.from_name("nano-moe-gpu"))
    assert moe_prefill_supported(ModelConfig.from_name("Mixtral-8x7B-v0.1"))


def test_moe_prefill_refuses_odd_intermediate_size():
    bad = ModelConfig.from_name("nano-moe-gpu", intermediate_size=208)
    assert bad.intermediate_size % 32 != 0
    assert not moe_prefill_supported(bad)
    assert not hip_prefill_supported(bad)  # torch fallback, as before


def test_moe_prefill_refuses_out_of_range_routing():
    for kw in (dict(n_expert=128), dict(n_expert=16, n_expert_per_token=9),
               dict(n_expert_per_token=5), dict(parallel_residual=True),
               dict(norm_class_name="LayerNorm")):
        cfg = ModelConfig.from_name("nano-moe-gpu", **kw)
        assert not moe_prefill_supported(cfg), kw


def test_dense_configs_unaffected():
    for name in ("nano-gpu", "Meta-Llama-3-8B-Instruct"):
        cfg = ModelConfig.from_name(name)
        assert not moe_prefill_supported(cfg)
        assert hip_prefill_supported(cfg)
    # a dense family the HIP prefill never ran stays on the torch path
    neox = ModelConfig.from_name("pythia-14m")
    assert not hip_prefill_supported(neox)
