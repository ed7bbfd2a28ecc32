"""CPU: which configs DecodeEngine.prefill_hidden takes (the dense rule is
the engine's own support plus a head geometry prefill_attn runs)."""

import pytest

from mdi_llm_amd import ModelConfig
from mdi_llm_amd.ops.engine import hip_prefill_supported

TABLE = [
    ("phi-2", {}, True),
    ("nano-neox-gpu", {}, True),
    ("nano-neox-gpu", dict(n_embd=320), True),            # head 80, MHA
    ("phi-2", dict(n_query_groups=16), False),            # head 80, qpk 2
    ("pythia-14m", {}, False),                            # head 32
    ("Meta-Llama-3-8B-Instruct", {}, True),
    ("nano-moe-gpu", {}, True),
]


@pytest.mark.parametrize("name,over,want", TABLE)
def test_hip_prefill_supported(name, over, want):
    cfg = ModelConfig.from_name(name, **over)
    if over.get("n_embd") == 320:
        assert cfg.head_size == 80 and cfg.q_per_kv == 1
    if "n_query_groups" in over:
        assert cfg.head_size == 80 and cfg.q_per_kv == 2
    assert hip_prefill_supported(cfg) is want
