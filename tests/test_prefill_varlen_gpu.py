"""GPU: batched (varlen) prefill.  rope_prefill_append_varlen and
prefill_attn_varlen on one pack of five prompts against the fp64 references
of prefill_reference.py (prefill_attn under its derived bf16-P bound C_V2; no
tolerance is set here), the host guards, DecodeEngine.prefill_prompts against
the fp32 torch stage with the per-prompt engine path as the yardstick, and
generate() under MDI_PREFILL_BATCH=1.

The pack: T = 1, an exact q tile, a tile + 1, tiles that would straddle the
neighbour's rows, and more than one 64-key chunk; two prompts start at
pos0 > 0 behind pre-filled keys.  Slot 2 stays unused.
"""

import pytest
import torch

import prefill_reference as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
N_KV, N_SLOTS, N_LAYERS, LAYER, MAX_SEQ, FREE_SLOT = 2, 6, 2, 1, 128, 2
LENS, POS0S, SLOTS = [1, 16, 17, 33, 70], [0, 0, 0, 5, 3], [3, 0, 5, 1, 4]
T_TOTAL = sum(LENS)
KV = pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _batch(ops, qpk, hs, kv8, rope_ne, seed=0):
    """Host inputs of one varlen call: raw qkv [T_TOTAL, qkv_dim], N(0,1)
    pools [k, v, kscale, vscale] with slot 2 sentinel-filled, rope tables,
    and the device table."""
    from mdi_llm_amd.ops.engine import prefill_varlen_table

    gen = torch.Generator().manual_seed(1000 * hs + 10 * qpk + kv8 + 7 * seed)
    raw = torch.randn(T_TOTAL, N_KV * (qpk + 2) * hs, generator=gen).to(BF)
    shape = (N_SLOTS, N_LAYERS, N_KV, MAX_SEQ, hs)
    kf = torch.randn(shape, generator=gen)
    vf = torch.randn(shape, generator=gen)
    if kv8:
        (k, ks), (v, vs) = P.fp8_quant_rows(kf), P.fp8_quant_rows(vf)
        k[FREE_SLOT] = v[FREE_SLOT] = P.FP8_GARBAGE_BYTE
        ks[FREE_SLOT] = vs[FREE_SLOT] = P.FP8_GARBAGE_SCALE
    else:
        k, v, ks, vs = kf.to(BF), vf.to(BF), None, None
        k[FREE_SLOT] = v[FREE_SLOT] = P.SENTINEL
    cos, sin = P.rope_tables(MAX_SEQ, rope_ne)
    tab = prefill_varlen_table(LENS, SLOTS, POS0S,
                               ops.prefill_varlen_qtpb(qpk), MAX_SEQ,
                               N_SLOTS, DEV)
    return dict(raw=raw, pools=[k, v, ks, vs], cos=cos, sin=sin, tab=tab)


def _dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _host(ts):
    return [None if t is None else t.cpu() for t in ts]


def _padded(t):
    """(buffer with P.PAD sentinels behind it, view of t's shape) on DEV."""
    buf = torch.full((t.numel() + P.PAD,), P.SENTINEL, dtype=BF, device=DEV)
    buf[:t.numel()] = t.to(DEV).flatten()
    return buf, buf[:t.numel()].view(t.shape)


def _rope(ops, b, qkv, dev, lists=(LENS, SLOTS, POS0S), tab=None):
    ops.rope_prefill_append_varlen(
        qkv, dev[0], dev[1], b["cos"].to(DEV), b["sin"].to(DEV),
        b["tab"] if tab is None else tab, *lists, LAYER, kscale=dev[2],
        vscale=dev[3])


def _attn(ops, b, out, qkv, dev, hs, lists=(LENS, SLOTS, POS0S), tab=None):
    ops.prefill_attn_varlen(out, qkv, dev[0], dev[1],
                            b["tab"] if tab is None else tab, *lists, LAYER,
                            hs ** -0.5, kscale=dev[2], vscale=dev[3])


def _assert_only_rows_written(before, after):
    """Nothing but [slot, LAYER, :, pos0:pos0+T] of the used slots changed:
    slot 2, the other layer, earlier keys and rows >= pos0 + T are as
    given."""
    for b, a in zip(before, after):
        if b is None:
            continue
        want = b.clone()
        for T, p0, s in zip(LENS, POS0S, SLOTS):
            want[s, LAYER, :, p0:p0 + T] = a[s, LAYER, :, p0:p0 + T]
        assert torch.equal(a, want), "a row outside the appended ones changed"


@KV
@pytest.mark.parametrize("hs,qpk", [(64, 1), (64, 2), (128, 4), (128, 8),
                                    (256, 2)])
def test_attn_varlen(ops, hs, qpk, kv8):
    b = _batch(ops, qpk, hs, kv8, hs)
    qkv, dev = b["raw"].to(DEV), _dev(b["pools"])
    _rope(ops, b, qkv, dev)
    n = T_TOTAL * N_KV * qpk * hs
    buf = torch.full((n + P.PAD,), P.SENTINEL, dtype=BF, device=DEV)
    _attn(ops, b, buf[:n].view(T_TOTAL, -1), qkv, dev, hs)
    torch.cuda.synchronize()
    host, roped, after = buf.cpu(), qkv.cpu(), _host(dev)
    assert bool((host[n:].float() == P.SENTINEL).all()), "pad behind out"
    out, r0 = host[:n].view(T_TOTAL, -1), 0
    for T, p0, s in zip(LENS, POS0S, SLOTS):
        ref = P.prefill_reference(roped[r0:r0 + T], after[0], after[1], p0,
                                  s, LAYER, hs ** -0.5, after[2], after[3])
        got = out[r0:r0 + T].contiguous()
        print(f"VARLEN_RATIO hs{hs} qpk{qpk} fp8={kv8} T{T} pos0 {p0}: "
              f"{P.prefill_error_ratio(got, ref.out, ref.A, P.C_V2):.4f}")
        assert P.prefill_error_ok(got, ref.out, ref.A, P.C_V2), (T, p0, s)
        r0 += T
    _assert_only_rows_written(b["pools"], after)


def _ulps(a, b):
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


@KV
@pytest.mark.parametrize("qpk,hs,ne", [(4, 128, 128), (1, 64, 16),
                                       (2, 256, 0)])
def test_rope_append_varlen(ops, qpk, hs, ne, kv8):
    cu = [sum(LENS[:i]) for i in range(len(LENS) + 1)]
    for seed in range(64):  # as make_rope_case: no near-total cancellation
        b = _batch(ops, qpk, hs, kv8, ne, seed)
        if all(P.rope_condition(b["raw"][cu[i]:cu[i + 1]], b["cos"], b["sin"],
                                POS0S[i], N_KV, hs) >= P.ROPE_COND
               for i in range(len(LENS))):
            break
    else:
        raise AssertionError("no well-conditioned seed")
    (buf, qkv), dev = _padded(b["raw"]), _dev(b["pools"])
    _rope(ops, b, qkv, dev)
    # the single-sequence op on the same rows, from the same pools
    (buf1, qkv1), dev1 = _padded(b["raw"]), _dev(b["pools"])
    for i, (T, p0, s) in enumerate(zip(LENS, POS0S, SLOTS)):
        ops.rope_prefill_append(qkv1[cu[i]:cu[i + 1]], dev1[0], dev1[1],
                                b["cos"].to(DEV), b["sin"].to(DEV), p0, s,
                                LAYER, kscale=dev1[2], vscale=dev1[3])
    torch.cuda.synchronize()
    assert torch.equal(buf, buf1), "qkv differs from the per-sequence op"
    after = _host(dev)
    for a, a1 in zip(after, _host(dev1)):
        assert a is None or torch.equal(a, a1), \
            "a pool differs from the per-sequence op"
    _assert_only_rows_written(b["pools"], after)
    got = buf.cpu()[:b["raw"].numel()].view(T_TOTAL, N_KV, qpk + 2, hs)
    raw = b["raw"].view(T_TOTAL, N_KV, qpk + 2, hs)
    assert torch.equal(got[:, :, -1], raw[:, :, -1]), "a v row was changed"
    for i, (T, p0) in enumerate(zip(LENS, POS0S)):
        want = P.rope_append_reference(b["raw"][cu[i]:cu[i + 1]], b["cos"],
                                       b["sin"], p0, N_KV, hs)
        d = _ulps(got[cu[i]:cu[i + 1], :, :-1],
                  want.to(torch.float32).to(BF)[:, :, :-1])
        assert int(d.max()) <= 1, f"seq {i}: q/k off by {int(d.max())} ulp"


# one refused edit of the accepted (lists, table) each
GUARDS = {
    "drop_slot": dict(lists=(LENS, SLOTS[:-1], POS0S)),
    "dup_slot": dict(lists=(LENS, [3, 0, 5, 1, 3], POS0S)),
    "zero_len": dict(lists=([1, 0, 17, 33, 70], SLOTS, POS0S)),
    "overflow": dict(lists=(LENS, SLOTS, [0, 0, 0, 5, MAX_SEQ - 69])),
    "short_table": dict(tab=lambda t: t[:-1].clone()),
    "long_table": dict(tab=lambda t: t.long()),
}


@pytest.mark.parametrize("which", list(GUARDS))
@pytest.mark.parametrize("op", ["rope", "attn"])
def test_host_guard_refuses_before_launch(ops, op, which):
    from mdi_llm_amd.ops.engine import prefill_varlen_table

    hs, qpk = 64, 2
    b = _batch(ops, qpk, hs, op == "attn", hs)
    (qbuf, qkv), dev = _padded(b["raw"]), _dev(b["pools"])
    obuf, out = _padded(torch.full((T_TOTAL, N_KV * qpk * hs), P.SENTINEL))

    def call(a):
        if op == "rope":
            _rope(ops, b, qkv, dev, a["lists"], a["tab"])
        else:
            _attn(ops, b, out, qkv, dev, hs, a["lists"], a["tab"])

    edit = GUARDS[which]
    a = dict(lists=edit.get("lists", (LENS, SLOTS, POS0S)),
             tab=edit["tab"](b["tab"]) if "tab" in edit else b["tab"])
    keep = [t.clone() for t in (qbuf, obuf)] + [
        None if t is None else t.clone() for t in dev]
    with pytest.raises(RuntimeError):
        call(a)
    if a["tab"] is b["tab"]:  # a list edit: the Python builder refuses too
        with pytest.raises(ValueError):
            prefill_varlen_table(*a["lists"], 2, MAX_SEQ, N_SLOTS, DEV)
    torch.cuda.synchronize()
    for t, k in zip([qbuf, obuf] + dev, keep):
        assert t is None or torch.equal(t, k), "written despite the refusal"
    call(dict(lists=(LENS, SLOTS, POS0S), tab=b["tab"]))  # unedited: accepted
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
ENGINE = {"nano-gpu": {}, "nano-neox-gpu": dict(n_embd=320),
          "nano-moe-gpu": {}}
E_LENS, E_SLOTS = (5, 16, 33, 1), (2, 0, 3, 1)


def _d(x, truth):
    """mean|x - truth| / std(truth), the metric of profiles/attn_mha80.md."""
    return float((x.float() - truth.float()).abs().mean() / truth.std())


def _starter(cfg, m, dtype, n_slots):
    from mdi_llm_amd.models.stages import StarterStage

    st = StarterStage(cfg, cfg.n_layer).to(device=DEV, dtype=dtype)
    st.load_state_dict(m.state_dict())
    st.eval()
    st.set_kv_cache(n_slots)
    return st


def _model(name, over, seed):
    from mdi_llm_amd import GPT, ModelConfig

    cfg = ModelConfig.from_name(name, **over)
    torch.manual_seed(seed)
    m = GPT(cfg)
    m.apply_init()
    return cfg, m.to(device=DEV, dtype=BF)


@torch.inference_mode()
@pytest.mark.parametrize("name", list(ENGINE))
def test_engine_prefill_prompts(name):
    """The packed pass may sit at most twice as far from the fp32 torch stage
    as the per-prompt engine path on the same prompts (the d80 <= 2 * d64
    rule of test_attn_mha80_gpu.py), on the hidden rows and on the K/V rows
    written."""
    from mdi_llm_amd.ops.engine import DecodeEngine
    from mdi_llm_amd.parallel.runner import HipRunner

    cfg, m = _model(name, ENGINE[name], seed=7080)
    st_b, st_s = _starter(cfg, m, BF, 4), _starter(cfg, m, BF, 4)
    truth = _starter(cfg, m, torch.float32, 4)
    runner = HipRunner(st_b, 4, n_chunks=8, use_graphs=False)
    single = DecodeEngine(st_s, st_s.kv_pool, n_chunks=8, use_graphs=False)
    assert runner.engine.supports_hip_prefill
    prompts = [torch.randint(0, 511, (T,), device=DEV) for T in E_LENS]
    xs_b = runner.prefill_heads(prompts, list(E_SLOTS))
    assert [tuple(x.shape) for x in xs_b] == [(T, cfg.n_embd) for T in E_LENS]
    xs_s = [single.prefill_prompt(p, s, 0) for p, s in zip(prompts, E_SLOTS)]
    xs_t = [truth.forward_head(p.view(1, -1), slot=s, input_pos=0)[0]
            for p, s in zip(prompts, E_SLOTS)]

    def rows(st, nm):
        return torch.cat([getattr(st.kv_pool, nm)[s, :, :, :T].flatten()
                          for T, s in zip(E_LENS, E_SLOTS)])

    for what, b, s, t in (
            ("hidden", torch.cat(xs_b), torch.cat(xs_s), torch.cat(xs_t)),
            ("k", rows(st_b, "k"), rows(st_s, "k"), rows(truth, "k")),
            ("v", rows(st_b, "v"), rows(st_s, "v"), rows(truth, "v"))):
        d_batch, d_single = _d(b, t), _d(s, t)
        print(f"VARLEN_D {name} {what}: batch {d_batch:.5f} single "
              f"{d_single:.5f}")
        assert d_batch <= 2 * d_single, what
    assert runner.engine.pos_table.tolist() == [
        E_LENS[E_SLOTS.index(s)] for s in range(4)]
    tok = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    for s in E_SLOTS:  # one decode step off each batch-filled slot
        logits = runner.tail(runner.decode_head(tok, s))
        assert bool(torch.isfinite(logits.float()).all()), s


def test_generate_prefills_in_one_batch(monkeypatch):
    from mdi_llm_amd.parallel.runner import make_runner
    from mdi_llm_amd.parallel.runtime import PipelineRuntime, SamplingParams

    monkeypatch.setenv("MDI_PREFILL_BATCH", "1")
    cfg, m = _model("nano-gpu", {}, seed=7081)
    runner = make_runner(_starter(cfg, m, BF, 4), 4, torch.device(DEV))
    assert runner.backend == "hip"
    rt = PipelineRuntime(runner, device=torch.device(DEV))
    batched, inner = [], runner.prefill_heads

    def counting(prompts, slots):
        batched.append(len(prompts))
        return inner(prompts, slots)

    runner.prefill_heads = counting
    prompts = [torch.randint(0, 511, (T,), device=DEV) for T in (8, 3, 17, 5)]
    res = rt.generate(prompts, 6, SamplingParams(temperature=0.0))
    assert batched == [4]
    assert [s.numel() for s in res.sequences] == [p.numel() + 6
                                                  for p in prompts]
