"""The attention error metric has teeth — shown without a GPU.

For a small matrix of the probe and mode cases of the GPU matrix (n_kv=2,
hs 64 and 128, S <= 300) the true fp64 reference, rounded to bf16, passes
attn_error_ok, and every applicable mutated reference, rounded to bf16,
fails it.  Each mutation models one way a decode-attention kernel goes
subtly wrong: a dropped key or tile, a rope taken from the wrong position,
a stale V row, a wrong slot/layer/head stride, a combine that skips a
rescale or ignores chunks past its register budget, a neighbour's fp8 scale.

Every (case, mutation) pair is one parametrised test, so the test report
lists each pair as detected; pairs that cannot apply to a case (no rope to
get wrong, no chunk >= 64 at S=17) are not generated at all, never skipped.
"""

import functools

import pytest
import torch

from attn_reference import (attend, attn_error_ok, gather_inputs,
                            bf16_round, keys_per_chunk, make_case,
                            pick_probes, rope_rows, rope_tables, split_qkv)

QPK, N_KV = 4, 2


def _matrix():
    cases = {}
    edge = [0, 15, 16, 63, 64]

    def add(name, S, cand, max_seq=128, **kw):
        pos = S - 1
        probes = pick_probes(S, list(cand) + [pos - 1, pos])
        for hs in (64, 128):
            for kv8 in (False, True):
                key = f"{name}-h{hs}-{'fp8' if kv8 else 'bf16'}"
                cases[key] = dict(qpk=QPK, n_kv=N_KV, hs=hs, pos=pos,
                                  max_seq=max_seq, probes=probes, kv8=kv8,
                                  seed=len(cases) + 1, **kw)

    for S in (2, 17, 65, 128):          # block-local S edges
        add(f"s_edge-S{S}", S, edge)
    for n_chunks, S in ((4, 65), (16, 257), (16, 300)):   # split chunk edges
        kpc = keys_per_chunk(S, n_chunks)
        add(f"chunk_edge-c{n_chunks}-S{S}", S,
            [0, kpc - 1, kpc, ((S - 1) // kpc) * kpc], max_seq=512)
    for mode in ("ascending", "descending", "outlier"):
        add(f"mode-{mode}", 300, [0, 150], max_seq=512, mode=mode)
    add("rope16-S83", 83, [0, 15, 16, 64], rope_ne=16)
    add("rope0-S83", 83, [0, 15, 16, 64], rope_ne=0)
    return cases


MATRIX = _matrix()


@functools.lru_cache(maxsize=None)
def built(name):
    case = make_case(**MATRIX[name])
    ref = case.reference()
    inp = gather_inputs(case.qkv[0], case.kpool, case.vpool, case.cos,
                        case.sin, case.pos[0], case.slot[0], case.layer,
                        case.kscale, case.vscale)
    return case, ref, inp


# ---------------------------------------------------------------------------
# split-S model: per-chunk (m, l, o) partials merged as the combine does
def merge_chunks(inp, scale, kpc, stale=None, ignore_from=None):
    """stale='auto': the chunk furthest below the global max is merged with
    weight 1, as if its m were already global (a skipped rescale).
    ignore_from=c: chunks >= c never reach the merge."""
    sc = torch.einsum("gjd,gsd->gjs", inp.q, inp.K) * scale
    S = sc.shape[-1]
    m, l, o = [], [], []
    for a in range(0, S, kpc):
        s_c = sc[..., a:a + kpc]
        m_c = s_c.amax(-1)
        e = torch.exp(s_c - m_c[..., None])
        m.append(m_c)
        l.append(e.sum(-1))
        o.append(torch.einsum("gjs,gsd->gjd", e, inp.V[:, a:a + kpc]))
    m, l, o = torch.stack(m), torch.stack(l), torch.stack(o)
    if ignore_from is not None:
        m, l, o = m[:ignore_from], l[:ignore_from], o[:ignore_from]
    M = m.amax(0)
    w = torch.exp(m - M)
    if stale == "auto":
        w[int((M - m).sum((1, 2)).argmax())] = 1.0
    out = (w[..., None] * o).sum(0) / (w * l).sum(0)[..., None]
    return out.reshape(-1, out.shape[-1])


def _attend(case, inp):
    return attend(inp.q, inp.K, inp.V, case.scale)[0]


def _regather(case, **over):
    a = dict(qkv=case.qkv[0], kpool=case.kpool, vpool=case.vpool,
             cos=case.cos, sin=case.sin, pos=case.pos[0], slot=case.slot[0],
             layer=case.layer, kscale=case.kscale, vscale=case.vscale)
    a.update(over)
    return gather_inputs(**a)


def _replace(inp, **kw):
    import dataclasses

    return dataclasses.replace(inp, **kw)


def mutate(name, mut):
    """The output a kernel with this mistake would produce (fp64)."""
    case, ref, inp = built(name)
    pos, hs = case.pos[0], case.hs
    q_raw, k_raw, _ = split_qkv(case.qkv[0], case.n_kv, hs)
    if mut.startswith("drop_key_"):
        s = int(mut[len("drop_key_"):])
        keep = [i for i in range(pos + 1) if i != s]
        return _attend(case, _replace(inp, K=inp.K[:, keep],
                                      V=inp.V[:, keep]))
    if mut == "q_rope_from_pos-1":
        q = bf16_round(rope_rows(q_raw, case.cos[pos - 1],
                                 case.sin[pos - 1]))
        return _attend(case, _replace(inp, q=q))
    if mut == "current_k_unroped":
        K = inp.K.clone()
        K[:, -1] = k_raw
        return _attend(case, _replace(inp, K=K))
    if mut == "rope_on_all_dims":
        cos, sin = rope_tables(case.max_seq, hs)
        return _attend(case, _regather(case, cos=cos, sin=sin))
    if mut == "current_v_from_zeroed_pool_row":
        V = inp.V.clone()
        V[:, -1] = 0.0
        return _attend(case, _replace(inp, V=V))
    if mut == "other_slot":
        return _attend(case, _regather(case, slot=(case.slot[0] + 1) % 3))
    if mut == "other_layer":
        return _attend(case, _regather(case, layer=1 - case.layer))
    if mut == "head_to_group_shifted":
        return _attend(case, _replace(inp, K=inp.K.roll(1, 0),
                                      V=inp.V.roll(1, 0)))
    if mut == "combine_skips_a_rescale":
        return merge_chunks(inp, case.scale, 16, stale="auto")
    if mut.startswith("combine_ignores_chunks_ge_"):
        # one key per chunk, so that S <= 300 reaches chunk indices >= 256
        return merge_chunks(inp, case.scale, 1,
                            ignore_from=int(mut.rsplit("_", 1)[1]))
    if mut == "fp8_neighbour_kscale":
        return _attend(case, _regather(case, kscale=case.kscale.roll(-1, -1)))
    raise KeyError(mut)


def mutations_for(name):
    kw = MATRIX[name]
    S, hs = kw["pos"] + 1, kw["hs"]
    ne = kw.get("rope_ne", hs)
    muts = [f"drop_key_{s}" for s in kw["probes"]]
    if ne > 0:
        muts += ["q_rope_from_pos-1", "current_k_unroped"]
    if ne < hs:
        muts.append("rope_on_all_dims")
    muts += ["current_v_from_zeroed_pool_row", "other_slot", "other_layer",
             "head_to_group_shifted"]
    if S > 16:
        muts.append("combine_skips_a_rescale")
    muts += [f"combine_ignores_chunks_ge_{c}" for c in (64, 192, 256)
             if S > c]
    if kw["kv8"]:
        muts.append("fp8_neighbour_kscale")
    return muts


PAIRS = [(n, m) for n in MATRIX for m in mutations_for(n)]


@pytest.mark.parametrize("name", list(MATRIX))
def test_reference_rounded_to_bf16_passes(name):
    case, ref, _ = built(name)
    assert case.probes_ok(ref), case.probe_weights(ref)
    assert attn_error_ok(ref.out.to(torch.bfloat16), ref.out, ref.A)


@pytest.mark.parametrize("name", list(MATRIX))
def test_chunk_merge_model_is_exact(name):
    """The split/merge model used by the combine mutations reproduces the
    reference when nothing is mutated."""
    case, ref, inp = built(name)
    for kpc in (1, 16):
        got = merge_chunks(inp, case.scale, kpc)
        assert torch.allclose(got, ref.out, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name,mut", PAIRS,
                         ids=[f"{n}::{m}" for n, m in PAIRS])
def test_mutation_is_detected(name, mut):
    case, ref, _ = built(name)
    bad = mutate(name, mut).to(torch.bfloat16)
    assert not attn_error_ok(bad, ref.out, ref.A), \
        f"{mut} would pass the GPU matrix on {name}"


def test_fp32_reference_stays_inside_the_condition_term():
    """The same algorithm in fp32 (same rounding points) differs from fp64
    by far less than 2^-9 A, so the bound needs no widening."""
    worst = 0.0
    for name in MATRIX:
        case, ref, _ = built(name)
        r32 = case.reference(dtype=torch.float32)
        worst = max(worst, float(((r32.out.double() - ref.out).abs()
                                  / (2.0 ** -9 * ref.A)).max()))
    assert worst < 0.25, worst


def test_gpu_matrix_cases_meet_the_probe_precondition():
    """Seeds and probe targets of every GPU case are checked here, on the
    CPU, so a GPU failure is never a broken precondition."""
    import test_attn_decode_matrix_gpu as gpu_matrix
    import test_attn_proj_gpu as proj

    specs = [(s.name, s.kw) for s in gpu_matrix.SPECS]
    specs += [(str(k), k) for k in proj.case_kwargs()]
    for name, kw in specs:
        for kv8 in ((False, True) if "kv8" not in kw else (kw["kv8"],)):
            case = make_case(**{**kw, "kv8": kv8})
            ref = case.reference()
            assert case.probes_ok(ref), (name, kv8, case.probe_weights(ref))
            assert attn_error_ok(ref.out.to(torch.bfloat16), ref.out, ref.A)


def test_clamp_attn_chunks():
    from mdi_llm_amd.ops.engine import clamp_attn_chunks

    assert [clamp_attn_chunks(n) for n in
            (-3, 0, 1, 4, 6, 7, 8, 16, 255, 256, 257, 260, 1024)] == \
        [4, 4, 4, 4, 4, 4, 8, 16, 252, 256, 256, 256, 256]
    for n in range(0, 600):
        c = clamp_attn_chunks(n)
        assert 4 <= c <= 256 and c % 4 == 0
