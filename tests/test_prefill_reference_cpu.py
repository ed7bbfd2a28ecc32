"""The prefill bounds have teeth — shown without a GPU.

prefill_attn: over a reduced matrix (n_kv 2, hs 64/128, bf16 and fp8) fp32
emulations of both kernels' arithmetic (v2: 64- or 32-key chunks, online
softmax, P rounded to bf16 before PV; v1: 16-key tiles, fp32 P) pass their
bound, and every applicable mutated reference, rounded to bf16, fails the
wider (v2) bound.  Each mutation models one way a prefill kernel goes
subtly wrong.  rope_prefill_append and mtile_gemm get the same treatment
against their own criteria.

Every (case, mutation) pair is one parametrised test; pairs that cannot
apply (no pos0 to ignore at pos0 = 0, no fp8 scale in a bf16 cache) are not
generated at all, never skipped.  The emulation tests print their worst
err/bound; profiles/prefill_error_margins.md keeps the figures.
"""

import functools

import pytest
import torch

import gemv_reference as G
import prefill_reference as P
from attn_reference import (attn_error_bound, bf16_round, bf16_ulp_distance,
                            rope_rows, rope_tables)
from prefill_reference import (C_V1, C_V2, F64, assign_probes, attend_masked,
                               causal_visible, gather_kv, prefill_error_ok,
                               prefill_error_ratio, split_q)

MATRIX = P.reduced_matrix()


@functools.lru_cache(maxsize=None)
def built(name):
    case = P.make_prefill_case(**MATRIX[name])
    ref = case.reference()
    assert case.probes_ok(ref), (case.probe_weights(ref),
                                 case.leak_margins())
    return case, ref


def _bf(x):
    return x.to(torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------
# fp32 emulations of the two kernels
def emulate(case, kch, p_bf16):
    """Online softmax over kch-key chunks in fp32.  p_bf16: P is rounded to
    bf16 before PV while l sums the unrounded P (v2); otherwise P stays
    fp32 (v1).  A chunk that is wholly masked for a row leaves its state
    unchanged (exp(-1e30 - m) is 0), as a wave that skips the chunk does."""
    q, K, V = (t.to(torch.float32) for t in case.qKV())
    T, S = case.T, case.S
    vis = causal_visible(T, S, case.pos0)[:, None, None, :]
    sc = torch.einsum("tgjd,gsd->tgjs", q, K) * torch.tensor(
        case.scale, dtype=torch.float32)
    sc = torch.where(vis, sc, torch.full_like(sc, -1e30))
    m = torch.full(sc.shape[:-1], -1e30)
    l = torch.zeros_like(m)
    o = torch.zeros(*m.shape, case.hs)
    for a in range(0, S, kch):
        s_c = sc[..., a:a + kch]
        m_new = torch.maximum(m, s_c.amax(-1))
        alpha = torch.exp(m - m_new)
        p = torch.exp(s_c - m_new[..., None])
        l = l * alpha + p.sum(-1)
        pp = p.to(torch.bfloat16).to(torch.float32) if p_bf16 else p
        o = o * alpha[..., None] + torch.einsum("tgjs,gsd->tgjd", pp,
                                                V[:, a:a + kch])
        m = m_new
    out = o * (1.0 / l)[..., None]
    return out.to(torch.bfloat16).reshape(T, case.n_head, case.hs)


EMULATIONS = {"v2-kch64": (64, True, C_V2), "v2-kch32": (32, True, C_V2),
              "v1-tile16": (16, False, C_V1)}


@pytest.mark.parametrize("emu", list(EMULATIONS))
@pytest.mark.parametrize("name", list(MATRIX))
def test_emulation_is_within_its_bound(name, emu):
    case, ref = built(name)
    kch, p_bf16, c = EMULATIONS[emu]
    got = emulate(case, kch, p_bf16)
    ratio = prefill_error_ratio(got, ref.out, ref.A, c)
    decode = float(((got.to(F64) - ref.out).abs()
                    / attn_error_bound(ref.out, ref.A)).max())
    print(f"EMU_RATIO {emu} {name} own {ratio:.3f} decode-bound "
          f"{decode:.3f}")
    assert prefill_error_ok(got, ref.out, ref.A, c), ratio


@pytest.mark.parametrize("name", list(MATRIX))
def test_rounded_reference_passes_both_bounds(name):
    case, ref = built(name)
    got = _bf(ref.out)
    assert prefill_error_ok(got, ref.out, ref.A, C_V1)
    assert prefill_error_ok(got, ref.out, ref.A, C_V2)


# ---------------------------------------------------------------------------
# prefill_attn mutations
def _mutations(kw):
    qpk, T, pos0, kv8 = kw["qpk"], kw["T"], kw["pos0"], kw["kv8"]
    S = pos0 + T
    keys, leak = assign_probes(pos0, T)
    pk = sorted({k for ks in keys.values() for k in ks})
    muts = [f"drop_key_{k}" for k in pk]
    muts += [f"drop_tile16_{a}" for a in sorted({k // 16 * 16 for k in pk})]
    muts += [f"drop_chunk64_{a}" for a in sorted({k // 64 * 64 for k in pk})]
    muts.append("mask_lt")
    if leak:
        muts += ["mask_le_plus1", "full_one_chunk_early"]
    if pos0 > 0:
        muts.append("mask_ignores_pos0")
    if T >= 2:
        muts.append("q_row_xor1")
    if qpk >= 2:
        muts.append("head_xor1")
    muts += ["kv_head_next", "other_slot", "other_layer", "stale_v_row",
             "garbage_row_S"]
    if kv8:
        muts += ["neighbour_kscale", "neighbour_vscale", "v_unscaled"]
    if kw.get("mode") == "ascending":
        muts.append("chunk_without_alpha")
    return muts


PAIRS = [(n, m) for n, kw in MATRIX.items() for m in _mutations(kw)]


def _online_fp64(q, K, V, scale, vis, kch, skip_alpha_at):
    """fp64 online softmax; the merge of chunk `skip_alpha_at` forgets to
    rescale the running output (l is still rescaled)."""
    sc = P.scores(q, K, scale).masked_fill(~vis[:, None, None, :],
                                           -float("inf"))
    S = sc.shape[-1]
    m = torch.full(sc.shape[:-1], -1e30, dtype=F64)
    l = torch.zeros_like(m)
    o = torch.zeros(*m.shape, V.shape[-1], dtype=F64)
    for ci, a in enumerate(range(0, S, kch)):
        s_c = sc[..., a:a + kch]
        m_new = torch.maximum(m, s_c.amax(-1))
        alpha = torch.exp(m - m_new)
        p = torch.exp(s_c - m_new[..., None])
        l = l * alpha + p.sum(-1)
        if ci != skip_alpha_at:
            o = o * alpha[..., None]
        o = o + torch.einsum("tgjs,gsd->tgjd", p, V[:, a:a + kch])
        m = m_new
    return (o / l[..., None]).reshape(sc.shape[0], -1, V.shape[-1])


def mutate(name, mut):
    """The output a kernel with this mistake would produce (fp64)."""
    case, ref = built(name)
    T, S, pos0, qpk = case.T, case.S, case.pos0, case.qpk
    q, K, V = case.qKV()
    vis = causal_visible(T, S, pos0)
    keys = torch.arange(S)[None, :]
    q_abs = (pos0 + torch.arange(T))[:, None]

    def att(q=q, K=K, V=V, vis=vis):
        return attend_masked(q, K, V, case.scale, vis)[0]

    if mut.startswith("drop_key_"):
        v = vis.clone()
        v[:, int(mut[len("drop_key_"):])] = False
        return att(vis=v)
    if mut.startswith("drop_tile16_") or mut.startswith("drop_chunk64_"):
        width = 16 if "tile16" in mut else 64
        a = int(mut.rsplit("_", 1)[1])
        v = vis.clone()
        v[:, a:a + width] = False
        return att(vis=v)
    if mut == "mask_lt":
        return att(vis=keys < q_abs)
    if mut == "mask_le_plus1":
        return att(vis=keys <= q_abs + 1)
    if mut == "mask_ignores_pos0":
        return att(vis=keys <= q_abs - pos0)
    if mut == "full_one_chunk_early":
        # the first chunk that is not interior to a q tile goes unmasked
        v = vis.clone()
        for t in range(T):
            c0 = (pos0 + t // 16 * 16 + 1) // 64
            v[t, c0 * 64:(c0 + 1) * 64] = True
        return att(vis=v)
    if mut == "q_row_xor1":
        idx = [t ^ 1 if (t ^ 1) < T else t for t in range(T)]
        return att(q=q[idx])
    if mut == "head_xor1":
        idx = [j ^ 1 if (j ^ 1) < qpk else j for j in range(qpk)]
        return att(q=q[:, :, idx])
    if mut == "kv_head_next":
        return att(K=K.roll(-1, 0), V=V.roll(-1, 0))
    if mut == "other_slot":
        return case.reference(slot=(case.slot + 1) % P.N_SLOTS).out
    if mut == "other_layer":
        return case.reference(layer=(case.layer + 1) % P.N_LAYERS).out
    if mut == "stale_v_row":
        return att(V=torch.cat([V[:, :1], V[:, :-1]], dim=1))
    if mut == "garbage_row_S":
        K1, V1 = gather_kv(case.kpool, case.vpool, case.kscale, case.vscale,
                           case.slot, case.layer, S + 1)
        v = torch.cat([vis, torch.zeros(T, 1, dtype=torch.bool)], dim=1)
        v[T - 1, S] = True
        return att(K=K1, V=V1, vis=v)
    if mut == "neighbour_kscale":
        return case.reference(kscale=case.kscale.roll(1, -1)).out
    if mut == "neighbour_vscale":
        return case.reference(vscale=case.vscale.roll(1, -1)).out
    if mut == "v_unscaled":
        return case.reference(vscale=torch.ones_like(case.vscale)).out
    if mut == "chunk_without_alpha":
        return _online_fp64(q, K, V, case.scale, vis, 64, (S - 1) // 64)
    raise KeyError(mut)


@pytest.mark.parametrize("name,mut", PAIRS)
def test_mutation_is_detected(name, mut):
    case, ref = built(name)
    bad = mutate(name, mut)
    assert bad.shape == ref.out.shape
    assert not prefill_error_ok(_bf(bad), ref.out, ref.A, C_V2), (
        f"{mut} passes the bound on {name}: err/bound "
        f"{prefill_error_ratio(_bf(bad), ref.out, ref.A, C_V2):.3f}")


def test_online_model_without_mutation_is_exact():
    """The fp64 online model used for chunk_without_alpha is the reference
    when no rescale is skipped."""
    name = next(n for n in MATRIX if "ascending" in n)
    case, ref = built(name)
    q, K, V = case.qKV()
    out = _online_fp64(q, K, V, case.scale,
                       causal_visible(case.T, case.S, case.pos0), 64, -1)
    assert torch.allclose(out, ref.out, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------
# rope_prefill_append
ROPE = {n: kw for n, kw in P.rope_matrix().items() if not kw["kv8"]}


@functools.lru_cache(maxsize=None)
def rope_built(name):
    case = P.make_rope_case(**ROPE[name])
    ref = P.rope_append_reference(case.qkv, case.cos, case.sin, case.pos0,
                                  case.n_kv, case.hs)
    return case, ref


def rope_emulate(case, fused):
    """The kernel's fp32 arithmetic: x1*c - x2*s and x2*c + x1*s, with or
    without the compiler contracting each into one fma."""
    T, ne, hs = case.T, case.rope_ne, case.hs
    x = case.qkv.reshape(T, case.n_kv, -1, hs).to(torch.float32)
    out = x.clone()
    if ne == 0:
        return out.to(torch.bfloat16)
    half = ne // 2
    c = case.cos[case.pos0:case.pos0 + T][:, None, None, :]
    s = case.sin[case.pos0:case.pos0 + T][:, None, None, :]
    x1, x2 = x[:, :, :-1, :half], x[:, :, :-1, half:ne]
    if fused:
        lo = (x1.double() * c[..., :half].double()
              - (x2 * s[..., :half]).double()).float()
        hi = (x2.double() * c[..., half:].double()
              + (x1 * s[..., half:]).double()).float()
    else:
        lo = x1 * c[..., :half] - x2 * s[..., :half]
        hi = x2 * c[..., half:] + x1 * s[..., half:]
    out[:, :, :-1, :half] = lo
    out[:, :, :-1, half:ne] = hi
    return out.to(torch.bfloat16)


def rope_ok(got, ref):
    """q/k within one bf16 ulp of the rounded reference; v bit-equal."""
    want = _bf(ref)
    ok_qk = bool((bf16_ulp_distance(got[:, :, :-1], want[:, :, :-1])
                  <= 1).all())
    return ok_qk and torch.equal(got[:, :, -1], want[:, :, -1])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(ROPE))
def test_rope_emulation_is_within_one_ulp(name, fused):
    case, ref = rope_built(name)
    assert rope_ok(rope_emulate(case, fused), ref)


def _rope_mutations(kw):
    ne, hs, T, pos0 = kw["rope_ne"], kw["hs"], kw["T"], kw["pos0"]
    if ne == 0:
        return []
    muts = []
    if pos0 + T < P.ROPE_MAX_SEQ:   # the table has a row to be wrong with
        muts.append("pos_plus1")
    if pos0 > 0:
        muts += ["pos_minus1", "pos0_ignored"]
    if pos0 + T - 1 >= 1:   # rope at position 0 is the identity
        muts += ["sin_sign", "adjacent_pairs", "rope_on_v"]
        if ne < hs:
            muts.append("rope_past_ne")
    return muts


ROPE_PAIRS = [(n, m) for n, kw in ROPE.items() for m in _rope_mutations(kw)]


def rope_mutate(name, mut):
    case, ref = rope_built(name)
    T, ne, hs, pos0 = case.T, case.rope_ne, case.hs, case.pos0
    x = case.qkv.reshape(T, case.n_kv, -1, hs).to(F64)
    out = x.clone()
    cos, sin = case.cos, case.sin
    for t in range(T):
        pos = pos0 + t
        if mut == "pos_plus1":
            pos += 1
        elif mut == "pos_minus1":
            pos -= 1
        elif mut == "pos0_ignored":
            pos = t
        c, s = cos[pos], sin[pos]
        rows = slice(None) if mut == "rope_on_v" else slice(None, -1)
        if mut == "sin_sign":
            out[t, :, rows] = rope_rows(x[t, :, rows], c, s, inverse=True)
        elif mut == "adjacent_pairs":
            # interleaved pairs (d, d+1) with the angle of pair d/2
            xr = x[t, :, rows, :ne]
            h = ne // 2
            ev, od = xr[..., 0::2], xr[..., 1::2]
            o = xr.clone()
            o[..., 0::2] = ev * c[:h].double() - od * s[:h].double()
            o[..., 1::2] = od * c[:h].double() + ev * s[:h].double()
            out[t, :, rows, :ne] = o
        elif mut == "rope_past_ne":
            cw, sw = rope_tables(case.max_seq, hs)
            out[t, :, rows] = rope_rows(x[t, :, rows], cw[pos], sw[pos])
        else:
            out[t, :, rows] = rope_rows(x[t, :, rows], c, s)
    return out


@pytest.mark.parametrize("name,mut", ROPE_PAIRS)
def test_rope_mutation_is_detected(name, mut):
    case, ref = rope_built(name)
    assert not rope_ok(_bf(rope_mutate(name, mut)), ref), (name, mut)


# ---------------------------------------------------------------------------
# mtile_gemm
MT = {c.id: c for c in P.mtile_reduced()}
MT_MUTS = ["drop_quarter_chunk", "swap_batch_rows", "swap_x_groups",
           "missing_bias", "res_from_row_xor1", "last_chunk_dropped"]


@functools.lru_cache(maxsize=None)
def mt_built(cid):
    inp = P.make_mtile_inputs(MT[cid])
    return inp, P.mtile_reference(inp)


def _mt(X, W, bias, res):
    y = X @ W.t()
    if bias is not None:
        y = y + bias[None]
    if res is not None:
        y = y + res
    return y


def mt_mutate(cid, mut):
    case = MT[cid]
    inp, _ = mt_built(cid)
    X, W = inp.X.to(F64), inp.W.to(F64)
    bias, res = inp.bias.to(F64), inp.res.to(F64)
    KC, B = case.KC, case.B
    flip = [b ^ 1 for b in range(B)]
    if mut == "drop_quarter_chunk":   # wave 2's q0 slice of chunk 1
        Xm = X.clone()
        a = KC + 2 * (KC // 4)
        Xm[:, a:a + KC // 4] = 0
        return _mt(Xm, W, bias, res)
    if mut == "swap_batch_rows":
        return _mt(X, W, bias, res)[flip]
    if mut == "swap_x_groups":        # one 8-element unit of chunk 1
        Xm = X.clone()
        a = KC + 40
        Xm[:, a:a + 8] = X[flip, a:a + 8]
        return _mt(Xm, W, bias, res)
    if mut == "missing_bias":
        return _mt(X, W, None, res)
    if mut == "res_from_row_xor1":
        return _mt(X, W, bias, res[flip])
    if mut == "last_chunk_dropped":
        Xm = X.clone()
        Xm[:, -KC:] = 0
        return _mt(Xm, W, bias, res)
    raise KeyError(mut)


@pytest.mark.parametrize("cid", list(MT))
def test_mtile_rounded_reference_passes(cid):
    inp, r = mt_built(cid)
    ok, worst = P.mtile_error_ok(_bf(r.ref), r, MT[cid].K)
    assert ok, worst


@pytest.mark.parametrize("mut", MT_MUTS)
@pytest.mark.parametrize("cid", list(MT))
def test_mtile_mutation_is_detected(cid, mut):
    inp, r = mt_built(cid)
    ok, worst = P.mtile_error_ok(_bf(mt_mutate(cid, mut)), r, MT[cid].K)
    assert not ok, f"{mut} passes the bound on {cid}: {worst:.3f}"


def test_matrices_are_what_the_gpu_files_expect():
    assert len(P.prefill_matrix()) == 2 * (7 + 7 + 14 + 4 + 3 + 2 + 3)
    assert set(P.V1_NAMES) <= set(P.prefill_matrix())
    assert len(P.kch32_matrix()) == 24
    assert len(P.rope_matrix()) == 5 * 2 * 3 * 2
    assert len(P.mtile_matrix()) == 4 * 3 * 3 * 4
