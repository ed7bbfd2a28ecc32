"""The GEMV error bound has teeth — shown without a GPU.

For every case of the GPU matrix (gemv_reference.matrix_cases, plus the
MDI_GEMV_PRE cases) an honest emulation passes the bound: torch fp32
arithmetic on the reference's building blocks with the same rounding points,
the result rounded to bf16 into a sentinel-filled buffer.  Every applicable
mutation of that emulation fails it.  Each mutation models one way a GEMV
kernel goes subtly wrong; `MUTATIONS` maps a name to the predicate that says
where it applies, and a pair that cannot apply (no norm to get wrong, one
int4 group only) is not generated.

Several mutations are limited by the resolution of the bound itself; their
predicates state that limit a priori (see resolution()), never from what
the emulation returns.
"""

import functools

import pytest
import torch

import gemv_reference as R
from gemv_reference import (EPS, INT4_GROUP, PRE_CASES, SENTINEL, bf16_round,
                            bf16_trunc, check_out_buffer, fragile_cap,
                            linear_tail, make_inputs, matrix_cases,
                            new_out_buffer, reference, stage_x, wraps)

F32 = torch.float32
CASES = {c.id: c for c in matrix_cases()}
CASES.update({c.id + "-preon": c for c in PRE_CASES})


def is_pre(name):
    return name.endswith("-preon")


@functools.lru_cache(maxsize=None)
def built(name):
    case = CASES[name]
    inp = make_inputs(case)
    return case, inp, reference(case, inp, pre=is_pre(name))


# ---------------------------------------------------------------------------
# fp32 model of the kernels, with one optional fault
def emulate(case, inp, pre=False, mut=None):
    """bf16 output buffer [M + pad] of an fp32 model of the kernel."""
    M, K = case.M, case.K
    knobs = {}
    if mut == "stats_short":
        knobs["stat_count"] = K - 8
    if mut == "eps_omitted":
        knobs["use_eps"] = False
    if mut == "var_uncentered":
        knobs["center_var"] = False
    if mut == "norm_bias_skipped":
        knobs["use_nb"] = False
    st = stage_x(inp.x, inp.nw, inp.nb, case.norm, EPS,
                 case.dispatch(pre).rounded, F32, **knobs)

    def dot(wt, e):
        wt = wt.expert(e)
        wd = wt.dense(F32, swap_pairs=mut == "nibble_swap",
                      use_zero=mut != "zero_dropped")
        xs = st.xs
        if mut == "chunk_dropped":
            xs = xs.clone()
            xs[-8:] = 0
        acc = wd @ xs
        if mut == "element_dropped":  # the row's largest term
            terms = wd * xs
            k = terms.abs().argmax(1, keepdim=True)
            acc = acc - terms.gather(1, k)[:, 0]
        if mut == "group_sum_shifted":
            # the kernel's (z - 128 s) * gsum[g] term fed gsum[g+1]
            xp = torch.zeros(wt.q.size(1) * 2, dtype=F32)
            xp[:K] = xs
            gs = xp.view(-1, INT4_GROUP).sum(1)
            s = wt.qp[..., 0].to(F32)
            z = wt.qp[..., 1].to(F32)
            acc = acc + ((z - 128.0 * s) * (torch.roll(gs, -1) - gs)[None]
                         ).sum(1)
        return acc, wt.rowscale(F32, 1 if mut == "row_scale_shifted" else 0)

    experts = [case.eidx if case.n_expert else None]
    if case.chain:
        experts.append(case.chain)
    if mut == "eidx_ignored":
        experts = [0] * len(experts)
    if case.op == "gemv":
        res = inp.res
        for step, e in enumerate(experts):
            acc, rs = dot(inp.wt, e)
            val = linear_tail(
                acc, st.post, rs,
                None if mut == "bias_skipped" else inp.bias, res,
                case.epilogue, F32,
                add_res=(case.epilogue != 1) if mut == "res_flipped"
                else None)
            if step + 1 < len(experts):
                # the next call reads its residual from the bf16 output;
                # chain_res_stale: from the first call's residual instead
                res = inp.res if mut == "chain_res_stale" else bf16_round(val)
                if mut == "chain_overwrites":
                    res = torch.zeros_like(val)
    else:
        acc, rs = dot(inp.wt, experts[0])
        uacc, urs = dot(inp.wu, experts[0])
        g = linear_tail(acc, st.post, rs, None, None, 0, F32)
        u = linear_tail(uacc, st.post, urs, None, None, 0, F32)
        val = R.activation(g, 2 if case.gelu_gate else 3) * u
        if case.escale is not None and mut != "escale_ignored":
            val = val * case.escale
    if mut == "scale_2pct":
        val = val * 1.02
    val = bf16_trunc(val) if mut == "truncated" else bf16_round(val)

    buf = new_out_buffer(M)
    buf[:M] = val.to(torch.bfloat16)
    blk = 4 * case.rows_eff
    if mut == "tail_rows_stale":
        buf[M - M % blk:M] = SENTINEL
    if mut == "row_past_end":
        buf[M] = buf[M - 1]
    if mut == "wrap_rows_stale":
        buf[R.WRAP_ROWS * case.rows_eff:M] = SENTINEL
    return buf


def _groups(c):
    return -(-c.K // INT4_GROUP)


def resolution(c):
    """A-priori width of the bound relative to |ref| for the generator's
    rows: 2^-8 plus the accumulation term at the condition A/|ref| the
    generator aims for (2.5 for a row with its +-0.5 sigma aligned part;
    int4 carries 128 s / mean|w| ~ 100 on top; a SwiGLU gate, whose aligned
    part is O(1), sqrt(K)/3)."""
    q = 100.0 if c.fmt == "int4" else 1.0
    cond = 2.5 * q
    if c.op == "swiglu":
        cond += q * c.K ** 0.5 / 3
    return 2.0 ** -8 + (c.K + 16) * 2.0 ** -24 * cond


def eps_shift(c, i):
    """Relative change of the norm scale when eps is left out."""
    if not c.norm:
        return 0.0
    xf = i.x.double()
    v = float((xf * xf).mean())
    if c.norm == 2:
        v -= float(xf.mean()) ** 2
    return 1.0 - (v / (v + EPS)) ** 0.5


def var_shift(c, i):
    """Relative change of the LayerNorm scale without the -mean^2."""
    xf = i.x.double()
    ms = float((xf * xf).mean())
    return 1.0 - ((ms - float(xf.mean()) ** 2 + EPS) / (ms + EPS)) ** 0.5


def clear(c, effect):
    """A numeric mutation applies where its nominal relative effect stands
    clear of resolution() by 2x, in a case of three rows or more: a single
    row may cancel against its own bias and residual, or sit at a dead
    point of its activation."""
    return c.M >= 3 and effect >= 2 * resolution(c)


# Nominal effects.  A dropped chunk is 8 of the K terms of a row whose
# aligned part makes the terms add up, 8/K of the row; one chunk's own
# share varies with its eight x values, so it is counted at 6/K.  The
# row's largest term is about |w|max |xs|max / (0.4 K mean|xs|), 12/K for
# normal tails.  Eight elements missing from the statistics move the scale
# by (sum of their squares)/(2 K ms), 4/K on average; a quiet chunk carries
# well under half of that, so 1.6/K.  eps and the variance's centring move
# the scale by what the inputs say.  A wrong weight, scale, bias or expert
# is an O(1) error, counted at 0.25.  These figures are estimates of the
# inputs, made before looking at what the emulation returns; they decide
# only where a mutation is tried, never whether it counts as rejected.
# Truncation errs by less than the 2^-8 |ref| term in most rows; it shows
# in the lower part of a binade only (about one row in four), so it needs a
# narrow accumulation term and rows enough (24) for one to land there.
# profiles/gemv_error_margins.md lists the (format, K) ranges each of these
# does not reach.
MUTATIONS = {
    # accumulation
    "chunk_dropped": lambda c, i: clear(c, 6.0 / c.K),
    "element_dropped": lambda c, i: clear(c, 12.0 / c.K),
    # norm
    "stats_short": lambda c, i: c.norm != 0 and clear(c, 1.6 / c.K),
    # (LayerNorm: halved, its bias carries part of the dot unscaled)
    "eps_omitted": lambda c, i: c.norm != 0 and clear(
        c, eps_shift(c, i) / c.norm),
    "var_uncentered": lambda c, i: c.norm == 2 and clear(
        c, var_shift(c, i) / 2),
    "norm_bias_skipped": lambda c, i: i.nb is not None and clear(c, 0.25),
    # epilogue
    "bias_skipped": lambda c, i: i.bias is not None and clear(c, 0.25),
    "res_flipped": lambda c, i: i.res is not None and clear(c, 0.25),
    "truncated": lambda c, i: c.M >= 24 and resolution(c) <= 1.25 * 2.0 ** -8,
    "scale_2pct": lambda c, i: clear(c, 0.02),
    # quantised weights
    "row_scale_shifted": lambda c, i: c.fmt == "fp8" and clear(c, 0.25),
    "group_sum_shifted": lambda c, i: (c.fmt == "int4" and _groups(c) >= 2
                                       and clear(c, 0.25)),
    "nibble_swap": lambda c, i: c.fmt == "int4" and clear(c, 0.25),
    "zero_dropped": lambda c, i: c.fmt == "int4" and clear(c, 0.25),
    # MoE
    "eidx_ignored": lambda c, i: c.n_expert > 0 and clear(c, 0.25),
    "escale_ignored": lambda c, i: c.escale is not None and clear(c, 0.25),
    "chain_res_stale": lambda c, i: c.chain > 0,
    "chain_overwrites": lambda c, i: c.chain > 0,
    # rows
    "tail_rows_stale": lambda c, i: c.M % (4 * c.rows_eff) != 0,
    "row_past_end": lambda c, i: True,
    "wrap_rows_stale": lambda c, i: wraps(c.M, c.rows_eff),
}


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_honest_model_passes_and_mutations_fail(name):
    case, inp, ref = built(name)
    pre = is_pre(name)
    ok, worst, msg = check_out_buffer(emulate(case, inp, pre), case.M, ref,
                                      case.K)
    assert ok, f"honest fp32 model outside the bound: {msg}"
    missed = []
    for mut, applies in MUTATIONS.items():
        if not applies(case, inp):
            continue
        ok, _, _ = check_out_buffer(emulate(case, inp, pre, mut), case.M,
                                    ref, case.K)
        if ok:
            missed.append(mut)
    assert not missed, f"mutations the bound accepts: {missed}"


@pytest.mark.parametrize("name", list(CASES))
def test_fragile_cap(name):
    case, inp, ref = built(name)
    assert ref.n_fragile <= fragile_cap(case.K), (ref.n_fragile, inp.seed)
    assert R.count_fragile(case, inp) <= fragile_cap(case.K)


def test_every_mutation_is_exercised():
    """No predicate is vacuous: each mutation applies to several cases, and
    the resolution-limited ones reach every weight format."""
    for mut, applies in MUTATIONS.items():
        hit = [c for n, c in CASES.items() if applies(c, built(n)[1])]
        assert len(hit) >= 4, (mut, len(hit))
    for mut in ("chunk_dropped", "truncated"):
        fmts = {c.fmt for n, c in CASES.items()
                if MUTATIONS[mut](c, built(n)[1])}
        assert fmts == {"bf16", "fp8", "int4"}, (mut, fmts)


def test_inputs_give_mutations_something_to_bite_on():
    for name in CASES:
        case, inp, _ = built(name)
        xf = inp.x.double()
        assert abs(float(xf.mean())) > 0.1 * float(xf.std()) or case.K <= 16
        if case.norm:
            ms = float((xf * xf).mean())
            shift = 1.0 - (ms / (ms + EPS)) ** 0.5
            assert shift > 2.0 ** -7, (name, shift)
            g = inp.nw.double()
            assert (g > 0).any() and (g < 0).any()
        if case.fmt == "fp8" and case.M >= 2:
            s = inp.wt.scale.double()
            r = s[1:] / s[:-1]
            assert bool(((r >= 2) | (r <= 0.5)).all()), name
        full = case.K // INT4_GROUP  # groups with all 128 k live
        if case.fmt == "int4" and full >= 2:
            z = inp.wt.qp[:, :full, 1].double()
            s = inp.wt.qp[:, :full, 0].double()
            assert bool(((z[:, 1:] - z[:, :-1]).abs() > 2 * s[:, 1:]).all())
        if case.n_expert:
            assert case.n_expert >= 3 and case.eidx != 0
            w = inp.wt.w
            assert not torch.equal(w[0], w[1]) and not torch.equal(w[1], w[2])
        if case.escale is not None:
            assert case.escale not in (0.0, 1.0)


def test_int4_packing_matches_the_engine():
    """The reference's nibble order is the project's: what the reference
    packs, the engine's dequantiser reads back, and the other way round."""
    from mdi_llm_amd.ops.engine import (dequantize_int4,
                                        quantize_int4_groupwise)

    torch.manual_seed(3)
    w = (torch.randn(5, 136) + 0.3).to(torch.bfloat16)
    packed, qp = R.int4_quant_groups(w)
    mine = R.Weights("int4", 136, q=packed, qp=qp).dense(F32)
    assert torch.equal(mine, dequantize_int4(packed, qp, 136))
    p2, q2 = quantize_int4_groupwise(w)
    assert torch.equal(p2, packed) and torch.equal(q2, qp)


# ---------------------------------------------------------------------------
# the dispatch-rule mirror against expectations written by hand from
# launch_gemv: (M, K, epilogue, norm, rows, res, eidx, pre) -> result
DISPATCH_TABLE = [
    # NORM 0, K <= 6144, one row: direct, 4 chunks in flight
    ((64, 4096, 0, 0, 1, False, False, False), ("direct", 1, 4, False)),
    ((64, 6144, 1, 0, 0, True, False, False), ("direct", 1, 4, False)),
    # ... past the K switch, or more rows: 2 chunks
    ((64, 6152, 0, 0, 1, False, False, False), ("direct", 1, 2, False)),
    ((64, 512, 0, 0, 2, False, False, False), ("direct", 2, 2, False)),
    ((64, 512, 0, 0, 4, False, False, False), ("direct", 4, 2, False)),
    # RMSNorm: direct, never 4 chunks, x*g not rounded
    ((64, 512, 0, 1, 1, False, False, False), ("direct", 1, 2, False)),
    ((64, 512, 3, 1, 4, False, False, False), ("direct", 4, 2, False)),
    # LayerNorm: staged at every K and rows
    ((64, 512, 0, 2, 1, False, False, False), ("staged", 1, 0, True)),
    ((64, 6152, 2, 2, 2, False, False, False), ("staged", 2, 0, True)),
    # auto rows: 1 up to 8192, 2 above, 4 from 32768
    ((8192, 64, 0, 0, 0, False, False, False), ("direct", 1, 4, False)),
    ((8193, 64, 0, 0, 0, False, False, False), ("direct", 2, 2, False)),
    ((32767, 64, 0, 1, 0, False, False, False), ("direct", 2, 2, False)),
    ((32768, 64, 0, 2, 0, False, False, False), ("staged", 4, 0, True)),
    # an unknown rows value falls to 1
    ((64, 512, 0, 0, 3, False, False, False), ("direct", 1, 4, False)),
    # MDI_GEMV_PRE=1: epilogue 0, RMS, one row, K a multiple of 512 up to
    # 8192, M a multiple of 4, no residual, no expert index
    ((52, 512, 0, 1, 1, False, False, True), ("direct_pre", 1, 8, True)),
    ((52, 4096, 0, 1, 0, False, False, True), ("direct_pre", 1, 8, True)),
    ((52, 4608, 0, 1, 1, False, False, True), ("direct_pre", 1, 16, True)),
    ((52, 8192, 0, 1, 1, False, False, True), ("direct_pre", 1, 16, True)),
    ((52, 8704, 0, 1, 1, False, False, True), ("direct", 1, 2, False)),
    ((52, 520, 0, 1, 1, False, False, True), ("direct", 1, 2, False)),
    ((52, 256, 0, 1, 1, False, False, True), ("direct", 1, 2, False)),
    ((53, 512, 0, 1, 1, False, False, True), ("direct", 1, 2, False)),
    ((52, 512, 1, 1, 1, False, False, True), ("direct", 1, 2, False)),
    ((52, 512, 0, 1, 2, False, False, True), ("direct", 2, 2, False)),
    ((52, 512, 0, 1, 1, True, False, True), ("direct", 1, 2, False)),
    ((52, 512, 0, 1, 1, False, True, True), ("direct", 1, 2, False)),
    ((52, 512, 0, 0, 1, False, False, True), ("direct", 1, 4, False)),
    ((16384, 512, 0, 1, 0, False, False, True), ("direct", 2, 2, False)),
    # the flag off: the same shape stays on the direct kernel
    ((52, 512, 0, 1, 1, False, False, False), ("direct", 1, 2, False)),
]


@pytest.mark.parametrize("args,want", DISPATCH_TABLE)
def test_dispatch_rule(args, want):
    assert tuple(R.gemv_dispatch(*args)) == want


def test_wrap_threshold():
    for rows in (1, 2, 4):
        assert not wraps(16384 * rows, rows)
        assert wraps(16384 * rows + 1, rows)
    for c in CASES.values():
        if c.family == "wrap":
            assert wraps(c.M, c.rows_eff), c.id
        else:
            assert not wraps(c.M, c.rows_eff), c.id


# ---------------------------------------------------------------------------
# the norm / glue references against the same kind of fp32 model
@pytest.mark.parametrize("n", [8, 2040, 2056])
def test_norm_references(n):
    g = torch.Generator().manual_seed(n)
    x = ((torch.randn(3, n, generator=g) + 0.5) * 0.01).to(torch.bfloat16)
    w = torch.randn(n, generator=g).to(torch.bfloat16)
    b = torch.randn(n, generator=g).to(torch.bfloat16)

    r = R.rmsnorm_ref(x, w)
    xf = x.float()
    got = bf16_round(xf * torch.rsqrt((xf * xf).mean(1, keepdim=True) + EPS)
                     * w.float())
    assert R.gemv_error_ok(got, r.ref, r.A, n)[0]
    assert not R.gemv_error_ok(got * 1.02, r.ref, r.A, n)[0]
    no_eps = bf16_round(xf * torch.rsqrt((xf * xf).mean(1, keepdim=True))
                        * w.float())
    assert not R.gemv_error_ok(no_eps, r.ref, r.A, n)[0]
    shifted = torch.roll(got, 1, 0)  # another batch row's result
    assert not R.gemv_error_ok(shifted, r.ref, r.A, n)[0]

    for bias in (None, b):
        r = R.layernorm_ref(x[0], w, bias)
        got = bf16_round(torch.nn.functional.layer_norm(
            x[0].float(), (n,), w.float(),
            None if bias is None else bias.float(), EPS))
        assert R.gemv_error_ok(got, r.ref, r.A, n)[0]
        assert not R.gemv_error_ok(bf16_trunc(got.float() * 1.02), r.ref,
                                   r.A, n)[0]
    r = R.layernorm_ref(x[0], w, b)
    no_b = bf16_round(torch.nn.functional.layer_norm(
        x[0].float(), (n,), w.float(), None, EPS))
    assert not R.gemv_error_ok(no_b, r.ref, r.A, n)[0]


@pytest.mark.parametrize("gelu", [False, True])
def test_swiglu_mul_reference(gelu):
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(2056, generator=g) * 2).to(torch.bfloat16)
    u = torch.randn(2056, generator=g).to(torch.bfloat16)
    r = R.swiglu_mul_ref(a, u, gelu)
    af = a.float()
    act = (torch.nn.functional.gelu(af, approximate="tanh") if gelu
           else torch.nn.functional.silu(af))
    assert R.gemv_error_ok(bf16_round(act * u.float()), r.ref, r.A, 1)[0]
    other = (torch.nn.functional.silu(af) if gelu
             else torch.nn.functional.gelu(af, approximate="tanh"))
    assert not R.gemv_error_ok(bf16_round(other * u.float()), r.ref, r.A,
                               1)[0]
    assert not R.gemv_error_ok(bf16_round(act * u.float() * 1.02), r.ref,
                               r.A, 1)[0]
