"""Shared decode-GEMV reference, error bound, input generator and case matrix.

Plain helper module (like attn_reference.py): the CPU test of the bound, the
GPU matrix and its MDI_GEMV_PRE child process all import it.  It is
device-agnostic, computes in float64 and imports no HIP ops.

Rounding points, as read off decode_kernels.hip.  The references mirror the
kernels at these points and nowhere else; everything between them is exact
(fp64), and the reference output is not rounded.

  * stage_x (gemv_kernel, every fp8 and int4 kernel, every gemv_swiglu*
    kernel) rounds the normalised x to bf16 in LDS.  For RMSNorm the staged
    value is bf16(x*g); the scale rsqrt(mean(x^2)+eps) is uniform over k and
    multiplies the dot product afterwards.  For LayerNorm the staged value
    is bf16((x-mean)*inv*g + b) and the post-scale is 1.
  * gemv_direct_kernel with NORM 1 does NOT round x*g: the product of two
    bf16 values is exact in fp32 and goes into the FMA as it is.
  * gemv_direct_pre_kernel (MDI_GEMV_PRE=1) does round x*g to bf16.
  * fp8 weights are decode(byte) exactly (e4m3fn); wscale[row] multiplies
    the dot product after the reduction, with the norm post-scale.
  * int4 weights are nib*scale + zero with bf16 (scale, zero) per group of
    128 k; rows are padded with zero nibbles to a multiple of 128, and the
    padded positions meet a zero-filled x.
  * bias, residual (epilogue 1 only) and the activation are applied in fp32
    and the result is rounded to bf16 once.

Which form a bf16 GEMV takes is the launcher's decision; gemv_dispatch()
reproduces launch_gemv's rule so that no test hard-codes it.

Error bound (gemv_error_ok):

    |got - ref| <= 2^-8 |ref| + (K+16) 2^-24 A + flip

  * 2^-8 |ref|: the one bf16 rounding of the result (2^-9) plus half an ulp
    of slack for rsqrtf / tanhf / expf.
  * (K+16) 2^-24 A: the order-independent worst case of K fp32 products
    summed in any order, relative to the condition sum A.  For plain GEMVs
    A = |post| * sum_k |w_k| |xs_k|.  Bias and residual are one fp32
    addition each: they add 2^-23 (|bias| + |res|), not multiplied by K,
    to the additive allowance that also holds `flip`.  For int4, A follows the kernel's decomposition
    sum_groups(|s| sum (128+nib)|x| + |z - 128 s| sum |x|): the kernel adds
    128 to every nibble and cancels it through the group sum of x, so its
    error is relative to that, not to sum |w||x|.  Through an activation or
    the SwiGLU product, A is propagated with the Lipschitz constant
    ACT_LIP = 1.13 (max |gelu'|, which also covers silu'):
    1.13 A_g |u| + |act(g)| A_u, times |escale|.
  * flip: a staged x element whose fp64 value lies closer to a bf16
    rounding midpoint than an fp32 error estimate of that element can round
    the other way in the kernel.  The estimate is 16 * 2^-24 *
    (|(x-mean)*inv*g| + |b|) for LayerNorm and 16 * 2^-24 * |x*g| for RMS
    (where x*g is exact in fp32, so only exact ties are flagged).  Each such
    "fragile" element k adds |w_mk| * ulp_bf16(xs_k) * |post| to row m.
    Cap: a case may have at most max(1, K/32) fragile elements; make_inputs
    advances the seed until the reference alone meets it.

Every constant is derived from the number formats; none is fitted to what a
GPU returns.
"""

from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from typing import List, NamedTuple, Optional

import torch

EPS = 1e-5
REL_TERM = 2.0 ** -8       # bf16 rounding of the result + half-ulp slack
ACC_UNIT = 2.0 ** -24      # fp32 unit roundoff
ADD_UNIT = 2.0 ** -23      # one fp32 addition each of bias and residual
ACC_EXTRA = 16             # reductions' tree levels, post-scales, epilogue
ACT_LIP = 1.13             # max |d gelu_tanh / dv| (1.129); silu' <= 1.1
FRAG_ULPS = 16             # fp32 error estimate of a staged element, in ulps
INT4_GROUP = 128
WRAP_ROWS = 16384          # rows one pass of the capped grid covers, / rows
SENTINEL = -(2.0 ** 100)   # pre-fill of out: exact in bf16, never a result
F64 = torch.float64


# ---------------------------------------------------------------------------
# number formats
def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest-even bf16, keep x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """Chop an fp32-representable tensor to bf16 (the truncation mutation)."""
    i = x.to(torch.float32).contiguous().view(torch.int32)
    return (i & -65536).view(torch.float32).to(x.dtype)


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """bf16 spacing in the binade of v (float64 in, float64 out)."""
    _, e = torch.frexp(v.abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(v), e - 8)


def fp8_decode(byte_t: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn bytes -> float32 values (exact)."""
    return byte_t.contiguous().view(torch.float8_e4m3fn).to(torch.float32)


def fp8_quant_rows(w: torch.Tensor):
    """Per-row absmax/448 e4m3fn quantisation: (uint8 bytes, fp32 scales)."""
    wf = w.to(torch.float32)
    s = wf.abs().amax(dim=-1).clamp_min(1e-12) / 448.0
    q = (wf / s[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.contiguous(), s.contiguous()


def int4_pack(nib: torch.Tensor) -> torch.Tensor:
    """uint8 nibbles [M, Kp] -> packed bytes [M, Kp/2] in the kernel's
    order: each 8 consecutive k are the bytes (n0|n2<<4, n4|n6<<4, n1|n3<<4,
    n5|n7<<4)."""
    M, Kp = nib.shape
    n = nib.view(M, Kp // 8, 8)
    return torch.stack(
        [n[..., 0] | (n[..., 2] << 4), n[..., 4] | (n[..., 6] << 4),
         n[..., 1] | (n[..., 3] << 4), n[..., 5] | (n[..., 7] << 4)],
        dim=2).view(M, Kp // 2).contiguous()


def int4_unpack(packed: torch.Tensor, swap_pairs: bool = False):
    """Packed bytes [M, Kp/2] -> uint8 nibbles [M, Kp].  swap_pairs reads
    the even and the odd k of every pair the other way round (mutation)."""
    M = packed.size(0)
    b = packed.view(M, -1, 4)
    lo, hi = b & 0xF, b >> 4
    order = [lo[..., 0], lo[..., 2], hi[..., 0], hi[..., 2],
             lo[..., 1], lo[..., 3], hi[..., 1], hi[..., 3]]
    if swap_pairs:
        order = [order[j ^ 1] for j in range(8)]
    return torch.stack(order, dim=2).view(M, -1)


def int4_quant_groups(w: torch.Tensor):
    """[M, K] -> (packed [M, Kp/2], bf16 qparams [M, G, 2]): asymmetric
    4-bit over groups of 128 k, scale=(max-min)/15 and zero=min as bf16."""
    M, K = w.shape
    G = -(-K // INT4_GROUP)
    Kp = G * INT4_GROUP
    wf = torch.zeros(M, Kp, dtype=torch.float32)
    wf[:, :K] = w.to(torch.float32)
    live = torch.zeros(Kp, dtype=torch.bool)
    live[:K] = True
    inf = float("inf")
    g = wf.view(M, G, INT4_GROUP)
    lv = live.view(1, G, INT4_GROUP)
    mn = torch.where(lv, g, torch.full_like(g, inf)).amin(2)
    mx = torch.where(lv, g, torch.full_like(g, -inf)).amax(2)
    scale = ((mx - mn) / 15.0).to(torch.bfloat16)
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    zero = mn.to(torch.bfloat16)
    nib = ((g - zero.float()[..., None]) / scale.float()[..., None]
           ).round().clamp(0, 15).to(torch.uint8)
    nib = torch.where(lv, nib, torch.zeros_like(nib)).view(M, Kp)
    return int4_pack(nib), torch.stack([scale, zero], dim=2).contiguous()


# ---------------------------------------------------------------------------
# weights of one GEMV in their stored format
@dataclass
class Weights:
    fmt: str                               # "bf16" | "fp8" | "int4"
    K: int
    w: Optional[torch.Tensor] = None       # bf16 [M, K] (or [E, M, K])
    q: Optional[torch.Tensor] = None       # fp8 bytes [M, K] / int4 packed
    scale: Optional[torch.Tensor] = None   # fp8: fp32 [M]
    qp: Optional[torch.Tensor] = None      # int4: bf16 [M, G, 2]

    def expert(self, e: Optional[int]) -> "Weights":
        if e is None or self.w is None or self.w.dim() == 2:
            return self
        return replace(self, w=self.w[e])

    def rowscale(self, dtype, shift: int = 0):
        """Per-row post-dot factor (fp8 wscale); shift=1 takes the
        neighbouring row's (mutation)."""
        if self.fmt != "fp8":
            return None
        return torch.roll(self.scale, shift).to(dtype)

    def dense(self, dtype=F64, swap_pairs=False, use_zero=True):
        """[M, K] weights as the kernel dequantises them (without the fp8
        row scale, which is applied after the dot)."""
        if self.fmt == "bf16":
            return self.w.to(dtype)
        if self.fmt == "fp8":
            return fp8_decode(self.q).to(dtype)
        nib = int4_unpack(self.q, swap_pairs).to(dtype)
        M = nib.size(0)
        s = self.qp[..., 0].to(dtype)[..., None]
        z = self.qp[..., 1].to(dtype)[..., None]
        wd = nib.view(M, -1, INT4_GROUP) * s
        if use_zero:
            wd = wd + z
        return wd.view(M, -1)[:, :self.K]

    def cond(self, xs_abs: torch.Tensor) -> torch.Tensor:
        """Condition sum of the dot with staged |x| [K] (see docstring)."""
        if self.fmt != "int4":
            return self.dense(F64).abs() @ xs_abs
        M = self.q.size(0)
        Kp = self.q.size(1) * 2
        xa = torch.zeros(Kp, dtype=F64)
        xa[:self.K] = xs_abs
        xa = xa.view(-1, INT4_GROUP)
        nib = int4_unpack(self.q).to(F64).view(M, -1, INT4_GROUP)
        s = self.qp[..., 0].to(F64)
        z = self.qp[..., 1].to(F64)
        biased = ((128.0 + nib) * xa[None]).sum(2)
        return (s.abs() * biased + (z - 128.0 * s).abs() * xa.sum(1)[None]
                ).sum(1)


# ---------------------------------------------------------------------------
# reference building blocks (the CPU mutation test recombines them)
class Staged(NamedTuple):
    xs: torch.Tensor        # staged x as the dot consumes it [K]
    post: torch.Tensor      # uniform post-dot scale (0-dim)
    exact: torch.Tensor     # staged value before any rounding [K]
    est: torch.Tensor       # fp32 error estimate of `exact` per element


def stage_x(x, nw, nb, norm, eps=EPS, rounded=True, dtype=F64,
            stat_count=None, use_eps=True, center_var=True, use_nb=True):
    """The staging pass of stage_x / the direct kernels.  The keyword knobs
    after dtype exist for the mutation test: statistics over the first
    stat_count elements only, eps omitted, LayerNorm variance without the
    -mean^2, norm bias skipped."""
    xf = x.to(dtype)
    K = xf.numel()
    one = torch.ones((), dtype=dtype)
    if norm == 0:
        return Staged(xf, one, xf, torch.zeros_like(xf))
    n = K if stat_count is None else stat_count
    e = eps if use_eps else 0.0
    g = nw.to(dtype)
    if norm == 1:
        ms = (xf[:n] * xf[:n]).sum() / K
        v = xf * g
        est = FRAG_ULPS * ACC_UNIT * v.abs()
        return Staged(bf16_round(v) if rounded else v, torch.rsqrt(ms + e),
                      v, est)
    mean = xf[:n].sum() / K
    ms = (xf[:n] * xf[:n]).sum() / K
    var = ms - mean * mean if center_var else ms
    inv = torch.rsqrt(var + e)
    core = (xf - mean) * inv * g
    v = core
    est = core.abs()
    if nb is not None:
        if use_nb:
            v = core + nb.to(dtype)
        est = est + nb.to(dtype).abs()
    return Staged(bf16_round(v), one, v, FRAG_ULPS * ACC_UNIT * est)


def fragile_mask(st: Staged) -> torch.Tensor:
    """Staged elements that fp32 arithmetic may round to the other bf16
    neighbour: closer to a rounding midpoint than their error estimate."""
    v = st.exact.to(F64)
    ulp = bf16_ulp(v)
    to_mid = ulp / 2 - (v - bf16_round(v)).abs()
    return to_mid < st.est.to(F64)


def fragile_cap(K: int) -> int:
    return max(1, K // 32)


def activation(v: torch.Tensor, kind: int) -> torch.Tensor:
    """Epilogue activations: 2 gelu(tanh), 3 silu; otherwise identity."""
    if kind == 2:
        c = 0.7978845608028654 * (v + 0.044715 * v * v * v)
        return 0.5 * v * (1.0 + torch.tanh(c))
    if kind == 3:
        return v / (1.0 + torch.exp(-v))
    return v


def linear_tail(acc, post, rowscale, bias, res, epilogue, dtype=F64,
                add_res=None):
    """acc*post*rowscale (+bias) (+res if epilogue 1), activation.
    add_res overrides when the residual is added (mutation)."""
    a = acc * post
    if rowscale is not None:
        a = a * rowscale
    if bias is not None:
        a = a + bias.to(dtype)
    if add_res is None:
        add_res = epilogue == 1
    if add_res and res is not None:
        a = a + res.to(dtype)
    return activation(a, epilogue)


class Ref(NamedTuple):
    ref: torch.Tensor       # fp64 [M], unrounded
    A: torch.Tensor         # condition sum [M]
    extra: torch.Tensor     # additive allowance [M]: flip, the epilogue's
    n_fragile: int          # two additions, a chain's first step


def _dot_parts(wt: Weights, st: Staged, rounded: bool = True):
    """(acc, A, flip, n_fragile) of one weight matrix against staged x;
    acc is before the post and row scales, A and flip carry both.  An
    unrounded path has no rounding to flip."""
    wd = wt.dense(F64)
    acc = wd @ st.xs
    post = st.post.abs()
    A = wt.cond(st.xs.abs()) * post
    frag = fragile_mask(st)
    if not rounded:
        frag = torch.zeros_like(frag)
    flip = (wd[:, frag].abs() * bf16_ulp(st.exact[frag])[None]).sum(1) * post
    rs = wt.rowscale(F64)
    if rs is not None:
        A, flip = A * rs.abs(), flip * rs.abs()
    return acc, A, flip, int(frag.sum())


def gemv_ref(wt: Weights, x, bias=None, res=None, epilogue=0, nw=None,
             nb=None, norm=0, eps=EPS, rounded=True, eidx=None) -> Ref:
    """out = act(W @ norm(x) * post (+bias) (+res)); `rounded` says whether
    the launcher's path rounds the normalised x to bf16."""
    wt = wt.expert(eidx)
    st = stage_x(x, nw, nb, norm, eps, rounded)
    acc, A, flip, nf = _dot_parts(wt, st, rounded)
    ref = linear_tail(acc, st.post, wt.rowscale(F64), bias, res, epilogue)
    # bias and residual are one fp32 addition each, not part of the K-sum
    add = torch.zeros_like(A)
    if bias is not None:
        add = add + bias.to(F64).abs()
    if epilogue == 1 and res is not None:
        add = add + res.to(F64).abs()
    extra = flip + ADD_UNIT * add
    if epilogue in (2, 3):
        A, extra = ACT_LIP * A, ACT_LIP * extra
    return Ref(ref, A, extra, nf)


def gemv_chain_ref(wt: Weights, x, res, nw, norm, eps, rounded,
                   experts) -> Ref:
    """The MoE down-projection as the engine runs it: one gemv per routed
    expert with epilogue 1, each after the first reading its residual from
    the buffer it writes (res aliased to out).  The kernel rounds every
    intermediate to bf16; the reference carries it unrounded and adds the
    previous step's whole bound to `extra` instead: that bound is exactly
    how far the kernel's bf16 intermediate may lie from the reference's,
    and it enters the next step through one exact addition."""
    K = x.numel()
    r = None
    for e in experts:
        step = gemv_ref(wt, x, None, res if r is None else r.ref, 1, nw,
                        None, norm, eps, rounded, e)
        carried = 0.0 if r is None else gemv_bound(r.ref, r.A, K, r.extra)
        r = Ref(step.ref, step.A, step.extra + carried, step.n_fragile)
    return r


def gemv_swiglu_ref(wg: Weights, wu: Weights, x, gelu_gate=False, nw=None,
                    nb=None, norm=0, eps=EPS, eidx=None, escale=None) -> Ref:
    """out = act(Wg @ xs) * (Wu @ xs) * escale; always the staged form."""
    wg, wu = wg.expert(eidx), wu.expert(eidx)
    st = stage_x(x, nw, nb, norm, eps, True)
    ga, Ag, fg, nf = _dot_parts(wg, st)
    ua, Au, fu, _ = _dot_parts(wu, st)
    g = linear_tail(ga, st.post, wg.rowscale(F64), None, None, 0)
    u = linear_tail(ua, st.post, wu.rowscale(F64), None, None, 0)
    act = activation(g, 2 if gelu_gate else 3)
    es = 1.0 if escale is None else float(escale)
    ref = act * u * es
    A = (ACT_LIP * Ag * u.abs() + act.abs() * Au) * abs(es)
    flip = (ACT_LIP * fg * u.abs() + act.abs() * fu) * abs(es)
    return Ref(ref, A, flip, nf)


def rmsnorm_ref(x, w, eps=EPS) -> Ref:
    """x [B, n] or [n]: x * rsqrt(mean(x^2)+eps) * w per row.  Every
    output is one product chain, so A = |ref| (the n-term mean square
    reaches it through the scale)."""
    xf = x.to(F64).view(-1, w.numel())
    ref = xf * torch.rsqrt((xf * xf).mean(1, keepdim=True) + eps) * w.to(F64)
    ref = ref.view(x.shape)
    return Ref(ref, ref.abs(), torch.zeros_like(ref), 0)


def layernorm_ref(x, w, b=None, eps=EPS) -> Ref:
    """(x-mean)*inv*w + b; A carries |x|+|mean| because the mean's fp32
    error is not relative to x-mean."""
    xf = x.to(F64)
    mean = xf.mean()
    inv = torch.rsqrt((xf * xf).mean() - mean * mean + eps)
    g = w.to(F64)
    ref = (xf - mean) * inv * g
    A = (xf.abs() + mean.abs()) * inv * g.abs()
    if b is not None:
        ref = ref + b.to(F64)
        A = A + b.to(F64).abs()
    return Ref(ref, A, torch.zeros_like(ref), 0)


def swiglu_mul_ref(g, u, gelu_gate=False) -> Ref:
    gf, uf = g.to(F64), u.to(F64)
    act = activation(gf, 2 if gelu_gate else 3)
    ref = act * uf
    A = ACT_LIP * gf.abs() * uf.abs() + ref.abs()
    return Ref(ref, A, torch.zeros_like(ref), 0)


# ---------------------------------------------------------------------------
# error bound
def gemv_bound(ref, A, K, flip=0.0) -> torch.Tensor:
    return REL_TERM * ref.abs() + (K + ACC_EXTRA) * ACC_UNIT * A + flip


def gemv_error_ok(got, ref, A, K, flip=0.0):
    """(ok, ratio): ok is True when every element of got is finite and
    within the bound of ref; ratio = |got-ref| / bound elementwise."""
    got = got.to(F64).cpu()
    bound = gemv_bound(ref, A, K, flip)
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(got), ratio,
                        torch.full_like(ratio, float("inf")))
    return bool((ratio <= 1.0).all()), ratio


PAD_ROWS = 24  # sentinel rows kept behind out[:M]


def new_out_buffer(M: int, device="cpu") -> torch.Tensor:
    """bf16 buffer of M + PAD_ROWS sentinels; the op writes its [:M] view."""
    return torch.full((M + PAD_ROWS,), SENTINEL, dtype=torch.bfloat16,
                      device=device)


def check_out_buffer(buf, M, r: Ref, K):
    """(ok, worst ratio, message): rows >= M still hold the sentinel, no row
    < M does, and rows < M meet the bound."""
    buf = buf.detach().cpu()
    ok, ratio = gemv_error_ok(buf[:M], r.ref, r.A, K, r.extra)
    worst = float(ratio.max())
    if not bool((buf[M:].float() == SENTINEL).all()):
        return False, worst, "a row >= M was written"
    stale = (buf[:M].float() == SENTINEL).nonzero().flatten()
    if stale.numel():
        return False, worst, f"row {int(stale[0])} (< M) was never written"
    if not ok:
        m = int(ratio.argmax())
        return False, worst, (
            f"row {m}: got {float(buf[m]):.6g} ref {float(r.ref[m]):.6g} "
            f"err/bound {worst:.3g}")
    return True, worst, ""


# ---------------------------------------------------------------------------
# launch_gemv's dispatch rule
class Dispatch(NamedTuple):
    kernel: str      # "direct" | "staged" | "direct_pre"
    rows: int        # rows per wave after the auto rule
    unr: int         # direct: W chunks in flight; direct_pre: MAXCH
    rounded: bool    # normalised x rounded to bf16 before the dot


def auto_rows(M: int, rows: int) -> int:
    if rows == 0:
        return 4 if M >= 32768 else (2 if M > 8192 else 1)
    return rows if rows in (2, 4) else 1


def gemv_dispatch(M, K, epilogue=0, norm=0, rows=0, has_res=False,
                  has_eidx=False, pre=False) -> Dispatch:
    """Which bf16 kernel launch_gemv launches.  pre: MDI_GEMV_PRE=1."""
    r = auto_rows(M, rows)
    if (pre and epilogue == 0 and norm == 1 and r == 1 and not has_eidx
            and not has_res and K >= 512 and K % 512 == 0 and K <= 8192
            and M % 4 == 0):
        return Dispatch("direct_pre", 1, 8 if K <= 4096 else 16, True)
    if norm == 0 and K <= 6144 and r == 1:
        return Dispatch("direct", r, 4, False)
    if norm != 2:
        return Dispatch("direct", r, 2, False)
    return Dispatch("staged", r, 0, True)


def wraps(M: int, rows: int) -> bool:
    """True when the 4096-block grid cap makes waves re-enter the row loop."""
    return M > WRAP_ROWS * rows


# ---------------------------------------------------------------------------
# cases and inputs
@dataclass(frozen=True)
class Case:
    op: str                  # "gemv" | "swiglu"
    fmt: str                 # "bf16" | "fp8" | "int4"
    M: int
    K: int
    epilogue: int = 0
    norm: int = 0
    rows: int = 0
    bias: bool = False       # gemv bias; with norm 2 also the norm bias
    res: bool = True         # residual tensor passed (used by epilogue 1)
    gelu_gate: bool = False
    n_expert: int = 0        # > 0: stacked bf16 weights + eidx
    eidx: int = 0
    escale: Optional[float] = None
    chain: int = 0           # > 0: a second gemv, expert `chain`, res = out
    family: str = ""

    @property
    def id(self) -> str:
        s = f"{self.family}-{self.op}-{self.fmt}-M{self.M}-K{self.K}"
        if self.op == "gemv":
            s += f"-e{self.epilogue}-n{self.norm}-r{self.rows}"
            s += "-b" if self.bias else ""
            s += "" if self.res else "-nores"
        else:
            s += f"-n{self.norm}" + ("-gelu" if self.gelu_gate else "")
        if self.n_expert:
            s += f"-x{self.eidx}of{self.n_expert}"
        if self.chain:
            s += f"-then{self.chain}"
        if self.escale is not None:
            s += f"-s{self.escale}"
        return s

    @property
    def rows_eff(self) -> int:
        return auto_rows(self.M, self.rows) if self.op == "gemv" else 1

    def dispatch(self, pre=False) -> Dispatch:
        if self.op == "gemv" and self.fmt == "bf16":
            return gemv_dispatch(self.M, self.K, self.epilogue, self.norm,
                                 self.rows, self.res, self.n_expert > 0, pre)
        return Dispatch("staged", self.rows_eff, 0, True)


@dataclass
class Inputs:
    x: torch.Tensor
    wt: Optional[Weights]             # gemv weights / swiglu gate
    wu: Optional[Weights] = None      # swiglu up
    bias: Optional[torch.Tensor] = None
    res: Optional[torch.Tensor] = None
    nw: Optional[torch.Tensor] = None
    nb: Optional[torch.Tensor] = None
    eidx_vec: Optional[torch.Tensor] = None    # int32, case.eidx at [1]
    escale_vec: Optional[torch.Tensor] = None  # fp32, case.escale at [2]
    seed: int = 0


def _bf(t):
    return t.to(torch.bfloat16).contiguous()


def _make_weights(fmt, M, K, n_expert, gen, xs_sign, align) -> Weights:
    """Random rows plus a part aligned with the staged x, so that a row's
    dot is not all cancellation and the bound has resolution (align[m] is
    the aligned amplitude in units of the random part's sigma).  fp8: row
    magnitudes 8x or more apart from both neighbours (row scales).  int4:
    groups of 128 k with clearly different offsets (zero-points).  MoE:
    n_expert distinct slabs."""
    E = max(n_expert, 1)
    w = torch.randn(E, M, K, generator=gen, dtype=torch.float32)
    w = w + align[:, None] * xs_sign[None]
    if fmt == "fp8":
        w = w * torch.tensor([1.0, 8.0, 0.25, 16.0]).repeat(-(-M // 4))[:M,
                                                                       None]
    if fmt == "int4":
        G = -(-K // INT4_GROUP)
        off = torch.tensor([-3.25, 2.5, -1.5, 4.0]).repeat(-(-G // 4))[:G]
        flip = 1.0 - 2.0 * (torch.arange(M) // 2 % 2).float()  # ++--
        w = w + off.repeat_interleave(INT4_GROUP)[:K] * flip[:, None]
    w = w / K ** 0.5
    if fmt == "bf16":
        return Weights("bf16", K, w=_bf(w if n_expert else w[0]))
    if fmt == "fp8":
        q, s = fp8_quant_rows(w[0])
        return Weights("fp8", K, q=q, scale=s)
    q, qp = int4_quant_groups(w[0])
    return Weights("int4", K, q=q, qp=qp)


def _make_inputs(case: Case, seed: int) -> Inputs:
    gen = torch.Generator().manual_seed(seed)
    M, K = case.M, case.K

    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float32)

    # non-zero mean; with a fused norm small enough for eps to matter:
    # mean(x^2) ~ 1.25e-4, so eps=1e-5 moves the RMS scale by ~4 % > 2^-7
    inp = Inputs(x=_bf((rn(K) + 0.5) * (0.01 if case.norm else 1.0)),
                 wt=None, seed=seed)
    if case.norm:
        # mixed sign and magnitude
        inp.nw = _bf(rn(K) * (0.25 + 1.5 * torch.rand(K, generator=gen)))
        if case.norm == 2 and case.bias:
            inp.nb = _bf(rn(K) * 0.25)
    st = stage_x(inp.x, inp.nw, inp.nb, case.norm, EPS, True)
    sgn = torch.sign(st.xs).float()
    alt = 0.5 * (1.0 - 2.0 * (torch.arange(M) % 2).float())  # +-0.5
    if case.op == "swiglu":
        # gate around +2: inside the activation's curved range
        gate = torch.full((M,), 2.5 / K ** 0.5)
        inp.wt = _make_weights(case.fmt, M, K, case.n_expert, gen, sgn, gate)
        inp.wu = _make_weights(case.fmt, M, K, case.n_expert, gen, sgn, alt)
    else:
        inp.wt = _make_weights(case.fmt, M, K, case.n_expert, gen, sgn, alt)
        # bias and residual of the same magnitude as the dot product
        wt = inp.wt.expert(case.eidx if case.n_expert else None)
        dot = (wt.dense(F64) @ st.xs) * st.post
        if wt.fmt == "fp8":
            dot = dot * wt.rowscale(F64)
        mag = float(dot.abs().median())
        if case.bias:
            inp.bias = _bf(rn(M) * mag)
        if case.res:
            inp.res = _bf(rn(M) * mag)
    if case.n_expert:
        inp.eidx_vec = torch.tensor([0, case.eidx, case.chain],
                                    dtype=torch.int32)
    if case.escale is not None:
        inp.escale_vec = torch.tensor([1.0, 0.0, case.escale],
                                      dtype=torch.float32)
    return inp


def count_fragile(case: Case, inp: Inputs) -> int:
    st = stage_x(inp.x, inp.nw, inp.nb, case.norm, EPS, True)
    return int(fragile_mask(st).sum())


def make_inputs(case: Case) -> Inputs:
    """Deterministic CPU inputs of a case.  The seed starts at a hash of
    the case id and advances until the reference alone has no more than
    fragile_cap(K) fragile staged elements."""
    seed = zlib.crc32(case.id.encode()) & 0x7FFFFFF
    for bump in range(64):
        inp = _make_inputs(case, seed + bump)
        if count_fragile(case, inp) <= fragile_cap(case.K):
            return inp
    raise AssertionError(f"no seed meets the fragile cap for {case.id}")


def reference(case: Case, inp: Inputs, pre: bool = False) -> Ref:
    e = case.eidx if case.n_expert else None
    if case.op == "swiglu":
        return gemv_swiglu_ref(inp.wt, inp.wu, inp.x, case.gelu_gate, inp.nw,
                               inp.nb, case.norm, EPS, e, case.escale)
    if case.chain:
        return gemv_chain_ref(inp.wt, inp.x, inp.res, inp.nw, case.norm, EPS,
                              case.dispatch(pre).rounded,
                              (case.eidx, case.chain))
    return gemv_ref(inp.wt, inp.x, inp.bias, inp.res, case.epilogue, inp.nw,
                    inp.nb, case.norm, EPS, case.dispatch(pre).rounded, e)


def run_case(ops, case: Case, inp: Inputs, device) -> torch.Tensor:
    """Launch the case's op from `ops` (the loaded extension module, passed
    in) on `device`; returns the whole sentinel-padded buffer.  eidx and
    escale go in as one-element slices at a non-zero offset, as the engine
    passes moe_eidx[j:j+1]."""
    def d(t):
        return None if t is None else t.to(device)

    M, K = case.M, case.K
    buf = new_out_buffer(M, device)
    out = buf[:M]
    x, nw, nb = d(inp.x), d(inp.nw), d(inp.nb)
    eidx = None if inp.eidx_vec is None else d(inp.eidx_vec)[1:2]
    escale = None if inp.escale_vec is None else d(inp.escale_vec)[2:3]
    wt, wu = inp.wt, inp.wu
    if case.op == "gemv":
        tail = (d(inp.bias), d(inp.res), case.epilogue, nw, nb, case.norm,
                EPS, case.rows)
        if case.fmt == "bf16":
            W = d(wt.w)
            ops.gemv(out, W, x, *tail, eidx, M * K)
            if case.chain:  # in place: the residual is the output buffer
                ops.gemv(out, W, x, None, out, *tail[2:],
                         d(inp.eidx_vec)[2:3], M * K)
        elif case.fmt == "fp8":
            ops.gemv_fp8(out, d(wt.q), d(wt.scale), x, *tail)
        else:
            ops.gemv_int4(out, d(wt.q), d(wt.qp), x, *tail)
    else:
        tail = (x, case.gelu_gate, nw, nb, case.norm, EPS)
        if case.fmt == "bf16":
            ops.gemv_swiglu(out, d(wt.w), d(wu.w), *tail, eidx, M * K,
                            escale)
        elif case.fmt == "fp8":
            ops.gemv_swiglu_fp8(out, d(wt.q), d(wt.scale), d(wu.q),
                                d(wu.scale), *tail)
        else:
            ops.gemv_swiglu_int4(out, d(wt.q), d(wt.qp), d(wu.q), d(wu.qp),
                                 *tail)
    return buf


# ---------------------------------------------------------------------------
# the GPU matrix (the CPU test walks the same list)
K_LIST = {"bf16": (8, 64, 520, 2568, 6152), "fp8": (16, 1040, 2064),
          "int4": (8, 136, 688, 2056)}
K_AWKWARD = {"bf16": 520, "fp8": 1040, "int4": 136}


def matrix_cases() -> List[Case]:
    cs: List[Case] = []
    fmts = ("bf16", "fp8", "int4")
    for fmt in fmts:  # cross product at one awkward shape
        for epi in (0, 1, 2, 3):
            for norm in (0, 1, 2):
                for rows in (1, 2, 4):
                    for bias in (False, True):
                        cs.append(Case("gemv", fmt, 4 * rows + 3,
                                       K_AWKWARD[fmt], epi, norm, rows, bias,
                                       family="cross"))
    for fmt in fmts:  # shape sweep
        for epi, norm in ((1, 1), (0, 2)):
            for rows in (0, 1, 2, 4):
                r = max(rows, 1)
                # 4r+3 and 8r-1 are both 7 at one row per wave
                for M in sorted({1, 3, 4 * r + 3, 8 * r - 1}):
                    for K in K_LIST[fmt]:
                        cs.append(Case("gemv", fmt, M, K, epi, norm, rows,
                                       True, family="sweep"))
    # bf16 without a norm: the only kernel with the K <= 6144 switch
    # (4 chunks in flight below it at one row per wave, 2 above)
    for epi in (0, 1):
        for rows in (0, 1):
            for M in (1, 3, 7):
                for K in K_LIST["bf16"]:
                    cs.append(Case("gemv", "bf16", M, K, epi, 0, rows, True,
                                   family="sweep"))
    for rows in (1, 2, 4):  # grid-stride wrap
        M = WRAP_ROWS * rows + 5
        for norm in (0, 1, 2):
            cs.append(Case("gemv", "bf16", M, 64, 1, norm, rows, True,
                           family="wrap"))
        for fmt in ("fp8", "int4"):
            cs.append(Case("gemv", fmt, M, 64, 1, 1, rows, True,
                           family="wrap"))
    for fmt in fmts:
        for norm in (1, 2):
            cs.append(Case("swiglu", fmt, WRAP_ROWS + 5, 64, norm=norm,
                           bias=norm == 2, family="wrap"))
    for fmt in fmts:  # SwiGLU
        for gelu in (False, True):
            for norm in (0, 1, 2):
                for K in K_LIST[fmt]:
                    cs.append(Case("swiglu", fmt, 7, K, norm=norm,
                                   gelu_gate=gelu, bias=norm == 2,
                                   family="swiglu"))
    for e, s in ((1, 0.375), (2, -1.75)):  # MoE indirection
        for norm in (0, 1):
            cs.append(Case("swiglu", "bf16", 7, 520, norm=norm, n_expert=3,
                           eidx=e, escale=s, family="moe"))
            # one step of the down projection, rows as the engine picks
            cs.append(Case("gemv", "bf16", 11, 520, 1, norm, 0, False,
                           n_expert=3, eidx=e, family="moe"))
            # ... and the chain itself: expert e, then the other one
            # accumulating in place (res is out), as the engine does
            cs.append(Case("gemv", "bf16", 11, 520, 1, norm, 0, False,
                           n_expert=3, eidx=e, chain=3 - e, family="moe"))
    return cs


# MDI_GEMV_PRE=1: three shapes the register-staged kernel takes (the last
# one its MAXCH=16 instantiation) and one that must fall through
PRE_CASES = [Case("gemv", "bf16", 52, K, 0, 1, 1, True, res=False,
                  family="pre") for K in (512, 4096, 4608, 520)]
