"""Shared grouped-MoE reference: fp64 routing, expert GEMMs, combine and row
kernels, their error bounds, the mutants that give the bounds teeth, and the
case tables of tests/test_moe_matrix_gpu.py.

Plain helper module built on gemv_reference.py (Weights, activation,
gemv_bound, the fp8 codecs and the constants): the CPU test of the bounds and
the GPU matrix both import it.  It is device-agnostic, computes in float64
and imports no HIP ops.

Layout convention (stated at the top of test_group_moe_gpu.py): the B*k
(token, rank) pairs are numbered f = token*k + rank; permuted row s in
[offset[e], offset[e+1]) belongs to expert e and holds pair perm[s],
ascending in f inside an expert; inv[f] = s.

Rounding points, as read off moe_group_gemm_kernel:

  * X (tokens, or the permuted bf16 ACT for the down GEMM) is staged as it
    is: no norm, no rounding.  bf16 x bf16 products are exact in fp32.
  * fp8 slabs are decode(byte) exactly; the row scale multiplies the reduced
    fp32 sum once (the gate's before its silu).
  * SwiGLU: silu(g) * u * escale in fp32, one bf16 rounding (ACT).
  * down: the reduced fp32 sum, times the row scale for fp8, stored as fp32
    (D): there is NO bf16 rounding of D.

Bounds.  None is fitted to what a GPU returns.

  ACT  gemv_bound of gemv_swiglu_ref for (token row, expert, that pair's
       escale): 2^-8 |ref| + (K+16) 2^-24 A, A propagated through silu with
       ACT_LIP.  group_swiglu_ref evaluates that formula for all rows of an
       expert at once; the CPU test holds it to gemv_swiglu_ref row by row.
  D    (K+16) 2^-24 A + 2^-24 |ref|: the accumulation term of gemv_bound
       without its bf16 result term REL_TERM, plus one fp32 rounding of the
       result (the fp8 row-scale multiply, or the last addition).
       A = |rowscale| sum_k |w_k| |x_k|.
  The split-K order needs no further term: (K+16) 2^-24 A is the worst case
  of K exact products added in ANY order, one fp32 rounding per addition,
  and the kernel's order (32-wide MFMA steps chained per wave, four waves
  added at the end) is one such order; the three extra additions of the
  cross-wave reduce and the row-scale multiply sit inside the +16.  The
  bound does assume that an MFMA accumulation errs by no more than one fp32
  rounding per product added; profiles/moe_error_margins.md records how far
  the hardware stays below that.
  combine  out = bf16(res + sum of k fp32 terms): the fp32 sum of k+1 terms
       errs by at most k 2^-24 A (A = |res| + sum |d|), the bf16 rounding by
       2^-8/(1+2^-8) of the computed sum; together at most
       2^-8 |ref| + (k+1) 2^-24 A for k <= 8.  The same for both combine
       kernels (moe_prefill_combine reads D as bf16, exactly).
  act  moe_prefill_act: gemv_bound of swiglu_mul_ref scaled by escale, K = 0.
  escale  ESCALE_RTOL of test_group_moe_gpu.py relative, plus the smallest
       normal fp32 absolute: __expf may flush a denormal result to zero.

Mutants (MUTANTS): each is a switch on the reference, not a second
implementation.  The CPU test shows that every one leaves the bound in every
case it applies to.

Out of contract, not tested: logits below -1e30 and NaN.  moe_token_topk
pads idle lanes with -1e30 and marks a taken lane with it, so such a logit
is indistinguishable from "no expert".
"""

from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import torch

import gemv_reference as R

F64 = R.F64
BF = torch.bfloat16
FP32_TINY = 2.0 ** -126     # smallest normal fp32: the escale floor
M_ROWS, N_E, TOP_K = 48, 3, 2
KC_OF_RB = {16: 512, 32: 512, 64: 256, 128: 128}
B_OF_RB = {16: 16, 32: 17, 64: 33, 128: 128}
MOE_SEG = 1024

MUTANTS = ("drop_last_chunk",      # (a)
           "drop_step",            # (b) one 32-wide step inside chunk 2
           "swap_chunks",          # (c) chunks 1 and 2 of the weight only
           "expert_plus_1",        # (d)
           "neighbour_rowscale",   # (e) fp8
           "ties_high",            # (f) routing, see route_ref
           "escale_next_rank")     # (g) escale of rank (j+1) mod k


def rb_of(B: int) -> int:
    """The RB instantiation moe_group_gemm_dispatch picks for B tokens."""
    for rb in (16, 32, 64, 128):
        if B <= rb:
            return rb
    raise ValueError(B)


def n_chunks(K: int, RB: int) -> int:
    return -(-K // KC_OF_RB[RB])


# ---------------------------------------------------------------------------
# routing
class Routing(NamedTuple):
    eidx: torch.Tensor      # long [B, k]
    escale: torch.Tensor    # fp64 [B, k]
    count: torch.Tensor     # long [n_e]
    offset: torch.Tensor    # long [n_e + 1]
    perm: torch.Tensor      # long [B*k]
    inv: torch.Tensor       # long [B*k]


def layout(eidx_flat: torch.Tensor, n_e: int):
    """(count, offset, perm, inv) of the flat [B*k] expert choice: a stable
    sort of the pairs by expert."""
    e = eidx_flat.long().reshape(-1)
    count = torch.bincount(e, minlength=n_e)
    offset = torch.cat([torch.zeros(1, dtype=torch.long), count.cumsum(0)])
    perm = torch.argsort(e, stable=True)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return count, offset, perm, inv


def route_ref(logits: torch.Tensor, k: int, ties_high=False) -> Routing:
    """Per token the top k by value, lowest index first among equals (a
    stable descending sort), softmax over the k selected logits in fp64.
    ties_high breaks ties highest index first (mutant f)."""
    lf = logits.to(F64)
    n_e = lf.size(1)
    if ties_high:
        idx = n_e - 1 - torch.sort(lf.flip(1), dim=1, descending=True,
                                   stable=True).indices[:, :k]
    else:
        idx = torch.sort(lf, dim=1, descending=True,
                         stable=True).indices[:, :k]
    escale = torch.softmax(lf.gather(1, idx), dim=1)
    return Routing(idx, escale, *layout(idx, n_e))


def gemm_routing(logits: torch.Tensor, k: int = TOP_K) -> Routing:
    """route_ref with escale rounded to fp32, as the GEMM kernels read it:
    the routing the expert-GEMM matrix uploads, so that a GEMM case tests
    the GEMM alone."""
    rt = route_ref(logits, k)
    return rt._replace(escale=rt.escale.float().to(F64))


def escale_ok(got: torch.Tensor, ref: torch.Tensor, rtol: float) -> bool:
    got, ref = got.to(F64).cpu().reshape(-1), ref.to(F64).reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return False
    return bool(((got - ref).abs() <= rtol * ref.abs() + FP32_TINY).all())


# ---------------------------------------------------------------------------
# expert slabs
@dataclass
class Slab:
    """[n_e, M, K] expert weights in their stored format."""
    fmt: str                                # "bf16" | "fp8"
    K: int
    w: Optional[torch.Tensor] = None        # bf16 [n_e, M, K]
    q: Optional[torch.Tensor] = None        # uint8 e4m3fn bytes [n_e, M, K]
    scale: Optional[torch.Tensor] = None    # fp32 [n_e, M]

    @property
    def n_e(self) -> int:
        return (self.w if self.fmt == "bf16" else self.q).size(0)

    @property
    def M(self) -> int:
        return (self.w if self.fmt == "bf16" else self.q).size(1)

    def expert(self, e: int) -> R.Weights:
        if self.fmt == "bf16":
            return R.Weights("bf16", self.K, w=self.w[e])
        return R.Weights("fp8", self.K, q=self.q[e], scale=self.scale[e])

    def dequant_bf16(self) -> torch.Tensor:
        """decode * scale as bf16; the caller asserts exactness."""
        return (R.fp8_decode(self.q) * self.scale[..., None]).to(BF)


def _dense(wt: R.Weights, RB: int, mut, dtype) -> torch.Tensor:
    """wt.dense with the K-chunk mutants applied."""
    w = wt.dense(dtype)
    KC, K = KC_OF_RB[RB], wt.K
    if mut == "drop_last_chunk":
        w = w.clone()
        w[:, (n_chunks(K, RB) - 1) * KC:] = 0
    elif mut == "drop_step":
        L = min(KC, K - 2 * KC)
        s = 2 * KC + (L // 2) // 32 * 32
        w = w.clone()
        w[:, s:s + 32] = 0
    elif mut == "swap_chunks":
        L = min(KC, K - 2 * KC)
        w = w.clone()
        a = w[:, KC:KC + L].clone()
        w[:, KC:KC + L] = w[:, 2 * KC:2 * KC + L]
        w[:, 2 * KC:2 * KC + L] = a
    return w


def _dots(x, w, RB, split):
    """x [n, K] @ w [M, K]^T.  split: in the kernel's order, 32-wide steps
    chained per wave over the chunks, then the four waves added."""
    if not split:
        return x @ w.T
    KC, K = KC_OF_RB[RB], x.size(1)
    seg = KC // 4
    acc = [torch.zeros(x.size(0), w.size(0), dtype=x.dtype) for _ in range(4)]
    for c0 in range(0, K, KC):
        for wv in range(4):
            lo = c0 + wv * seg
            for s in range(lo, min(lo + seg, K), 32):
                acc[wv] = acc[wv] + x[:, s:s + 32] @ w[:, s:s + 32].T
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


class GroupRef(NamedTuple):
    ref: torch.Tensor               # [rows, M] in the evaluation dtype
    A: Optional[torch.Tensor]       # fp64 condition sum (fp64 runs only)
    bound: Optional[torch.Tensor]


def act_bound(ref, A, K):
    return R.gemv_bound(ref.abs(), A, K)


def d_bound(ref, A, K):
    """fp32 output: no REL_TERM; see the module docstring."""
    return (K + R.ACC_EXTRA) * R.ACC_UNIT * A + R.ACC_UNIT * ref.abs()


def _src_expert(e, n_e, mut):
    return (e + 1) % n_e if mut == "expert_plus_1" else e


def group_swiglu_ref(Wg: Slab, Wu: Slab, X, rt: Routing, RB: int, mut=None,
                     dtype=F64, split=False) -> GroupRef:
    """ACT[s] = silu(x Wg[e]^T * sg) * (x Wu[e]^T * su) * escale[perm[s]]
    for every permuted row s, x = X[perm[s] // k].  dtype/split evaluate
    the same formula in fp32 (the CPU test's emulation); A and the bound
    come with the fp64 run only."""
    K, n_e, k = Wg.K, Wg.n_e, rt.eidx.size(1)
    rows = rt.perm.numel()
    es_all = rt.escale
    if mut == "escale_next_rank":
        es_all = es_all.roll(-1, dims=1)
    es_all = es_all.reshape(-1)
    shift = 1 if mut == "neighbour_rowscale" else 0
    ref = torch.zeros(rows, Wg.M, dtype=dtype)
    A = torch.zeros(rows, Wg.M, dtype=F64) if dtype == F64 else None
    for e in range(n_e):
        lo, hi = int(rt.offset[e]), int(rt.offset[e + 1])
        if hi == lo:
            continue
        f = rt.perm[lo:hi]
        x = X[f // k].to(dtype)
        es = es_all[f].to(dtype)[:, None]
        wg = Wg.expert(_src_expert(e, n_e, mut))
        wu = Wu.expert(_src_expert(e, n_e, mut))
        dg, du = _dense(wg, RB, mut, dtype), _dense(wu, RB, mut, dtype)
        g, u = _dots(x, dg, RB, split), _dots(x, du, RB, split)
        rg, ru = wg.rowscale(dtype, shift), wu.rowscale(dtype, shift)
        if rg is not None:
            g, u = g * rg, u * ru
        act = R.activation(g, 3)
        ref[lo:hi] = act * u * es
        if A is not None:
            Ag, Au = x.abs() @ dg.abs().T, x.abs() @ du.abs().T
            if rg is not None:
                Ag, Au = Ag * rg.abs(), Au * ru.abs()
            A[lo:hi] = (R.ACT_LIP * Ag * u.abs() + act.abs() * Au) * es.abs()
    return GroupRef(ref, A, None if A is None else act_bound(ref, A, K))


def group_down_ref(Wd: Slab, ACT, rt: Routing, RB: int, mut=None, dtype=F64,
                   split=False) -> GroupRef:
    """D[s] = ACT[s] Wd[e]^T * sd for every permuted row s of expert e.
    ACT is the GEMM's bf16 input as given (the kernel's own ACT in an
    end-to-end run), so the bound is for one GEMM."""
    K, n_e = Wd.K, Wd.n_e
    shift = 1 if mut == "neighbour_rowscale" else 0
    ref = torch.zeros(ACT.size(0), Wd.M, dtype=dtype)
    A = torch.zeros(ACT.size(0), Wd.M, dtype=F64) if dtype == F64 else None
    for e in range(n_e):
        lo, hi = int(rt.offset[e]), int(rt.offset[e + 1])
        if hi == lo:
            continue
        x = ACT[lo:hi].to(dtype)
        wd = Wd.expert(_src_expert(e, n_e, mut))
        dd = _dense(wd, RB, mut, dtype)
        d = _dots(x, dd, RB, split)
        rs = wd.rowscale(dtype, shift)
        if rs is not None:
            d = d * rs
        ref[lo:hi] = d
        if A is not None:
            Ad = x.abs() @ dd.abs().T
            A[lo:hi] = Ad if rs is None else Ad * rs.abs()
    return GroupRef(ref, A, None if A is None else d_bound(ref, A, K))


def combine_ref(res, D, inv, k: int) -> GroupRef:
    """res[b] + sum over ranks 0..k-1 of D[inv[b*k + rank]], entries of inv
    outside [0, B*k) skipped."""
    B = res.size(0)
    ref = res.to(F64).clone()
    A = ref.abs()
    iv = inv.long().view(B, k)
    Df = D.to(F64)
    for j in range(k):
        s = iv[:, j]
        ok = ((s >= 0) & (s < B * k))[:, None]
        d = torch.where(ok, Df[s.clamp(0, B * k - 1)],
                        torch.zeros((), dtype=F64))
        ref, A = ref + d, A + d.abs()
    bound = R.REL_TERM * ref.abs() + (k + 1) * R.ACC_UNIT * A
    return GroupRef(ref, A, bound)


def prefill_act_ref(G, U, escale, perm) -> GroupRef:
    """silu(G[s]) * U[s] * escale[perm[s]] (rows with perm in range)."""
    r = R.swiglu_mul_ref(G, U)
    es = escale.to(F64)[perm.long().clamp(0, escale.numel() - 1)][:, None]
    ref, A = r.ref * es, r.A * es.abs()
    return GroupRef(ref, A, R.gemv_bound(ref, A, 0))


def ratio(got, r: GroupRef) -> torch.Tensor:
    """|got - ref| / bound per element; inf where got is not finite."""
    g = got.detach().to(F64).cpu()
    q = (g - r.ref).abs() / r.bound.clamp_min(1e-300)
    return torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf")))


# ---------------------------------------------------------------------------
# the expert-GEMM matrix
def k_table(RB: int):
    """(label, nch, K) per chunk count the matrix visits."""
    KC = KC_OF_RB[RB]
    return [("1", 1, KC), ("2", 2, 2 * KC), ("3", 3, 3 * KC),
            ("3r", 3, 2 * KC + 32), ("4", 4, 4 * KC),
            ("5r", 5, 4 * KC + KC // 4 + 32)]


@dataclass(frozen=True)
class GemmCase:
    op: str          # "swiglu" | "down"
    fmt: str         # "bf16" | "fp8"
    RB: int
    label: str       # k_table label
    K: int
    routing: str     # "full" | "starved"

    @property
    def B(self) -> int:
        return B_OF_RB[self.RB]

    @property
    def nch(self) -> int:
        return n_chunks(self.K, self.RB)

    @property
    def id(self) -> str:
        return (f"{self.op}-{self.fmt}-RB{self.RB}-nch{self.label}"
                f"-K{self.K}-{self.routing}")


def gemm_cases() -> List[GemmCase]:
    return [GemmCase(op, fmt, RB, label, K, routing)
            for RB in (16, 32, 64, 128)
            for label, _, K in k_table(RB)
            for op in ("swiglu", "down")
            for fmt in ("bf16", "fp8")
            for routing in ("full", "starved")]


def applies(mut: str, case: GemmCase) -> bool:
    if mut in ("drop_step", "swap_chunks"):
        return case.nch >= 3
    if mut == "neighbour_rowscale":
        return case.fmt == "fp8"
    if mut == "escale_next_rank":
        return case.op == "swiglu"
    return mut != "ties_high"


def routing_logits(B: int, kind: str) -> torch.Tensor:
    """Tie-free [B, 3] logits for k = 2.  full: every token but token 1
    picks expert 0 (count B-1: one short of RB-full at B = 16 and 128), the
    other pick alternates between experts 1 and 2.  starved: expert 1 gets
    no token, experts 0 and 2 get all B.  The rank order flips every fourth
    token and the gap between the two picks varies, so the two ranks of a
    token never share an escale."""
    lg = torch.full((B, N_E), -2.0)
    for b in range(B):
        if kind == "full":
            pair = (1, 2) if b == 1 else (0, 1 + b % 2)
        else:
            pair = (0, 2)
        first, second = pair if b % 4 != 3 else pair[::-1]
        lg[b, first] = 1.0
        lg[b, second] = 1.0 - 0.25 * (1 + b % 3)
    return lg.to(BF)


@dataclass
class GemmInputs:
    logits: torch.Tensor            # bf16 [B, 3]
    X: torch.Tensor                 # bf16: swiglu [B, K]; down [B*k, K]
    Wa: Slab                        # gate (swiglu) or down slab
    Wb: Optional[Slab]              # up slab (swiglu)


def _make_slab(fmt, K, gen, mean_amp) -> Slab:
    """Random slabs, distinct per expert, plus a per-row mean (mean_amp[m]
    in units of sigma*sqrt(K)) so that against the non-zero-mean X a row's
    dot is not all cancellation.  fp8: row magnitudes 8x or more apart from
    both neighbours, so the neighbouring row's scale is visibly wrong."""
    w = torch.randn(N_E, M_ROWS, K, generator=gen)
    w = (w + mean_amp[None, :, None] / K ** 0.5) / K ** 0.5
    if fmt == "bf16":
        return Slab("bf16", K, w=w.to(BF).contiguous())
    w = w * torch.tensor([1.0, 8.0, 0.25, 16.0]).repeat(M_ROWS // 4)[None, :,
                                                                    None]
    q, s = R.fp8_quant_rows(w)
    return Slab("fp8", K, q=q, scale=s)


def make_gemm_inputs(case: GemmCase) -> GemmInputs:
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode())
                                        & 0x7FFFFFF)
    K, B = case.K, case.B
    rows = B if case.op == "swiglu" else B * TOP_K
    X = (torch.randn(rows, K, generator=gen) + 0.5).to(BF).contiguous()
    alt = 1.0 - 2.0 * (torch.arange(M_ROWS) % 2).float()
    if case.op == "swiglu":
        # gate around +2 (x has mean 0.5): inside silu's curved range
        gate = torch.full((M_ROWS,), 4.0)
        Wa, Wb = (_make_slab(case.fmt, K, gen, gate),
                  _make_slab(case.fmt, K, gen, alt))
    else:
        Wa, Wb = _make_slab(case.fmt, K, gen, alt), None
    return GemmInputs(routing_logits(B, case.routing), X, Wa, Wb)


def gemm_reference(case: GemmCase, inp: GemmInputs, rt: Routing, mut=None,
                   dtype=F64, split=False) -> GroupRef:
    if case.op == "swiglu":
        return group_swiglu_ref(inp.Wa, inp.Wb, inp.X, rt, case.RB, mut,
                                dtype, split)
    return group_down_ref(inp.Wa, inp.X, rt, case.RB, mut, dtype, split)


# ---------------------------------------------------------------------------
# exact one-hot slabs
def one_hot_K(RB: int) -> int:
    return 3 * KC_OF_RB[RB] + 32


def one_hot_tokens(B: int, K: int, shift: int) -> torch.Tensor:
    X = torch.zeros(B, K, dtype=BF)
    X[torch.arange(B), (torch.arange(B) + shift) % K] = 1.0
    return X


def exact_bf16_slab(n_e: int, M: int, K: int, salt: int) -> torch.Tensor:
    """bf16 [n_e, M, K], distinct along k inside a row (K < 2048) and 10 %
    or more apart between neighbouring k: bit patterns 0x3E00 + a stride-29
    walk through 2048 codes (2^-3 .. 2^13), sign alternating."""
    assert K < 2048
    e = torch.arange(n_e)[:, None, None]
    m = torch.arange(M)[None, :, None]
    k = torch.arange(K)[None, None, :]
    bits = 0x3E00 + (m * 37 + k * 29 + e * 411 + salt) % 2048
    bits = bits | (((m + k) & 1) << 15)
    return bits.to(torch.int16).view(BF).contiguous()


def exact_fp8_slab(n_e: int, M: int, K: int, step: int) -> Slab:
    """Finite e4m3fn codes that differ along k with power-of-two row
    scales: decode * scale is exact in bf16 (asserted by the users)."""
    finite = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F],
                          dtype=torch.uint8)
    e = torch.arange(n_e)[:, None, None]
    m = torch.arange(M)[None, :, None]
    k = torch.arange(K)[None, None, :]
    q = finite[(m * 3 + step * k + 11 * e) % 254].contiguous()
    s = (2.0 ** -(4 + (torch.arange(n_e * M) % 3))).float().view(n_e, M)
    return Slab("fp8", K, q=q, scale=s)


def swap_chunks_1_2(w: torch.Tensor, RB: int) -> torch.Tensor:
    """[.., K] with K-chunks 1 and 2 exchanged (as far as chunk 2 goes)."""
    KC = KC_OF_RB[RB]
    L = min(KC, w.size(-1) - 2 * KC)
    out = w.clone()
    out[..., KC:KC + L] = w[..., 2 * KC:2 * KC + L]
    out[..., 2 * KC:2 * KC + L] = w[..., KC:KC + L]
    return out


# ---------------------------------------------------------------------------
# router cases
class RouterCase(NamedTuple):
    id: str
    logits: torch.Tensor    # bf16 [B, n_e]
    k: int
    tie: str                # "" | "all" | "across" | "inside" | "top_idx"


def lattice_logits(B: int, n_e: int, seed: int) -> torch.Tensor:
    """Four levels 0.25 apart: ties of every kind wherever n_e > 4."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 4, (B, n_e), generator=g).float() * 0.25
            - 0.5).to(BF)


def tie_logits(n_e: int, k: int, kind: str) -> torch.Tensor:
    """Two rows: a descending ramp with the tie planted, and its mirror
    image (so the tied experts sit at low and at high indices)."""
    v = -torch.arange(n_e, dtype=torch.float32) * 0.25
    if kind == "all":
        v = torch.zeros(n_e)
    elif kind == "across":      # k-th and (k+1)-th place equal
        v[k] = v[k - 1]
    elif kind == "inside":      # first and second place equal
        v[1] = v[0]
    elif kind == "top_idx":     # the two highest indices tie for the top
        v = torch.zeros(n_e)
        v[n_e - 2:] = 1.0
        return torch.stack([v, v]).to(BF)
    return torch.stack([v, v.flip(0)]).to(BF)


def gap_logits(gap: float, n_e: int = 5) -> torch.Tensor:
    """One row: first place `gap` above the second, the rest far below."""
    v = torch.full((1, n_e), -120.0)
    base = 1.0 if 0 < gap < 1 else 0.0
    v[0, 1], v[0, 3] = base + gap, base
    return v.to(BF)


ROUTER_SHAPES = [(n_e, k) for n_e in (1, 2, 5, 8, 33, 63, 64)
                 for k in (1, 2, 3, 8) if k <= n_e]
ROUTER_B = (1, 63, 64, 65, 128)


def router_cases() -> List[RouterCase]:
    cs = []
    for i, (n_e, k) in enumerate(ROUTER_SHAPES):
        B = ROUTER_B[i % len(ROUTER_B)]
        cs.append(RouterCase(f"lattice-B{B}-ne{n_e}-k{k}",
                             lattice_logits(B, n_e, 900 + i), k, ""))
        cs.append(RouterCase(f"all-ne{n_e}-k{k}", tie_logits(n_e, k, "all"),
                             k, "all"))
        if k < n_e:
            cs.append(RouterCase(f"across-ne{n_e}-k{k}",
                                 tie_logits(n_e, k, "across"), k, "across"))
        if k >= 2:
            cs.append(RouterCase(f"inside-ne{n_e}-k{k}",
                                 tie_logits(n_e, k, "inside"), k, "inside"))
        if n_e in (5, 33, 63):
            cs.append(RouterCase(f"top_idx-ne{n_e}-k{k}",
                                 tie_logits(n_e, k, "top_idx"), k, "top_idx"))
    for B in ROUTER_B:   # every group size at one tied shape
        cs.append(RouterCase(f"lattice-B{B}-ne5-k2",
                             lattice_logits(B, 5, 950 + B), 2, ""))
    for gap in (0.0, 0.0078125, 16.0, 96.0):
        for k in (1, 2, 3):
            cs.append(RouterCase(f"gap{gap}-k{k}", gap_logits(gap), k, ""))
    return cs


# (T, k) with T*k at the segment edges of moe_route_prefill; 342*3 = 1026
# puts the three pairs of token 341 on both sides of pair 1024
PREFILL_EDGES = [(1023, 1), (512, 2), (1025, 1), (342, 3), (1024, 2),
                 (683, 3)]


def prefill_edge_cases() -> List[RouterCase]:
    return [RouterCase(f"edge-T{T}-k{k}", lattice_logits(T, 5, 970 + T), k,
                       "") for T, k in PREFILL_EDGES]
