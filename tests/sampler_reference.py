"""Draw-for-draw CPU reference of the fused sampler, and its case table.

Plain helper module (like gemv_reference.py and attn_reference.py): pure
numpy/torch on the CPU, fp64 wherever a value is real, no GPU and no
extension import.  test_sampler_reference_cpu.py checks the reference and
the preconditions of every case; test_sampler_matrix_gpu.py imports the same
case table and holds launch_sample to it.

What the sampler is specified to do (read off the sample_* kernels of
decode_kernels.hip, written here without their launch structure):

  * every bf16 logit has an integer u16 *sortable code*; positive values get
    the sign bit set, negative values are complemented.  Code order is float
    order with ONE exception: -0.0 (0x7FFF) sorts below +0.0 (0x8000), where
    a float compare calls them equal.  (NaN codes sit above +inf / below
    -inf; NaN logits are outside this reference.)
  * top-k keeps `code >= t` with t the k-th largest code, so ties at the
    k-th value are all kept.  Inactive for k <= 0 or k >= V.
  * top-p works on the codes the top-k pass kept: mass exp((l - max) *
    inv_temp) per code, walked from the top; the threshold is the first code
    whose cumulative mass reaches top_p * total.  The final threshold is the
    max of the two.  Inactive unless 0 < top_p < 1.
  * the draw is argmax over the kept set of  l * inv_temp + g_i  with
    g_i = -log(-log(uu_i)),  uu_i = (h_i >> 8) * 2^-24 + 1e-12f  in fp32,
    h_i = hash_u32(hash_u32(i ^ salt) + salt),
    salt = seed ^ (pos + pos_bias) * 0x9E3779B9 ^ slot * 0x85EBCA6B  (mod
    2^32).  On equal score the LOWEST index wins.  With the noise off the
    score is l * inv_temp alone; temperature 0 means inv_temp = 1.

The integer parts (codes, thresholds, hash, uu) are reproduced exactly.  Only
two things are real-valued in the kernel, and each gets a derived allowance.

eps: how far the kernel's fp32 score may sit from the fp64 one
---------------------------------------------------------------
u = 2^-24 is the fp32 unit roundoff, so one ulp of x is at most 2u|x|.  The
extension is built with -O3 and no fast-math: logf is the device library's
routine, whose error is bounded in ulps.  We take K = 3 ulp, the bound the
OpenCL specification sets for log and that the library is built to meet (its
documentation quotes 1 ulp; the larger figure costs nothing here).  For one
candidate, with L = |l * inv_temp| and G = |g|:

  * two logf calls.  a = logf(uu) = log(uu)(1 + t1), |t1| <= 2Ku.  The outer
    call sees log(-a) = log(-log uu) + log(1 + t1), an absolute error of
    2Ku, and adds its own K ulp, 2Ku G.  Together 2Ku (1 + G).
  * the fp32 product l * inv_temp: one rounding, u L.  (inv_temp itself is
    the same fp32 number in the kernel and here.)
  * the fp32 sum of the two: one rounding at the magnitude of the score,
    at most u (L + G).

uu is formed exactly as in the kernel (the product is exact, the sum of
1e-12f is one fp32 rounding that numpy reproduces; a fused multiply-add
gives the same bits because the product is exact), so the logf argument is
identical.  Two candidates are compared, hence

    eps = 2 [ 2Ku (1 + G) + u L + u (L + G) ]

with G and L the largest over the kept set of that draw.  G <= 27.7 always
(uu >= 1e-12) and is about 12 in a 128k vocabulary, so eps is 1e-6 to 1e-5.
A draw whose fp64 gap between best and second best exceeds eps is
*decisive*: the kernel must return exactly the reference winner.  Otherwise
the kernel's pick must lie in the kept set with an fp64 score within eps of
the best.  With the noise off every score is one exact-enough fp32 product
of a bf16 and an fp32 (distinct logits cannot collide, equal logits give
equal products), so every draw is decisive and ties go to the lowest index.

delta: how far the kernel's top-p mass fraction may sit from the fp64 one
-------------------------------------------------------------------------
The kernel sums fp32 __expf masses with float atomics in no fixed order and
decides  cum + mass[code] >= top_p * total.  For a sum of n non-negative
fp32 terms in ANY order the relative error is at most (n - 1) u to first
order.  A term whose exponent x = (l - max) * inv_temp is below -104 is
below 2^-150 and is exactly zero in fp32 (with or without denormals), and
adding zero is exact, so n counts the terms with x >= -104 only.  One term
is  exp2(fl(fl(fl(l it) - m) log2e)):  the product l*it errs by u|l it|,
the difference by u|x|, the scaling by log2e by u|x| again, the hardware
exp2 by one ulp, 2u; the rounding of m multiplies every term alike and
cancels in a fraction.  With a = max(|l it| + 2|x| + 2) over those terms,
cum and total each carry a relative error of (n + a) u, their ratio twice
that, and the product top_p * total, the remainder handed to the low-byte
pass and its re-summation add a handful of single roundings (8 u covers
them).  So a fraction moves by at most

    delta = 2 (n + a + 8) u.

A top-p case is valid only if the reference's cumulative fraction clears
top_p by delta on both sides of the boundary code (its *margin*); the
tests assert that as a precondition.

Both allowances are derived from the number formats; nothing here was fitted
to what the kernels return.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
LOGF_ULPS = 3           # bound on the device logf, in ulps
EXP_ZERO_BELOW = -104.0  # exp(x) is exactly 0 in fp32 below this
MAX_NONDECISIVE = 0.02  # share of draws of a case that may be non-decisive
SCRATCH_PER_ROW = 520   # int32 entries of sampler scratch per row
SCRATCH_CLEANED = 518   # entries [0, 518) are zero after every call

_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# codes
def bf16_bits(logits_bf16: torch.Tensor) -> np.ndarray:
    assert logits_bf16.dtype == torch.bfloat16
    return (logits_bf16.detach().cpu().contiguous().view(torch.int16)
            .numpy().astype(np.int64) & 0xFFFF)


def sortable_codes(logits_bf16: torch.Tensor) -> np.ndarray:
    """The integer u16 code of every logit (int64 array, values 0..65535).

    Code order equals float order except that -0.0 (code 0x7FFF) sorts
    strictly below +0.0 (code 0x8000)."""
    b = bf16_bits(logits_bf16)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def codes_to_bf16(codes) -> torch.Tensor:
    """Inverse of sortable_codes."""
    c = np.asarray(codes, dtype=np.int64)
    b = np.where(c & 0x8000, c & 0x7FFF, ~c & 0xFFFF)
    return torch.from_numpy(b.astype(np.uint16).view(np.int16).copy()).view(
        torch.bfloat16)


def code_of(value: float) -> int:
    """Code of a value that bf16 represents exactly."""
    t = torch.tensor([value], dtype=torch.float32).to(torch.bfloat16)
    assert float(t) == value or (value != value), value
    return int(sortable_codes(t)[0])


def inv_temp_f32(temperature: float) -> float:
    """launch_sample's inv_temp: an fp32 division, 1 at temperature 0."""
    t = np.float32(temperature)
    return float(np.float32(1.0) / t) if t > 0 else 1.0


# ---------------------------------------------------------------------------
# thresholds
def topk_threshold(codes: np.ndarray, k: int) -> int:
    """k-th largest code; the kept set is code >= t.  0 when inactive."""
    V = codes.shape[0]
    if k <= 0 or k >= V:
        return 0
    return int(np.sort(codes)[V - k])


def _masses(codes, logits_bf16, inv_temp, kt):
    l = logits_bf16.detach().cpu().to(torch.float64).numpy()
    x = (l - l.max()) * inv_temp
    sel = codes >= kt
    return l, x, sel


def topp_threshold(codes: np.ndarray, logits_bf16: torch.Tensor,
                   inv_temp: float, top_p: float, kt: int,
                   mass_kt: Optional[int] = None) -> Tuple[int, float]:
    """(final threshold, margin).  The mass is taken over codes >= kt
    (mass_kt overrides that set for the teeth, it never should in use);
    the final threshold is max(nucleus threshold, kt).  margin is the
    distance of the cumulative mass fraction from top_p, the smaller of the
    two sides of the boundary code; inf when top-p is inactive."""
    if not (0.0 < top_p < 1.0):
        return kt, math.inf
    _, x, sel = _masses(codes, logits_bf16, inv_temp,
                        kt if mass_kt is None else mass_kt)
    uc, inv = np.unique(codes[sel], return_inverse=True)
    mass = np.bincount(inv, weights=np.exp(x[sel]), minlength=uc.shape[0])
    uc, mass = uc[::-1], mass[::-1]            # from the top code down
    frac = np.cumsum(mass) / mass.sum()
    frac[-1] = 1.0
    j = int(np.argmax(frac >= top_p))
    below = float(frac[j - 1]) if j > 0 else 0.0
    margin = min(top_p - below, float(frac[j]) - top_p)
    return max(int(uc[j]), kt), margin


def topp_delta(codes: np.ndarray, logits_bf16: torch.Tensor, inv_temp: float,
               kt: int) -> float:
    """delta of the module docstring for this input."""
    l, x, sel = _masses(codes, logits_bf16, inv_temp, kt)
    live = sel & (x >= EXP_ZERO_BELOW)
    a = float((np.abs(l[live] * inv_temp) + 2 * np.abs(x[live]) + 2).max())
    return 2.0 * (int(live.sum()) + a + 8) * U


def final_threshold(logits_bf16: torch.Tensor, temperature: float, top_k: int,
                    top_p: float) -> Tuple[int, float, float]:
    """(threshold, top-p margin, delta) of one sampler call."""
    codes = sortable_codes(logits_bf16)
    it = inv_temp_f32(temperature)
    kt = topk_threshold(codes, top_k)
    t, margin = topp_threshold(codes, logits_bf16, it, top_p, kt)
    delta = (topp_delta(codes, logits_bf16, it, kt)
             if 0.0 < top_p < 1.0 else 0.0)
    return t, margin, delta


# ---------------------------------------------------------------------------
# RNG
def hash_u32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    x = x ^ (x >> np.uint32(16))
    return x


def salt_of(seed, pos, slot) -> np.ndarray:
    """seed ^ pos * 0x9E3779B9 ^ slot * 0x85EBCA6B in 32-bit wraparound
    (pos already includes pos_bias); broadcasts over arrays."""
    pos = np.asarray(pos, dtype=np.int64) & _M32
    slot = np.asarray(slot, dtype=np.int64) & _M32
    s = ((int(seed) & _M32) ^ ((pos * 0x9E3779B9) & _M32)
         ^ ((slot * 0x85EBCA6B) & _M32))
    return (s & _M32).astype(np.uint32)


def uu_of_hash(h: np.ndarray) -> np.ndarray:
    """(h >> 8) * 2^-24 + 1e-12f in float32, as the kernel forms it."""
    h = np.asarray(h, dtype=np.uint32)
    return ((h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
            + np.float32(1e-12))


def uniform_f32(idx: np.ndarray, salt: np.ndarray) -> np.ndarray:
    """uu of the given indices under the given salt (float32)."""
    salt = np.asarray(salt, dtype=np.uint32)
    return uu_of_hash(hash_u32(hash_u32(idx.astype(np.uint32) ^ salt) + salt))


def gumbel(V: int, seed: int, pos: int, slot: int,
           idx: Optional[np.ndarray] = None) -> np.ndarray:
    """fp64 Gumbel noise of indices 0..V-1 (or of idx) for one key."""
    if idx is None:
        idx = np.arange(V)
    uu = uniform_f32(np.asarray(idx), salt_of(seed, pos, slot))
    return -np.log(-np.log(uu.astype(np.float64)))


# ---------------------------------------------------------------------------
# draws
@dataclass
class Draws:
    """n draws of one (logits, threshold) over n keys."""
    winner: np.ndarray     # lowest index of the best fp64 score, -1 if none
    gap: np.ndarray        # best minus second-best fp64 score
    eps: np.ndarray        # the fp32 allowance of that draw
    best: np.ndarray       # best fp64 score
    decisive: np.ndarray   # gap > eps (always, with the noise off)
    kept: np.ndarray       # kept indices, ascending
    _score_of: object = None

    def score(self, draw: int, token: int) -> float:
        return self._score_of(draw, token)

    def head(self, m: int) -> "Draws":
        """The first m draws."""
        return Draws(self.winner[:m], self.gap[:m], self.eps[:m],
                     self.best[:m], self.decisive[:m], self.kept,
                     self._score_of)


def draw_many(logits_bf16: torch.Tensor, threshold: int, inv_temp: float,
              noise: bool, seed: int, pos, slot) -> Draws:
    """Reference draws for the keys (seed, pos[j], slot[j]); pos includes
    pos_bias.  pos and slot broadcast against each other."""
    codes = sortable_codes(logits_bf16)
    pos, slot = np.broadcast_arrays(np.atleast_1d(np.asarray(pos)),
                                    np.atleast_1d(np.asarray(slot)))
    n = pos.shape[0]
    kept = np.nonzero(codes >= threshold)[0]
    base = (logits_bf16.detach().cpu().to(torch.float64).numpy()[kept]
            * inv_temp)
    salts = salt_of(seed, pos, slot)
    winner = np.full(n, -1, dtype=np.int64)
    gap = np.full(n, math.inf)
    best = np.full(n, -math.inf)
    gmax = np.zeros(n)
    K = kept.shape[0]

    def score_of(j, token):
        s = float(logits_bf16[token].double()) * inv_temp
        if noise:
            uu = uniform_f32(np.array([token]), salts[j])
            s += float(-np.log(-np.log(uu.astype(np.float64)))[0])
        return s

    if K:
        step = max(1, (1 << 22) // K)
        for a in range(0, n, step):
            b = min(n, a + step)
            if noise:
                uu = uniform_f32(kept[None, :], salts[a:b, None])
                g = -np.log(-np.log(uu.astype(np.float64)))
                s = base[None, :] + g
                gmax[a:b] = np.abs(g).max(axis=1)
            else:
                s = np.broadcast_to(base[None, :], (b - a, K))
            w = s.argmax(axis=1)          # first maximum = lowest index
            winner[a:b] = kept[w]
            best[a:b] = s[np.arange(b - a), w]
            if K > 1:
                s2 = s.copy()
                s2[np.arange(b - a), w] = -math.inf
                gap[a:b] = best[a:b] - s2.max(axis=1)
    if noise:
        L = float(np.abs(base).max()) if K else 0.0
        eps = 2.0 * (2 * LOGF_ULPS * U * (1 + gmax) + U * L + U * (L + gmax))
        decisive = gap > eps
    else:
        eps = np.zeros(n)
        decisive = np.ones(n, dtype=bool)
    return Draws(winner, gap, eps, best, decisive, kept, score_of)


def draw(logits_bf16: torch.Tensor, threshold: int, inv_temp: float,
         noise: bool, seed: int, pos: int, slot: int
         ) -> Tuple[int, float, float]:
    """(winner, gap, eps) of one draw; see draw_many."""
    d = draw_many(logits_bf16, threshold, inv_temp, noise, seed, [pos],
                  [slot])
    return int(d.winner[0]), float(d.gap[0]), float(d.eps[0])


def check_draws(ref: Draws, got: Sequence[int]) -> Tuple[int, int, str]:
    """Hold the kernel's tokens to the reference.  Returns (decisive draws,
    draws, message); the message is empty when everything holds: exact
    winners on decisive draws, kept-set membership and a score within eps
    of the best on the others, and at most 2% of the others."""
    got = np.asarray(got, dtype=np.int64)
    n = got.shape[0]
    assert n == ref.winner.shape[0]
    dec = ref.decisive
    bad = np.nonzero(dec & (got != ref.winner))[0]
    if bad.size:
        j = int(bad[0])
        return int(dec.sum()), n, (
            f"{bad.size} of {n} decisive draws differ; first at draw {j}: "
            f"kernel {int(got[j])}, reference {int(ref.winner[j])} "
            f"(gap {ref.gap[j]:.3g}, eps {ref.eps[j]:.3g})")
    kept = set(ref.kept.tolist())
    for j in np.nonzero(~dec)[0]:
        tok = int(got[j])
        if tok not in kept:
            return int(dec.sum()), n, f"draw {j}: {tok} is not in the kept set"
        if ref.best[j] - ref.score(int(j), tok) > ref.eps[j]:
            return int(dec.sum()), n, (
                f"draw {j}: {tok} scores more than eps below the best")
    if (n - int(dec.sum())) > MAX_NONDECISIVE * n:
        return int(dec.sum()), n, (
            f"{n - int(dec.sum())} of {n} draws are not decisive")
    return int(dec.sum()), n, ""


# ---------------------------------------------------------------------------
# the case table
def ladder(c0: int, n: int):
    """n consecutive codes from c0 down."""
    return [c0 - i for i in range(n)]


@dataclass(frozen=True)
class Case:
    """One sampler setting, drawn n times: row j of a batched call has the
    same logits and the key (seed, pos0 + j, slot)."""
    id: str
    V: int
    T: float
    k: int = 0
    p: float = 1.0
    n: int = 256
    # logits: `head` codes (placed at scattered indices) over a background
    # of codes in [bg_lo, bg_hi] below them; or randn * scale when head is
    # empty
    head: Tuple[int, ...] = ()
    bg: Tuple[int, int] = (0, 0)
    scale: float = 1.0
    lseed: int = 0
    seed: int = 7
    slot: int = 3
    pos0: int = 0
    # perturbed references the kernel must disagree with:
    #   lower / higher: final threshold one code lower / higher
    #   key: pos and slot swapped
    #   nomask: top-p mass not restricted to the top-k set
    teeth: Tuple[str, ...] = ()


@functools.lru_cache(maxsize=None)
def _case_logits(case: Case) -> torch.Tensor:
    rng = np.random.RandomState(1000 + case.lseed)
    if not case.head:
        g = torch.Generator().manual_seed(case.lseed)
        return (torch.randn(case.V, generator=g) * case.scale).to(
            torch.bfloat16)
    codes = rng.randint(case.bg[0], case.bg[1] + 1, size=case.V)
    assert case.bg[1] < min(case.head)
    where = rng.permutation(case.V)[:len(case.head)]
    codes[where] = np.asarray(case.head)
    return codes_to_bf16(codes)


def case_logits(case: Case) -> torch.Tensor:
    """The case's [V] bf16 logits (cached; do not modify)."""
    return _case_logits(case)


def case_keys(case: Case, swapped: bool = False):
    pos = case.pos0 + np.arange(case.n)
    slot = np.full(case.n, case.slot)
    return (slot, pos) if swapped else (pos, slot)


@functools.lru_cache(maxsize=None)
def case_reference(case: Case):
    """(threshold, margin, delta, Draws) of the case."""
    lg = case_logits(case)
    t, margin, delta = final_threshold(lg, case.T, case.k, case.p)
    pos, slot = case_keys(case)
    d = draw_many(lg, t, inv_temp_f32(case.T), True, case.seed, pos, slot)
    return t, margin, delta, d


def perturbed_winners(case: Case, tooth: str) -> np.ndarray:
    """Winners of a deliberately wrong reference (see Case.teeth)."""
    lg = case_logits(case)
    it = inv_temp_f32(case.T)
    t = case_reference(case)[0]
    pos, slot = case_keys(case, swapped=(tooth == "key"))
    if tooth == "lower":
        t -= 1
    elif tooth == "higher":
        t += 1
    elif tooth == "nomask":
        codes = sortable_codes(lg)
        kt = topk_threshold(codes, case.k)
        t, _ = topp_threshold(codes, lg, it, case.p, kt, mass_kt=0)
    else:
        assert tooth == "key", tooth
    return draw_many(lg, t, it, True, case.seed, pos, slot).winner


def _threshold_cases():
    NOISY = 50.0   # temperature at which the noise dominates
    full = ("lower", "higher", "key")
    one = ("lower", "higher")   # one kept token: no key can change the draw
    pos_bg = (code_of(2.0 ** -9), code_of(1.0))
    base = ladder(code_of(8.0) - 1, 300)        # 7.97 down to 1.3
    out = []
    for k in (1, 2, 8, 255, 256, 257):
        out.append(Case(f"k{k}", 4096, NOISY, k=k, head=tuple(base),
                        bg=pos_bg, n=2048 if k > 8 else 256,
                        teeth=one if k == 1 else full))
    # all negative: the threshold takes the complemented branch of the map
    neg = ladder(code_of(-1.0), 300)
    out.append(Case("negative_k8", 4096, NOISY, k=8, head=tuple(neg),
                    bg=(min(neg) - 1500, min(neg) - 1), teeth=full))
    # straddling zero, +0 and -0 both present and each once the threshold
    zero = [code_of(v) for v in (2.0, 1.0, 0.5)] + [0x8000, 0x7FFF, 0x7FFE] \
        + [code_of(v) for v in (-0.5, -1.0, -1.5, -2.0, -3.0, -4.0)]
    zbg = (code_of(-4096.0), code_of(-8.0))
    out.append(Case("zero_plus_is_threshold", 4096, NOISY, k=4,
                    head=tuple(zero), bg=zbg, teeth=full))
    out.append(Case("zero_minus_is_threshold", 4096, NOISY, k=5,
                    head=tuple(zero), bg=zbg, teeth=full))
    # low byte 0x00 (also: cum + count == k at a bucket edge, cum == 0) and
    # low byte 0xFF, the first code of the next hi bucket down
    c1 = ladder(0xC105, 300)
    out.append(Case("lo_byte_00", 4096, NOISY, k=6, head=tuple(c1),
                    bg=pos_bg, teeth=full))
    out.append(Case("lo_byte_ff", 4096, NOISY, k=7, head=tuple(c1),
                    bg=pos_bg, teeth=full))
    # hi scan: 3 in bucket 0xC2, exactly 5 more in 0xC1 -> cum + count == 8
    edge = [0xC202, 0xC201, 0xC200] + ladder(0xC104, 300)
    out.append(Case("bucket_edge", 4096, NOISY, k=8, head=tuple(edge),
                    bg=pos_bg, teeth=full))
    # three tokens share the 8th value: 10 are kept
    c0 = base[0]
    tie = ladder(c0, 7) + [c0 - 7] * 3 + ladder(c0 - 8, 290)
    out.append(Case("tie_at_kth", 4096, NOISY, k=8, head=tuple(tie),
                    bg=pos_bg, teeth=full))
    # top-p only.  The ladder of consecutive codes sits where one bf16 step
    # times inv_temp is 1 (T 0.5) or 0.5 (T 1 and 2): a mass ratio of e^-1
    # or e^-0.5 per code, so the boundary token of every p keeps a mass
    # well above delta; the background is so far below that its fp32 mass
    # is exactly zero.  p 0.999 needs many draws: whatever lies below its
    # boundary holds under 0.1% of the mass, and has to win once.
    far = (code_of(-65536.0), code_of(-4096.0))
    top = {0.5: 100.0, 1.0: 100.0, 2.0: 200.0}
    for i, T in enumerate((0.5, 1.0, 2.0)):
        for p in (0.1, 0.5, 0.9, 0.999):
            alone = p < 0.3 or (T == 0.5 and p == 0.5)
            out.append(Case(f"p{p}_T{T}", 4096, T, p=p,
                            head=tuple(ladder(code_of(top[T]), 24)), bg=far,
                            n=16384 if p > 0.99 else 256, lseed=i,
                            teeth=one if alone else full))
    # one dominant logit: the nucleus is that token alone
    out.append(Case("dominant", 4096, 2.0, p=0.9,
                    head=tuple(ladder(code_of(1536.0), 8)), bg=far, n=512,
                    teeth=one))
    # top-k with top-p: p tighter than k (the only setting in which the
    # restriction of the mass to the top-k set can show), and k tighter
    both = tuple(ladder(code_of(100.0), 24))
    out.append(Case("k4_p0.85_p_tighter", 4096, 1.0, k=4, p=0.85, head=both,
                    bg=far, teeth=full + ("nomask",)))
    out.append(Case("k3_p0.999_k_tighter", 4096, 1.0, k=3, p=0.999,
                    head=both, bg=far, teeth=full))
    return out


def _shape_cases():
    out = [
        Case("V1", 1, 0.8, n=8),
        Case("V1_k5_above_V", 1, 0.8, k=5, n=8),
        Case("V1_p0.5", 1, 0.8, p=0.5, n=8),
        Case("V63", 63, 0.8, n=64, lseed=1),
        Case("V63_k8", 63, 0.8, k=8, n=64, lseed=1),
        Case("V63_k64_above_V", 63, 0.8, k=64, n=64, lseed=1),
        Case("V1000", 1000, 0.8, n=256, lseed=2),
        Case("V1000_k50", 1000, 0.8, k=50, n=256, lseed=2),
        Case("V1000_p0.6", 1000, 0.8, p=0.6, n=256, lseed=2),
        Case("V4096_T50_k8", 4096, 50.0, k=8, n=256, lseed=3),
        Case("V32769", 32769, 0.8, n=64, lseed=4),
        Case("V32769_k200", 32769, 0.8, k=200, n=64, lseed=4),
        Case("V128256", 128256, 0.8, n=64, lseed=5),
        Case("V128256_k200", 128256, 0.8, k=200, n=256, lseed=5),
    ]
    return out


THRESHOLD_CASES = {c.id: c for c in _threshold_cases()}
SHAPE_CASES = {c.id: c for c in _shape_cases()}
SINGLE_DRAWS = 64   # draws of a case that also go through the one-row path

# greedy ties: (V, indices that share the maximum)
TIE_CASES = {
    "same_wave": (40000, (5, 37)),
    "same_block_two_waves": (40000, (5, 70)),
    "one_thread_at_32_blocks": (40000, (0, 8192)),
    "one_thread_at_128_blocks": (40000, (100, 32868)),
    "three_blocks": (40000, (300, 9000, 33000)),
}


def tie_logits(name: str) -> torch.Tensor:
    V, idx = TIE_CASES[name]
    g = torch.Generator().manual_seed(len(name))
    lg = torch.randn(V, generator=g).clamp_(max=5.0)
    lg[list(idx)] = 20.0
    return lg.to(torch.bfloat16)


# batched rows with distinct logits, pos and slot: (top_k, top_p) per mode
BATCH_V = 1000
BATCH_T = 0.8
BATCH_MODES = {"none": (0, 1.0), "k": (50, 1.0), "p": (0, 0.6),
               "k_and_p": (50, 0.8)}


@functools.lru_cache(maxsize=None)
def batch_rows(B: int):
    """(logits [B, V] bf16, pos [B], slot [B]) for the batched-equals-single
    test.  Rows are randn draws; a candidate row whose top-p margin does not
    clear delta in either top-p mode is passed over (decided here, on the
    reference alone), so float summation order cannot move a threshold."""
    rows, lseed = [], 100 * B
    while len(rows) < B:
        g = torch.Generator().manual_seed(lseed)
        lg = torch.randn(BATCH_V, generator=g).to(torch.bfloat16)
        lseed += 1
        ok = True
        for k, p in BATCH_MODES.values():
            _, margin, delta = final_threshold(lg, BATCH_T, k, p)
            ok = ok and margin >= delta
        if ok:
            rows.append(lg)
    pos = np.array([11 + 3 * b for b in range(B)])
    slot = np.array([(5 * b + 2) % 7 for b in range(B)])
    return torch.stack(rows), pos, slot
