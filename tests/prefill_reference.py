"""Shared prefill references, error bounds, input generators and case
matrices: prefill_attn (both kernels), rope_prefill_append and mtile_gemm.

Plain helper module (like attn_reference.py and gemv_reference.py, which it
imports and does not copy).  The CPU test of the bounds, the GPU matrices
and their child processes all import it.  It is device-agnostic, computes
in float64 and imports no HIP ops.

prefill_attn
------------
The reference mirrors the kernels only at the rounding points read off
prefill_attn_kernel (v1) and prefill_attn_mfma_kernel (v2):

  * q (already roped) and bf16 pool K/V are bf16 as given;
  * fp8 K is e4m3fn(byte) * kscale[row], an fp32 multiply, rounded to bf16
    (pool_rows(round_bf16=True));
  * fp8 V takes the same path: both kernels dequantise V through
    fp8x8_to_bf16, so V is rounded to bf16 after the fp32 multiply (the
    decode kernels do not round V; the decode reference does not either);
  * scores, the causal softmax (key <= pos0 + t) and PV are exact, and the
    output is not rounded.

Error bound (prefill_error_ok):  |got - ref| <= 2^-8 |ref| + c A  with
A[t,h,d] = sum_s p[t,h,s] |V[s,d]|.

  * 2^-8 |ref| is the one bf16 rounding of the result, as for decode.
  * v1 keeps P in fp32 and accumulates PV in fp32: the decode constant
    c = 2^-9 carries over (fp32 accumulation, __expf, relative to the
    condition number of a softmax-weighted sum).
  * v2 rounds every P to bf16 before the PV MFMA, while the denominator l
    sums the unrounded P.  One bf16 rounding moves each p by at most
    2^-9 p, so the numerator moves by at most 2^-9 sum p|V| = 2^-9 A and
    nothing in l cancels it: c = 2^-9 + 2^-9 = 2^-8.

Both constants come from the number formats; neither is fitted to what a
GPU returns.  profiles/prefill_error_margins.md has the measured ratios.

rope_prefill_append
-------------------
rope_append_reference is rope_rows (rotate-half, pairs (d, d + ne/2)) at
cos[pos0 + t] for every t, on the q rows and the k row of every kv group,
in fp64 and unrounded; v rows and dims >= rope_ne pass through.

mtile_gemm
----------
mtile_reference is fp64 X W^T (+bias) (+res) with the GEMV bound of
gemv_reference: 2^-8 |ref| + (K+16) 2^-24 A + 2^-23 (|bias| + |res|),
A = |X| |W|^T.
"""

from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

import gemv_reference as G
from attn_reference import (BF16_GARBAGE, FP8_GARBAGE_BYTE,
                            FP8_GARBAGE_SCALE, W_MAX, W_MIN, _write_row,
                            bf16_round, fp8_quant_rows, pool_rows, rope_rows,
                            rope_tables)

F64 = torch.float64
REL_TERM = 2.0 ** -8
C_V1 = 2.0 ** -9                 # fp32 P (prefill_attn_kernel)
C_V2 = 2.0 ** -9 + 2.0 ** -9     # bf16 P before the PV MFMA (v2)
LEAK_MARGIN = 15.0               # a leaked key scores this far above the max
SENTINEL = G.SENTINEL
PAD = 64                         # sentinel elements kept behind an output

N_KV, N_SLOTS, N_LAYERS, SLOT, LAYER, MAX_SEQ = 2, 3, 2, 1, 1, 320


# ---------------------------------------------------------------------------
# prefill_attn reference
def split_q(qkv: torch.Tensor, n_kv: int, hs: int, dtype=F64):
    """[T, qkv_dim] -> q [T, n_kv, qpk, hs]."""
    T = qkv.shape[0]
    grp = qkv.reshape(T, n_kv, -1, hs)
    return grp[:, :, :grp.shape[2] - 2].to(dtype)


def gather_kv(kpool, vpool, kscale, vscale, slot, layer, n_rows, dtype=F64):
    """(K, V) [n_kv, n_rows, hs] as the prefill kernels dequantise them."""
    K = pool_rows(kpool, kscale, slot, layer, n_rows, dtype, True)
    V = pool_rows(vpool, vscale, slot, layer, n_rows, dtype, True)
    return K, V


def causal_visible(T: int, S: int, pos0: int) -> torch.Tensor:
    """[T, S] bool: key s is visible to query row t."""
    return torch.arange(S)[None, :] <= (pos0 + torch.arange(T))[:, None]


def scores(q, K, scale):
    """Unmasked scaled scores [T, n_kv, qpk, S]."""
    return torch.einsum("tgjd,gsd->tgjs", q, K) * scale


def attend_masked(q, K, V, scale, visible):
    """Exact softmax attention under a [T, S] visibility mask:
    (out, A) [T, n_head, hs] and p [T, n_head, S]."""
    T, n_kv, qpk, hs = q.shape
    sc = scores(q, K, scale).masked_fill(~visible[:, None, None, :],
                                         -math.inf)
    p = torch.softmax(sc, dim=-1)
    out = torch.einsum("tgjs,gsd->tgjd", p, V)
    A = torch.einsum("tgjs,gsd->tgjd", p, V.abs())
    nh = n_kv * qpk
    return out.reshape(T, nh, hs), A.reshape(T, nh, hs), p.reshape(T, nh, -1)


class PrefillRef(NamedTuple):
    out: torch.Tensor   # [T, n_head, hs] fp64, unrounded
    A: torch.Tensor     # [T, n_head, hs]
    p: torch.Tensor     # [T, n_head, S]


def prefill_reference(qkv, kpool, vpool, pos0, slot, layer, scale,
                      kscale=None, vscale=None, dtype=F64) -> PrefillRef:
    n_kv, hs = kpool.shape[2], kpool.shape[4]
    T = qkv.shape[0]
    S = pos0 + T
    q = split_q(qkv, n_kv, hs, dtype)
    K, V = gather_kv(kpool, vpool, kscale, vscale, slot, layer, S, dtype)
    return PrefillRef(*attend_masked(q, K, V, scale,
                                     causal_visible(T, S, pos0)))


# ---------------------------------------------------------------------------
# metric
def prefill_bound(ref, A, c):
    return REL_TERM * ref.abs() + c * A


def prefill_error_ratio(got, ref, A, c) -> float:
    """max |got - ref| / bound (inf for a non-finite output); got is bf16."""
    assert got.dtype == torch.bfloat16, "the kernel output is bf16"
    g = got.detach().cpu().to(ref.dtype).reshape(ref.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float(((g - ref).abs() / prefill_bound(ref, A, c)).max())


def prefill_error_ok(got, ref, A, c) -> bool:
    """|got - ref| <= 2^-8 |ref| + c A elementwise; got is bf16."""
    assert got.dtype == torch.bfloat16, "the kernel output is bf16"
    g = got.detach().cpu().to(ref.dtype).reshape(ref.shape)
    return bool(((g - ref).abs() <= prefill_bound(ref, A, c)).all())


# ---------------------------------------------------------------------------
# generator
class Probe(NamedTuple):
    t: int      # query row (relative to the prompt)
    g: int      # kv group
    key: int    # absolute key index
    j: int      # head within the group that the key is planted for
    want: float


class Leak(NamedTuple):
    t: int
    g: int
    key: int    # pos0 + t + 1: the first key row t must not see
    j: int


@dataclass
class PrefillCase:
    name: str
    qpk: int
    n_kv: int
    hs: int
    max_seq: int
    slot: int
    layer: int
    scale: float
    pos0: int
    T: int
    mode: str
    family: str
    qkv: torch.Tensor            # bf16 [T, qkv_dim], q already roped
    kpool: torch.Tensor          # bf16 or uint8 [slots, layers, n_kv, seq, hs]
    vpool: torch.Tensor
    kscale: Optional[torch.Tensor]
    vscale: Optional[torch.Tensor]
    probes: List[Probe] = field(default_factory=list)
    leaks: List[Leak] = field(default_factory=list)

    @property
    def n_head(self):
        return self.n_kv * self.qpk

    @property
    def S(self):
        return self.pos0 + self.T

    @property
    def kv8(self):
        return self.kscale is not None

    def reference(self, **over) -> PrefillRef:
        a = dict(qkv=self.qkv, kpool=self.kpool, vpool=self.vpool,
                 pos0=self.pos0, slot=self.slot, layer=self.layer,
                 scale=self.scale, kscale=self.kscale, vscale=self.vscale)
        a.update(over)
        return prefill_reference(**a)

    def qKV(self):
        q = split_q(self.qkv, self.n_kv, self.hs)
        K, V = gather_kv(self.kpool, self.vpool, self.kscale, self.vscale,
                         self.slot, self.layer, self.S)
        return q, K, V

    def probe_weights(self, ref: PrefillRef):
        return [(pr, float(ref.p[pr.t, pr.g * self.qpk + pr.j, pr.key]))
                for pr in self.probes]

    def leak_margins(self):
        """Score of each leak key on its (row, head) minus that row's
        maximum over the keys it may see."""
        q, K, _ = self.qKV()
        sc = scores(q, K, self.scale)
        res = []
        for lk in self.leaks:
            row = sc[lk.t, lk.g, lk.j]
            res.append((lk, float(row[lk.key]
                                  - row[:self.pos0 + lk.t + 1].max())))
        return res

    def probes_ok(self, ref: PrefillRef) -> bool:
        """The precondition of every comparison: each probe carries weight
        in [0.02, 0.5] on its (row, head), and each leak key scores at
        least 15 above the maximum of the row that must not see it."""
        return (all(W_MIN <= w <= W_MAX for _, w in self.probe_weights(ref))
                and all(m >= LEAK_MARGIN for _, m in self.leak_margins()))


def designated_rows(T: int) -> List[int]:
    return sorted({t for t in (0, 15, 16, T - 1) if 0 <= t < T})


def probe_candidates(pos0: int, t: int) -> List[int]:
    """Candidate probe keys of row t, the diagonal first.  A row with a
    single visible key has none: that key carries weight 1."""
    last = pos0 + t
    if last < 1:
        return []
    cand = [last, last - 1, 0, 15, 16, 63, 64, pos0 - 1, pos0]
    seen, out = set(), []
    for c in cand:
        if 0 <= c <= last and c not in seen:
            seen.add(c)
            out.append(c)
    return out


def assign_probes(pos0: int, T: int) -> Tuple[Dict[int, List[int]],
                                               Dict[int, int]]:
    """(row -> probe keys, row -> leak key).  A pool row holds one planted
    vector, so every key serves one row: leak keys (pos0 + t + 1 for each
    designated t < T-1) come first, then the rows take turns claiming
    their next free candidate."""
    rows = designated_rows(T)
    leak = {t: pos0 + t + 1 for t in rows if t < T - 1}
    taken = set(leak.values())
    cand = {t: probe_candidates(pos0, t) for t in rows}
    got: Dict[int, List[int]] = {t: [] for t in rows}
    progress = True
    while progress:
        progress = False
        for t in rows:
            while cand[t]:
                c = cand[t].pop(0)
                if c not in taken:
                    taken.add(c)
                    got[t].append(c)
                    progress = True
                    break
    return got, leak


def make_prefill_case(name, qpk, hs, T, pos0, kv8=False, mode="random",
                      family="", n_kv=N_KV, max_seq=MAX_SEQ, slot=SLOT,
                      layer=LAYER, n_layers=N_LAYERS, n_slots=N_SLOTS,
                      scale=None) -> PrefillCase:
    """Inputs of one prefill_attn call.

    Pools are N(0,1) in every slot and layer; rows >= pos0 + T of the live
    slot hold large finite garbage.  qkv is random bf16: its q part is
    used as the roped q, its k/v parts are never read by prefill_attn.
    Probe keys are planted as K[key] = tau q / (scale |q|^2) for the bf16
    q of one (row, head); tau is refined on the reference until the weight
    is 0.5 / (probes on that (row, head) + 1).  Leak keys are planted the
    same way with tau = row maximum + 16.

    mode shapes the non-probe keys as seen from the last row:
    "ascending" / "descending" ramp the scores over 0..12 with the key
    index, "outlier" plants one key at about -30 and one at about +12."""
    S = pos0 + T
    assert 1 <= T and S <= max_seq
    scale = 1.0 / math.sqrt(hs) if scale is None else scale
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFF)
    qkv = torch.randn(T, n_kv * (qpk + 2) * hs, generator=gen).to(
        torch.bfloat16)
    shape = (n_slots, n_layers, n_kv, max_seq, hs)
    kf = torch.randn(shape, generator=gen)
    vf = torch.randn(shape, generator=gen)
    q = split_q(qkv, n_kv, hs)                     # [T, n_kv, qpk, hs]

    if mode != "random":
        q_last = q[T - 1]
        u = q_last.mean(dim=1)                     # [n_kv, hs]
        per_unit = scale * torch.einsum("gjd,gd->gj", q_last, u).mean(1)
        if mode == "outlier":
            ramp = torch.zeros(S, dtype=F64)
            noise = 1.0
            if S >= 8:
                ramp[S // 3] = -30.0
                ramp[(2 * S) // 3] = 12.0
        else:
            ramp = torch.linspace(0.0, 12.0, S, dtype=F64)
            if mode == "descending":
                ramp = ramp.flip(0)
            noise = 0.25
        rows = (ramp[None, :, None] / per_unit[:, None, None]) * u[:, None]
        kf[slot, layer, :, :S] = noise * kf[slot, layer, :, :S] + rows.float()

    if kv8:
        kpool, kscale = fp8_quant_rows(kf)
        vpool, vscale = fp8_quant_rows(vf)
    else:
        kpool, vpool = kf.to(torch.bfloat16), vf.to(torch.bfloat16)
        kscale = vscale = None
    del kf, vf
    sl = (slot, slice(None), slice(None), slice(S, None))
    if kv8:
        kpool[sl] = FP8_GARBAGE_BYTE
        vpool[sl] = FP8_GARBAGE_BYTE
        kscale[sl] = FP8_GARBAGE_SCALE
        vscale[sl] = FP8_GARBAGE_SCALE
    else:
        kpool[sl] = BF16_GARBAGE
        vpool[sl] = -BF16_GARBAGE

    case = PrefillCase(name, qpk, n_kv, hs, max_seq, slot, layer, scale,
                       pos0, T, mode, family, qkv, kpool, vpool, kscale,
                       vscale)
    keys, leak = assign_probes(pos0, T)
    for t, ks in keys.items():
        on_head = [sum(1 for i in range(len(ks)) if i % qpk == j)
                   for j in range(qpk)]
        for i, key in enumerate(ks):
            j = i % qpk
            for g in range(n_kv):
                case.probes.append(Probe(t, g, key, j,
                                         0.5 / (on_head[j] + 1)))
    for n, (t, key) in enumerate(sorted(leak.items())):
        for g in range(n_kv):
            case.leaks.append(Leak(t, g, key, n % qpk))

    tau_p = [math.log(pos0 + pr.t + 1) + 1.0 for pr in case.probes]
    tau_l = [20.0 for _ in case.leaks]

    def plant():
        for pr, tau in zip(case.probes, tau_p):
            v = q[pr.t, pr.g, pr.j]
            _write_row(kpool, kscale, (slot, layer, pr.g, pr.key),
                       tau * v / (scale * float(v @ v)))
        for lk, tau in zip(case.leaks, tau_l):
            v = q[lk.t, lk.g, lk.j]
            _write_row(kpool, kscale, (slot, layer, lk.g, lk.key),
                       tau * v / (scale * float(v @ v)))

    for _ in range(8 if (case.probes or case.leaks) else 0):
        plant()
        ref = case.reference()
        for n, pr in enumerate(case.probes):
            w = float(ref.p[pr.t, pr.g * qpk + pr.j, pr.key].clamp(
                1e-300, 1 - 1e-12))
            tau_p[n] += (math.log(pr.want / (1 - pr.want))
                         - math.log(w / (1 - w)))
        for n, (lk, m) in enumerate(case.leak_margins()):
            tau_l[n] += (LEAK_MARGIN + 1.0) - m
    plant()
    return case


def run_prefill(ops, case: PrefillCase, device):
    """Launch prefill_attn on `device`.  Returns (padded out buffer, the
    device tensors that must come back bit-unchanged, as a dict)."""
    def d(t):
        return None if t is None else t.to(device)

    n = case.T * case.n_head * case.hs
    buf = torch.full((n + PAD,), SENTINEL, dtype=torch.bfloat16,
                     device=device)
    dev = dict(qkv=d(case.qkv), kpool=d(case.kpool), vpool=d(case.vpool),
               kscale=d(case.kscale), vscale=d(case.vscale))
    ops.prefill_attn(buf[:n].view(case.T, case.n_head * case.hs), dev["qkv"],
                     dev["kpool"], dev["vpool"], case.pos0, case.slot,
                     case.layer, case.scale, kscale=dev["kscale"],
                     vscale=dev["vscale"])
    return buf, dev


def check_prefill(case: PrefillCase, ref: PrefillRef, buf, dev, c):
    """(ok, ratio, message) of one run_prefill result."""
    n = case.T * case.n_head * case.hs
    host = buf.detach().cpu()
    ratio = prefill_error_ratio(host[:n], ref.out, ref.A, c)
    if not bool((host[n:].float() == SENTINEL).all()):
        return False, ratio, "the sentinel tail behind out was written"
    for k in ("qkv", "kpool", "vpool", "kscale", "vscale"):
        want = getattr(case, k)
        if want is not None and not torch.equal(dev[k].cpu(), want):
            return False, ratio, f"{k} was modified"
    if not prefill_error_ok(host[:n], ref.out, ref.A, c):
        g = host[:n].to(F64).reshape(ref.out.shape)
        r = (g - ref.out).abs() / prefill_bound(ref.out, ref.A, c)
        t, h, dd = [int(i) for i in
                    torch.unravel_index(torch.nan_to_num(
                        r, nan=math.inf).argmax(), r.shape)]
        return False, ratio, (f"row {t} head {h} dim {dd}: got "
                              f"{float(g[t, h, dd]):.6g} ref "
                              f"{float(ref.out[t, h, dd]):.6g} err/bound "
                              f"{ratio:.3g}")
    return True, ratio, ""


# ---------------------------------------------------------------------------
# prefill_attn case matrices: name -> make_prefill_case kwargs
def _kv(spec):
    out = {}
    for kv8 in (False, True):
        for name, kw in spec:
            full = f"{name}-{'fp8' if kv8 else 'bf16'}"
            out[full] = dict(name=full, kv8=kv8, **kw)
    return out


def prefill_matrix() -> Dict[str, dict]:
    spec = []
    for qpk in (1, 2, 3, 4, 5, 7, 8):
        spec.append((f"wave-qpk{qpk}", dict(qpk=qpk, hs=64, T=40, pos0=5,
                                            family="wave mapping")))
    for T in (1, 15, 16, 17, 31, 32, 33):
        spec.append((f"qtile-T{T}", dict(qpk=4, hs=128, T=T, pos0=0,
                                         family="q-tile edges")))
    for S in (63, 64, 65, 127, 128, 129, 193):
        for T in (1, 17):
            spec.append((f"chunk-S{S}-T{T}",
                         dict(qpk=4, hs=128, T=T, pos0=S - T,
                              family="chunk edges")))
    for pos0 in (47, 48, 63, 64):
        spec.append((f"full-pos{pos0}", dict(qpk=4, hs=128, T=17, pos0=pos0,
                                             family="full flip")))
    spec += [
        ("multi-qpk1-T130-pos0", dict(qpk=1, hs=128, T=130, pos0=0,
                                      family="multi-tile blocks")),
        ("multi-qpk1-T130-pos60", dict(qpk=1, hs=128, T=130, pos0=60,
                                       family="multi-tile blocks")),
        ("multi-qpk2-T49-pos3", dict(qpk=2, hs=128, T=49, pos0=3,
                                     family="multi-tile blocks")),
        ("hs256-qpk4-T33-pos70", dict(qpk=4, hs=256, T=33, pos0=70,
                                      family="head size")),
        ("hs64-qpk1-T33", dict(qpk=1, hs=64, T=33, pos0=0,
                               family="head size")),
    ]
    for mode in ("ascending", "descending", "outlier"):
        spec.append((f"mode-{mode}", dict(qpk=4, hs=128, T=60, pos0=240,
                                          mode=mode,
                                          family="score profiles")))
    return _kv(spec)


# MDI_PREFILL_V1=1: one case per family, both KV modes.  qpk 1 at T 130
# puts tiles 0..3 (1..4 key tiles at pos0 0) in one block: waves of one
# block loop a different number of times.
V1_NAMES = [n + s for n in ("wave-qpk3", "qtile-T17", "chunk-S65-T17",
                            "full-pos48", "multi-qpk1-T130-pos0",
                            "hs256-qpk4-T33-pos70", "mode-ascending")
            for s in ("-bf16", "-fp8")]


def kch32_matrix() -> Dict[str, dict]:
    """MDI_PREFILL_KCH=32: the chunk-edge family around 32 and 64."""
    spec = []
    for S in (31, 32, 33, 63, 64, 65):
        for T in (1, 17):
            spec.append((f"kch32-S{S}-T{T}",
                         dict(qpk=4, hs=128, T=T, pos0=S - T,
                              family="chunk edges KCH 32")))
    return _kv(spec)


def reduced_matrix() -> Dict[str, dict]:
    """The CPU matrix: n_kv 2, hs 64/128, bf16 and fp8."""
    spec = []
    for hs in (64, 128):
        spec += [
            (f"r-wave-h{hs}", dict(qpk=3, hs=hs, T=40, pos0=5)),
            (f"r-qtile-h{hs}", dict(qpk=4, hs=hs, T=17, pos0=0)),
            (f"r-chunk-h{hs}", dict(qpk=4, hs=hs, T=17, pos0=48)),
            (f"r-full-h{hs}", dict(qpk=2, hs=hs, T=17, pos0=64)),
            (f"r-multi-h{hs}", dict(qpk=1, hs=hs, T=130, pos0=60)),
            (f"r-T1-h{hs}", dict(qpk=4, hs=hs, T=1, pos0=128)),
        ]
        for mode in ("ascending", "descending", "outlier"):
            spec.append((f"r-{mode}-h{hs}", dict(qpk=4, hs=hs, T=60,
                                                 pos0=240, mode=mode)))
    return _kv(spec)


# ---------------------------------------------------------------------------
# rope_prefill_append
ROPE_COND = 2.0 ** -13   # |result| >= this * (|x1 c| + |x2 s|), see below


def rope_append_reference(qkv, cos, sin, pos0, n_kv, hs, dtype=F64):
    """fp64 [T, n_kv, qpk+2, hs]: q rows and the k row roped at
    cos[pos0 + t], v and dims >= rope_ne as given; unrounded."""
    T = qkv.shape[0]
    x = qkv.reshape(T, n_kv, -1, hs).to(dtype)
    out = x.clone()
    for t in range(T):
        out[t, :, :-1] = rope_rows(x[t, :, :-1], cos[pos0 + t],
                                   sin[pos0 + t])
    return out


def rope_condition(qkv, cos, sin, pos0, n_kv, hs) -> float:
    """min |r| / (|x1 c| + |x2 s|) over the roped elements.  The kernel
    ropes in fp32; where the two products cancel to below 2^-13 of their
    size, its 2^-24 product roundings reach a bf16 ulp of the result and
    "within one ulp" would no longer follow from the formats."""
    ne = cos.shape[1] if cos.dim() > 1 else 0
    if ne == 0:
        return math.inf
    T = qkv.shape[0]
    x = qkv.reshape(T, n_kv, -1, hs).to(F64)[:, :, :-1, :ne]
    half = ne // 2
    c = cos[pos0:pos0 + T].to(F64)[:, None, None, :]
    s = sin[pos0:pos0 + T].to(F64)[:, None, None, :]
    rot = torch.cat([-x[..., half:], x[..., :half]], dim=-1)
    r = x * c + rot * s
    mag = (x * c).abs() + (rot * s).abs()
    live = mag > 0
    if not bool(live.any()):
        return math.inf
    return float((r.abs()[live] / mag[live]).min())


@dataclass
class RopeCase:
    name: str
    qpk: int
    hs: int
    rope_ne: int
    T: int
    pos0: int
    kv8: bool
    n_kv: int
    max_seq: int
    slot: int
    layer: int
    zero_v: Tuple[int, int]      # (t, g) of the all-zero v row
    qkv: torch.Tensor            # bf16 [T, qkv_dim], raw
    cos: torch.Tensor
    sin: torch.Tensor


ROPE_SHAPES = [(4, 128, 128), (1, 64, 64), (7, 64, 16), (2, 256, 64),
               (3, 64, 0)]
ROPE_MAX_SEQ = 64


def rope_matrix() -> Dict[str, dict]:
    out = {}
    for qpk, hs, ne in ROPE_SHAPES:
        for T in (1, 5):
            for pos0 in (0, 37, ROPE_MAX_SEQ - T):
                for kv8 in (False, True):
                    name = (f"rope-q{qpk}-h{hs}-ne{ne}-T{T}-p{pos0}-"
                            f"{'fp8' if kv8 else 'bf16'}")
                    out[name] = dict(name=name, qpk=qpk, hs=hs, rope_ne=ne,
                                     T=T, pos0=pos0, kv8=kv8)
    return out


def make_rope_case(name, qpk, hs, rope_ne, T, pos0, kv8, n_kv=N_KV,
                   max_seq=ROPE_MAX_SEQ, slot=SLOT, layer=LAYER) -> RopeCase:
    """Raw qkv N(0,1) with one all-zero v row.  The seed advances until
    the reference alone says that no roped element is a near-total
    cancellation (rope_condition >= 2^-13)."""
    cos, sin = rope_tables(max_seq, rope_ne)
    seed = zlib.crc32(name.encode()) & 0x7FFFFFF
    for bump in range(64):
        gen = torch.Generator().manual_seed(seed + bump)
        qkv = torch.randn(T, n_kv * (qpk + 2) * hs, generator=gen).to(
            torch.bfloat16)
        zt, zg = T - 1, n_kv - 1
        qkv.view(T, n_kv, qpk + 2, hs)[zt, zg, qpk + 1] = 0
        if rope_condition(qkv, cos, sin, pos0, n_kv, hs) >= ROPE_COND:
            return RopeCase(name, qpk, hs, rope_ne, T, pos0, kv8, n_kv,
                            max_seq, slot, layer, (zt, zg), qkv, cos, sin)
    raise AssertionError(f"no well-conditioned seed for {name}")


# ---------------------------------------------------------------------------
# mtile_gemm
MTILE_KC = {16: 512, 32: 512, 64: 256, 128: 128}


@dataclass(frozen=True)
class MtileCase:
    B: int
    K: int
    M: int
    bias: bool
    res: bool

    @property
    def id(self):
        return (f"mtile-B{self.B}-K{self.K}-M{self.M}"
                + ("-bias" if self.bias else "") + ("-res" if self.res else ""))

    @property
    def KC(self):
        return MTILE_KC[self.B]


def mtile_matrix() -> List[MtileCase]:
    return [MtileCase(B, n * MTILE_KC[B], M, bias, res)
            for B in (16, 32, 64, 128) for n in (2, 4, 6)
            for M in (16, 48, 272)
            for bias in (False, True) for res in (False, True)]


def mtile_reduced() -> List[MtileCase]:
    """The CPU subset: every B at its deepest K, M 48, bias and res."""
    return [MtileCase(B, 6 * MTILE_KC[B], 48, True, True)
            for B in (16, 32, 64, 128)]


@dataclass
class MtileInputs:
    X: torch.Tensor               # bf16 [B, K]
    W: torch.Tensor               # bf16 [M, K]
    bias: Optional[torch.Tensor]  # bf16 [M]
    res: Optional[torch.Tensor]   # bf16 [B, M]


def make_mtile_inputs(case: MtileCase) -> MtileInputs:
    """Independent N(0,1) rows (no two X rows or W rows are close: their
    outputs differ by about sqrt(2K) sigma, far outside the bound), bias
    and res of the magnitude of the dot products."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode())
                                        & 0x7FFFFFF)
    X = (torch.randn(case.B, case.K, generator=gen) * 0.5).to(torch.bfloat16)
    W = (torch.randn(case.M, case.K, generator=gen)
         / case.K ** 0.5).to(torch.bfloat16)
    mag = float((X.to(F64) @ W.to(F64).t()).abs().median())
    bias = ((torch.randn(case.M, generator=gen) * mag).to(torch.bfloat16)
            if case.bias else None)
    res = ((torch.randn(case.B, case.M, generator=gen) * mag).to(
        torch.bfloat16) if case.res else None)
    return MtileInputs(X, W, bias, res)


def mtile_reference(inp: MtileInputs) -> G.Ref:
    X, W = inp.X.to(F64), inp.W.to(F64)
    ref = X @ W.t()
    A = X.abs() @ W.abs().t()
    add = torch.zeros_like(ref)
    if inp.bias is not None:
        ref = ref + inp.bias.to(F64)[None]
        add = add + inp.bias.to(F64).abs()[None]
    if inp.res is not None:
        ref = ref + inp.res.to(F64)
        add = add + inp.res.to(F64).abs()
    return G.Ref(ref, A, G.ADD_UNIT * add, 0)


def mtile_error_ok(got, r: G.Ref, K):
    """(ok, worst ratio) under gemv_bound; got [B, M]."""
    ok, ratio = G.gemv_error_ok(got.reshape(r.ref.shape), r.ref, r.A, K,
                                r.extra)
    return ok, float(ratio.max())
