"""Shared decode-attention reference, error metric and input generator.

Plain helper module (like helpers.py): the CPU test of the metric, the GPU
matrix and the fused attention+projection test all import it.

The reference is vectorised torch in float64 and device-agnostic.  It
mirrors the kernels only at their documented bf16 rounding points (read off
attn_decode_block_kernel):

  * roped q is rounded to bf16;
  * the roped current k is rounded to bf16, and that row is what is appended;
  * fp8 KV: pool K is e4m3fn(byte) * kscale[row] (an fp32 multiply, as in
    the kernel), rounded to bf16 before QK^T;
  * pool V is dequantised without rounding;
  * scores, softmax and PV are exact (fp64) and the output is not rounded.

Error bound (attn_error_ok):  |got - ref| <= 2^-8 |ref| + 2^-9 A  with
A[h,d] = sum_s p[h,s] |V[s,d]|.  The first term is the bf16 rounding of the
result (the only rounding the kernel applies to its output); the second
allows for fp32 accumulation, __expf and rare 1-ulp bf16 disagreements in
the roped q/k, relative to the condition number of a softmax-weighted sum.
Both constants are derived from the number formats, not tuned.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

REL_TERM = 2.0 ** -8    # bf16 rounding of the result
COND_TERM = 2.0 ** -9   # accumulation/exp error relative to sum p|V|

BF16_GARBAGE = 3.0e4    # rows >= S of the live slot: large, finite
FP8_GARBAGE_BYTE = 0x7E  # e4m3fn 448.0 (0x7F would be NaN)
FP8_GARBAGE_SCALE = 100.0

W_MIN, W_MAX = 0.02, 0.5  # required softmax weight of every probe key


# ---------------------------------------------------------------------------
# number formats
def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 ulps between two bf16 tensors (monotonic bit map)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def fp8_decode(byte_t: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn bytes -> float32 values (exact)."""
    return byte_t.contiguous().view(torch.float8_e4m3fn).to(torch.float32)


def fp8_quant_rows(x: torch.Tensor):
    """Per-row absmax/448 e4m3fn quantisation: (uint8 bytes, fp32 scales)."""
    xf = x.to(torch.float32)
    s = xf.abs().amax(dim=-1).clamp_min(1e-12) / 448.0
    q = (xf / s[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s


# ---------------------------------------------------------------------------
# reference building blocks (the CPU mutation test recombines them)
def rope_rows(x: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor,
              inverse: bool = False) -> torch.Tensor:
    """Rotate-half rope on the first ne = cos_row.numel() dims of x[..., hs].
    inverse=True rotates back (rope with -sin)."""
    ne = cos_row.numel()
    if ne == 0:
        return x.clone()
    half = ne // 2
    c = cos_row.to(x.dtype)
    s = sin_row.to(x.dtype)
    if inverse:
        s = -s
    xr = x[..., :ne]
    rot = torch.cat([-xr[..., half:], xr[..., :half]], dim=-1)
    out = x.clone()
    out[..., :ne] = xr * c + rot * s
    return out


def split_qkv(qkv: torch.Tensor, n_kv: int, hs: int, dtype=torch.float64):
    """Raw interleaved qkv [n_kv, qpk+2, hs] -> (q [n_kv,qpk,hs], k, v)."""
    grp = qkv.reshape(n_kv, -1, hs).to(dtype)
    qpk = grp.shape[1] - 2
    return grp[:, :qpk], grp[:, qpk], grp[:, qpk + 1]


def pool_rows(pool, scale_t, slot, layer, n_rows, dtype, round_bf16):
    """Rows [0, n_rows) of every kv head of (slot, layer), dequantised."""
    rows = pool[slot, layer, :, :n_rows]
    if scale_t is None:
        return rows.to(dtype)
    sc = scale_t[slot, layer, :, :n_rows].to(torch.float32)
    val = fp8_decode(rows)
    if round_bf16:  # K: fp32 multiply, then bf16 (the MFMA operand)
        return (val * sc[..., None]).to(torch.bfloat16).to(dtype)
    return val.to(dtype) * sc[..., None].to(dtype)


@dataclass
class AttnInputs:
    q: torch.Tensor      # [n_kv, qpk, hs] roped, bf16-rounded
    K: torch.Tensor      # [n_kv, S, hs]; row S-1 is the current token's
    V: torch.Tensor      # [n_kv, S, hs]
    k_row: torch.Tensor  # [n_kv, hs] expected appended K (bf16-rounded)
    v_row: torch.Tensor  # [n_kv, hs] expected appended V (raw)


def gather_inputs(qkv, kpool, vpool, cos, sin, pos, slot, layer,
                  kscale=None, vscale=None, dtype=torch.float64) -> AttnInputs:
    n_kv, hs = kpool.shape[2], kpool.shape[4]
    q_raw, k_raw, v_raw = split_qkv(qkv, n_kv, hs, dtype)
    c, s = cos[pos], sin[pos]
    q = bf16_round(rope_rows(q_raw, c, s))
    k_row = bf16_round(rope_rows(k_raw, c, s))
    K = torch.cat([pool_rows(kpool, kscale, slot, layer, pos, dtype, True),
                   k_row[:, None]], dim=1)
    V = torch.cat([pool_rows(vpool, vscale, slot, layer, pos, dtype, False),
                   v_raw[:, None]], dim=1)
    return AttnInputs(q, K, V, k_row, v_raw.clone())


def attend(q, K, V, scale):
    """Exact softmax attention per kv group: (out, A, p), heads flattened."""
    n_kv, qpk, hs = q.shape
    sc = torch.einsum("gjd,gsd->gjs", q, K) * scale
    p = torch.softmax(sc, dim=-1)
    out = torch.einsum("gjs,gsd->gjd", p, V)
    A = torch.einsum("gjs,gsd->gjd", p, V.abs())
    return (out.reshape(n_kv * qpk, hs), A.reshape(n_kv * qpk, hs),
            p.reshape(n_kv * qpk, -1))


@dataclass
class AttnRef:
    out: torch.Tensor    # [B?, n_head, hs]
    A: torch.Tensor      # [B?, n_head, hs]
    p: object            # [n_head, S], or a list of those when batched
    k_row: torch.Tensor  # [B?, n_kv, hs]
    v_row: torch.Tensor  # [B?, n_kv, hs]


def attn_decode_reference(qkv, kpool, vpool, cos, sin, pos, slot, layer,
                          scale, kscale=None, vscale=None,
                          dtype=torch.float64) -> AttnRef:
    """pos/slot: ints (single sample, qkv [qkv_dim]) or sequences (batched,
    qkv [B, qkv_dim]; every result gets a leading batch dimension)."""
    if isinstance(pos, int):
        inp = gather_inputs(qkv, kpool, vpool, cos, sin, pos, slot, layer,
                            kscale, vscale, dtype)
        out, A, p = attend(inp.q, inp.K, inp.V, scale)
        return AttnRef(out, A, p, inp.k_row, inp.v_row)
    per = [attn_decode_reference(qkv[b], kpool, vpool, cos, sin, int(pos[b]),
                                 int(slot[b]), layer, scale, kscale, vscale,
                                 dtype) for b in range(len(pos))]
    return AttnRef(torch.stack([r.out for r in per]),
                   torch.stack([r.A for r in per]), [r.p for r in per],
                   torch.stack([r.k_row for r in per]),
                   torch.stack([r.v_row for r in per]))


# ---------------------------------------------------------------------------
# metric
def attn_error_bound(ref, A):
    return REL_TERM * ref.abs() + COND_TERM * A


def attn_error_ratio(got, ref, A) -> float:
    """max |got - ref| / bound (inf for a non-finite output)."""
    assert got.dtype == torch.bfloat16, "the kernel output is bf16"
    g = got.to(ref.dtype).reshape(ref.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float(((g - ref).abs() / attn_error_bound(ref, A)).max())


def attn_error_ok(got, ref, A) -> bool:
    """|got - ref| <= 2^-8 |ref| + 2^-9 A elementwise; got is bf16."""
    assert got.dtype == torch.bfloat16, "the kernel output is bf16"
    g = got.to(ref.dtype).reshape(ref.shape)
    return bool(((g - ref).abs() <= attn_error_bound(ref, A)).all())


# ---------------------------------------------------------------------------
# input generator with planted heavy keys
def keys_per_chunk(S: int, n_chunks: int) -> int:
    return ((S + n_chunks - 1) // n_chunks + 15) & ~15


def pick_probes(S: int, candidates: Sequence[int]) -> List[int]:
    """Distinct candidates inside [0, S).  S == 1 has no probe: its only
    key carries weight 1, outside the required [0.02, 0.5]."""
    if S < 2:
        return []
    return sorted({int(c) for c in candidates if 0 <= c < S})


def rope_tables(max_seq: int, ne: int, base: float = 10000.0):
    """fp32 cos/sin [max_seq, ne], rotate-half layout (theta duplicated)."""
    theta = 1.0 / (base ** (torch.arange(0, ne, 2).float() / max(ne, 1)))
    ang = torch.outer(torch.arange(max_seq).float(), theta)
    ang = torch.cat([ang, ang], dim=1)
    return torch.cos(ang).contiguous(), torch.sin(ang).contiguous()


@dataclass
class AttnCase:
    qpk: int
    n_kv: int
    hs: int
    max_seq: int
    layer: int
    scale: float
    batched: bool
    pos: List[int]
    slot: List[int]
    probes: List[List[int]]
    qkv: torch.Tensor           # bf16 [B, qkv_dim]
    kpool: torch.Tensor         # bf16 or uint8 [slots, layers, n_kv, seq, hs]
    vpool: torch.Tensor
    kscale: Optional[torch.Tensor]
    vscale: Optional[torch.Tensor]
    cos: torch.Tensor
    sin: torch.Tensor
    extra: dict = field(default_factory=dict)

    @property
    def n_head(self):
        return self.n_kv * self.qpk

    @property
    def kv8(self):
        return self.kscale is not None

    def reference(self, dtype=torch.float64, **over) -> AttnRef:
        a = dict(qkv=self.qkv if self.batched else self.qkv[0],
                 kpool=self.kpool, vpool=self.vpool, cos=self.cos,
                 sin=self.sin,
                 pos=self.pos if self.batched else self.pos[0],
                 slot=self.slot if self.batched else self.slot[0],
                 layer=self.layer, scale=self.scale, kscale=self.kscale,
                 vscale=self.vscale, dtype=dtype)
        a.update(over)
        return attn_decode_reference(**a)

    def probe_weights(self, ref: AttnRef):
        """[(sample, kv group, key, best weight over the group's heads)]"""
        res = []
        for b, plist in enumerate(self.probes):
            p = ref.p[b] if self.batched else ref.p
            for s in plist:
                for g in range(self.n_kv):
                    w = p[g * self.qpk:(g + 1) * self.qpk, s]
                    ok = w[(w >= W_MIN) & (w <= W_MAX)]
                    res.append((b, g, s, float(ok.max()) if ok.numel()
                                else float(w.max())))
        return res

    def probes_ok(self, ref: AttnRef) -> bool:
        """The precondition of every comparison: each probe key carries
        weight in [0.02, 0.5] in at least one query head of its group."""
        return all(W_MIN <= w <= W_MAX
                   for _, _, _, w in self.probe_weights(ref))


def _write_row(pool, scale_t, idx, row):
    if scale_t is None:
        pool[idx] = row.to(torch.bfloat16)
    else:
        q, s = fp8_quant_rows(row)
        pool[idx] = q
        scale_t[idx] = s


def make_case(qpk, n_kv, hs, pos, max_seq, rope_ne=None, probes=(),
              mode="random", kv8=False, slot=1, layer=1, n_layers=2,
              n_slots=3, scale=None, seed=0) -> AttnCase:
    """Inputs for one attn_decode call.  pos/slot/probes are an int, an int
    and a list of key indices (single sample), or lists of those (batched).

    Pools are N(0,1) everywhere (other slots and layers hold different
    data), rows >= pos of each live slot hold large finite garbage, and
    every probe key is planted as K[probe] = t * q_j / (scale |q_j|^2) with
    q_j the bf16 roped q of head j = probe_index % qpk, i.e. score t on
    that head.  t starts at ln(S) + 1 and is refined on the reference
    itself until the probe's weight is 0.5 / (probes on that head + 1).
    A probe at pos is planted through the raw k (inverse rope of the row).

    mode shapes the non-probe keys of a single-sample case:
      "ascending" / "descending": scores ramp over 0..12 with the key index,
      so the running max moves on every tile (or never after the first);
      "outlier": one key at about -30 and one at about +12.
    """
    batched = not isinstance(pos, int)
    pos_l = list(pos) if batched else [pos]
    slot_l = list(slot) if batched else [slot]
    probes_l = [list(p) for p in probes] if batched else [list(probes)]
    B = len(pos_l)
    rope_ne = hs if rope_ne is None else rope_ne
    scale = 1.0 / math.sqrt(hs) if scale is None else scale
    assert mode == "random" or not batched
    assert len(set(slot_l)) == B and max(pos_l) < max_seq

    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, n_kv * (qpk + 2) * hs, generator=gen).to(
        torch.bfloat16)
    shape = (n_slots, n_layers, n_kv, max_seq, hs)
    kf = torch.randn(shape, generator=gen)
    vf = torch.randn(shape, generator=gen)
    cos, sin = rope_tables(max_seq, rope_ne)

    q_hat = []  # per sample: roped bf16 q, fp64 [n_kv, qpk, hs]
    for b in range(B):
        q_raw, _, _ = split_qkv(qkv[b], n_kv, hs)
        q_hat.append(bf16_round(rope_rows(q_raw, cos[pos_l[b]],
                                          sin[pos_l[b]])))

    if mode != "random":
        # non-probe keys along u = mean roped q of the group: key s scores
        # about ramp[s] on every head of the group, plus a little noise
        P = pos_l[0]
        u = q_hat[0].mean(dim=1)                              # [n_kv, hs]
        per_unit = scale * torch.einsum("gjd,gd->gj", q_hat[0], u).mean(1)
        if mode == "outlier":
            ramp = torch.zeros(P, dtype=torch.float64)
            noise = 1.0
            if P >= 8:
                ramp[P // 3] = -30.0
                ramp[(2 * P) // 3] = 12.0
        else:
            ramp = torch.linspace(0.0, 12.0, max(P, 1),
                                  dtype=torch.float64)[:P]
            if mode == "descending":
                ramp = ramp.flip(0)
            noise = 0.25
        rows = (ramp[None, :, None] / per_unit[:, None, None]) * u[:, None]
        kf[slot_l[0], layer, :, :P] = (
            noise * kf[slot_l[0], layer, :, :P] + rows.float())

    if kv8:
        kpool, kscale = fp8_quant_rows(kf)
        vpool, vscale = fp8_quant_rows(vf)
    else:
        kpool, vpool = kf.to(torch.bfloat16), vf.to(torch.bfloat16)
        kscale = vscale = None
    del kf, vf
    for b in range(B):  # garbage at and past pos, in every layer
        sl = (slot_l[b], slice(None), slice(None), slice(pos_l[b], None))
        if kv8:
            kpool[sl] = FP8_GARBAGE_BYTE
            vpool[sl] = FP8_GARBAGE_BYTE
            kscale[sl] = FP8_GARBAGE_SCALE
            vscale[sl] = FP8_GARBAGE_SCALE
        else:
            kpool[sl] = BF16_GARBAGE
            vpool[sl] = -BF16_GARBAGE

    case = AttnCase(qpk, n_kv, hs, max_seq, layer, scale, batched, pos_l,
                    slot_l, probes_l, qkv, kpool, vpool, kscale, vscale,
                    cos, sin)

    # ---- plant the probes, refining each target score on the reference ---
    plan = []  # (b, g, key, head j, desired weight)
    for b in range(B):
        on_head = [sum(1 for i in range(len(probes_l[b])) if i % qpk == j)
                   for j in range(qpk)]
        for i, s in enumerate(probes_l[b]):
            assert 0 <= s <= pos_l[b]
            j = i % qpk
            for g in range(n_kv):
                plan.append((b, g, s, j, 0.5 / (on_head[j] + 1)))
    target = [math.log(pos_l[b] + 1) + 1.0 for b, *_ in plan]

    def plant():
        for (b, g, s, j, _), t in zip(plan, target):
            q = q_hat[b][g, j]
            row = t * q / (scale * float(q @ q))
            if s == pos_l[b]:
                raw = rope_rows(row, cos[s], sin[s], inverse=True)
                grp = qkv[b].view(n_kv, qpk + 2, hs)
                grp[g, qpk] = raw.to(torch.bfloat16)
            else:
                _write_row(kpool, kscale, (slot_l[b], layer, g, s), row)

    for _ in range(8 if plan else 0):
        plant()
        ref = case.reference()
        for n, (b, g, s, j, want) in enumerate(plan):
            p = ref.p[b] if batched else ref.p
            w = float(p[g * qpk + j, s].clamp(1e-300, 1 - 1e-12))
            target[n] += math.log(want / (1 - want)) - math.log(w / (1 - w))
    plant()
    return case
