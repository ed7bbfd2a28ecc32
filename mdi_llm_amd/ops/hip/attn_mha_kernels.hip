// MHA attention (q_per_kv == 1) for head sizes the MFMA tile code of
// decode_kernels.hip cannot map: the decode kernels first, the prefill
// kernel (prefill_attn_mha80_kernel) at the end.  A translation unit of its
// own: its inner loops scale long fp32 rows by one scalar, and it is built
// without the packed fp32 instruction forms (setup.py).
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "decode_kernels.h"
#include "device_common.h"

// ---------------------------------------------------------------------------
// MHA decode attention for head sizes that are no multiple of 32 (HS = 80:
// phi-2, StableLM-3B, Pythia-2.8B).  QPK == 1: one query vector per K
// stream, so a 16-column MFMA tile would be 15/16 empty and the tile core
// cannot map 80 dims onto 64 lanes.  This path is VALU only.
//
// A tile is 32 consecutive keys.  Lane l owns key (l >> 1) and dim half
// (l & 1), HS/2 dims: a bf16 half row is HS bytes (80 = five 16-B loads,
// fp8 five 8-B loads) and the 64 lanes cover 32 * HS * 2 contiguous bytes
// of the pool, so a tile is one fully coalesced 5-KB read for K and one for
// V.  The lane keeps its HS/2 q values in registers, takes the half dot
// product, one shfl_xor(1) joins the halves; m, l and alpha are
// wave-uniform.  P*V uses the SAME lane map: the lane multiplies its own V
// half row by the p it already holds and accumulates HS/2 fp32 values for
// its key residue class, so the key loop moves nothing across lanes for
// P*V.  The 32 residue classes are folded once after the loop
// (mha_fold_keys).  The next tile's K and V are loaded before the current
// tile is consumed; one wave per SIMD leaves the registers for that.
//
// mha_wave_core is the one copy of the loop; attn_mha_block_kernel and
// attn_mha_split_kernel differ only in which keys a wave walks and where
// its partial goes.  Partials use attn_decode_kernel's layout, so
// attn_combine_kernel serves both.
// ---------------------------------------------------------------------------
template <int HS, int KV8>
struct MhaTile {
  static constexpr int NV = HS / 16;  // 8-element vectors per half row
  using vec = std::conditional_t<KV8 != 0, i32x2_t, bf16x8_t>;
  vec k[NV], v[NV];
  float ks, vs;  // fp8 row scales
};

// Folds the 32 key residue classes of a wave: in, lane l holds N = HS/2
// partial sums for dims [(l & 1) * N, +N) of key class l >> 1.  Each of
// the first three steps halves what a lane carries (it keeps one half of
// its dims and hands the other to its partner), the last two add whole
// vectors.  Out: every lane holds N/8 sums in o[0 .. N/8); their first dim
// is returned.  Lanes that differ only in bits 1 and 2 hold copies.
template <int N>
DEVINL int mha_fold_keys(float (&o)[N], int lane) {
  static_assert(N % 8 == 0, "three halving steps");
  int d0 = (lane & 1) * N;
#pragma unroll
  for (int st = 0; st < 3; ++st) {
    const int n = N >> (st + 1);  // values kept after this step
    const int off = 32 >> st;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float keep = up ? o[i + n] : o[i];
      const float send = up ? o[i] : o[i + n];
      o[i] = keep + __shfl_xor(send, off, 64);
    }
    if (up) d0 += n;
  }
#pragma unroll
  for (int i = 0; i < N / 8; ++i) {
    o[i] += __shfl_xor(o[i], 4, 64);
    o[i] += __shfl_xor(o[i], 2, 64);
  }
  return d0;
}

// One wave's online softmax over the keys {key_first + i * key_stride + j :
// j < 32} below key_end (key_end <= S).  q_lds holds the roped bf16 q,
// k_cur the roped bf16 current k; the row at pos comes from k_cur and the
// raw v row, never from the pool.  Out: m, l and, after mha_fold_keys, the
// wave's unnormalised output in o.
template <int HS, int KV8>
DEVINL void mha_wave_core(
    float (&o)[HS / 2], float& m_out, float& l_out, const bf16* q_lds,
    const bf16* k_cur, const bf16* __restrict__ vrow_cur,
    const std::conditional_t<KV8 != 0, u8kv, bf16>* __restrict__ kpool,
    const std::conditional_t<KV8 != 0, u8kv, bf16>* __restrict__ vpool,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    size_t cache_base, size_t scl_base, int pos, int key_first,
    int key_stride, int key_end, float scale, int lane) {
  constexpr int N = HS / 2;
  using Tile = MhaTile<HS, KV8>;
  constexpr int NV = Tile::NV;
  const int kl = lane >> 1;
  const int d0 = (lane & 1) * N;

  float q[N];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bf16x8_t qv = *reinterpret_cast<const bf16x8_t*>(q_lds + d0 + 8 * i);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[8 * i + j] = (float)qv[j];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) o[i] = 0.f;
  float m_st = -1e30f, l_st = 0.f;

  // pool rows below pos only: the row at pos is not in the pool yet, and
  // rows past it hold whatever an earlier sample left
  auto load = [&](int key0, Tile& t) {
    const int key = key0 + kl;
    t.ks = 1.f;
    t.vs = 1.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      t.k[i] = typename Tile::vec{};
      t.v[i] = typename Tile::vec{};
    }
    if (key < pos && key < key_end) {
      const size_t off = cache_base + (size_t)key * HS + d0;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        t.k[i] = *reinterpret_cast<const typename Tile::vec*>(kpool + off +
                                                              8 * i);
        t.v[i] = *reinterpret_cast<const typename Tile::vec*>(vpool + off +
                                                              8 * i);
      }
      if constexpr (KV8) {
        t.ks = kscale[scl_base + key];
        t.vs = vscale[scl_base + key];
      }
    }
  };

  Tile cur, nxt;
  load(key_first, cur);
  nxt = cur;
  for (int key0 = key_first; key0 < key_end; key0 += key_stride) {
    if (key0 + key_stride < key_end) load(key0 + key_stride, nxt);
    const int key = key0 + kl;
    const bool is_cur = key == pos;

    float dot = 0.f;
    if (is_cur) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const bf16x8_t kv =
            *reinterpret_cast<const bf16x8_t*>(k_cur + d0 + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += q[8 * i + j] * (float)kv[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        bf16x8_t kv;
        if constexpr (KV8)
          kv = fp8x8_to_bf16(reinterpret_cast<const u8kv*>(&cur.k[i]),
                             cur.ks);
        else
          kv = cur.k[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += q[8 * i + j] * (float)kv[j];
      }
    }
    dot += __shfl_xor(dot, 1, 64);
    const bool valid = key < key_end;
    const float sc = valid ? dot * scale : -1e30f;

    const float m_new = fmaxf(m_st, wave_reduce_max(sc));
    const float alpha = __expf(m_st - m_new);
    m_st = m_new;
    const float p = valid ? __expf(sc - m_new) : 0.f;
    // both lanes of a key hold its p: the wave sum counts every key twice
    l_st = l_st * alpha + 0.5f * wave_reduce_sum(p);

#pragma unroll
    for (int i = 0; i < N; ++i) o[i] *= alpha;
    if (is_cur) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const bf16x8_t vv =
            *reinterpret_cast<const bf16x8_t*>(vrow_cur + d0 + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[8 * i + j] += p * (float)vv[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if constexpr (KV8) {
          fp8x8_fma(&o[8 * i], p, reinterpret_cast<const u8kv*>(&cur.v[i]),
                    cur.vs);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[8 * i + j] += p * (float)cur.v[i][j];
        }
      }
    }
    cur = nxt;
  }
  m_out = m_st;
  l_out = l_st;
}

// Block-local variant (max_seq <= ATTN_BLOCK_MAX_SEQ): grid.x = n_batch *
// n_heads, block = 256; the four waves take key tiles interleaved and
// their partials are combined through LDS.  BATCH as in attn_decode_kernel.
template <int HS, int BATCH, int KV8>
__global__ __launch_bounds__(256) void attn_mha_block_kernel(
    bf16* __restrict__ out, const bf16* __restrict__ qkv,
    void* __restrict__ kpool_v, void* __restrict__ vpool_v,
    float* __restrict__ kscale, float* __restrict__ vscale,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int rope_ne, const int* __restrict__ pos_p,
    const int* __restrict__ slot_p, int layer, int n_layers_pool,
    int n_heads, int max_seq, float scale, int n_batch) {
  static_assert(HS % 16 == 0, "a half row is whole 8-element vectors");
  using kvt = std::conditional_t<KV8 != 0, u8kv, bf16>;
  kvt* kpool = reinterpret_cast<kvt*>(kpool_v);
  kvt* vpool = reinterpret_cast<kvt*>(vpool_v);

  __shared__ __attribute__((aligned(16))) bf16 q_lds[HS];
  __shared__ __attribute__((aligned(16))) bf16 k_cur[HS];
  __shared__ float o_part[ATTN_WAVES][HS];
  __shared__ float ml_part[ATTN_WAVES][2];
  __shared__ unsigned kvmax[2];  // KV8: row absmax bits (k, v)

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int b = BATCH ? (int)blockIdx.x / n_heads : 0;
  const int g = BATCH ? (int)blockIdx.x % n_heads : (int)blockIdx.x;
  if (b >= n_batch) return;

  const int pos = pos_p[b];
  const int S = pos + 1;
  const int slot = slot_p[b];
  if (BATCH) {
    qkv += (size_t)b * n_heads * 3 * HS;
    out += (size_t)b * n_heads * HS;
  }
  const size_t scl_base =
      (((size_t)slot * n_layers_pool + layer) * n_heads + g) *
      (size_t)max_seq;
  const size_t cache_base = scl_base * HS;
  const bf16* qrow = qkv + (size_t)g * 3 * HS;
  const bf16* krow_cur = qrow + HS;
  const bf16* vrow_cur = krow_cur + HS;
  if (KV8 && threadIdx.x < 2) kvmax[threadIdx.x] = 0;

  // rope in fp32, one rounding to bf16
  for (int d = threadIdx.x; d < 2 * HS; d += 256) {
    if (d < HS)
      q_lds[d] = f2b(rope_elem(qrow, d, rope_ne, cos_t, sin_t, pos));
    else
      k_cur[d - HS] =
          f2b(rope_elem(krow_cur, d - HS, rope_ne, cos_t, sin_t, pos));
  }
  __syncthreads();

  // append the current token's k, v (no other block touches this head)
  if constexpr (KV8) {
    if (threadIdx.x < HS) {
      lds_fmax_u(&kvmax[0], fabsf(b2f(k_cur[threadIdx.x])));
      lds_fmax_u(&kvmax[1], fabsf(b2f(vrow_cur[threadIdx.x])));
    }
    __syncthreads();
    const float ks = fmaxf(__uint_as_float(kvmax[0]), 1e-12f) / 448.f;
    const float vs = fmaxf(__uint_as_float(kvmax[1]), 1e-12f) / 448.f;
    if (threadIdx.x < HS) {
      const int d = threadIdx.x;
      kpool[cache_base + (size_t)pos * HS + d] =
          f32_to_fp8(b2f(k_cur[d]) / ks);
      vpool[cache_base + (size_t)pos * HS + d] =
          f32_to_fp8(b2f(vrow_cur[d]) / vs);
    }
    if (threadIdx.x == 0) {
      kscale[scl_base + pos] = ks;
      vscale[scl_base + pos] = vs;
    }
  } else if (threadIdx.x < HS) {
    kpool[cache_base + (size_t)pos * HS + threadIdx.x] = k_cur[threadIdx.x];
    vpool[cache_base + (size_t)pos * HS + threadIdx.x] =
        vrow_cur[threadIdx.x];
  }

  float o[HS / 2], m_st, l_st;
  mha_wave_core<HS, KV8>(o, m_st, l_st, q_lds, k_cur, vrow_cur, kpool, vpool,
                         kscale, vscale, cache_base, scl_base, pos, wave * 32,
                         ATTN_WAVES * 32, S, scale, lane);
  const int d0 = mha_fold_keys(o, lane);
  if ((lane & 6) == 0) {
#pragma unroll
    for (int i = 0; i < HS / 16; ++i) o_part[wave][d0 + i] = o[i];
  }
  if (lane == 0) {
    ml_part[wave][0] = m_st;  // a wave without tiles: m = -1e30, l = 0
    ml_part[wave][1] = l_st;
  }
  __syncthreads();

  if (threadIdx.x < HS) {
    const int d = threadIdx.x;
    float M = -1e30f;
#pragma unroll
    for (int w = 0; w < ATTN_WAVES; ++w) M = fmaxf(M, ml_part[w][0]);
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int w = 0; w < ATTN_WAVES; ++w) {
      const float wgt = __expf(ml_part[w][0] - M);
      den += wgt * ml_part[w][1];
      num += wgt * o_part[w][d];
    }
    out[(size_t)g * HS + d] = f2b(num / den);
  }
}

// Split-S variant: one wave per (head, chunk), chunk rule, early exits,
// append ownership and partial layout as in attn_decode_kernel (n_chunks
// is a multiple of 4, so a block's waves share one (batch, head) and q is
// staged once per block); attn_combine_kernel reduces the partials.
template <int HS, int BATCH, int KV8>
__global__ __launch_bounds__(256) void attn_mha_split_kernel(
    float* __restrict__ part_o, float* __restrict__ part_ml,
    const bf16* __restrict__ qkv, void* __restrict__ kpool_v,
    void* __restrict__ vpool_v, float* __restrict__ kscale,
    float* __restrict__ vscale, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, int rope_ne,
    const int* __restrict__ pos_p, const int* __restrict__ slot_p, int layer,
    int n_layers_pool, int n_heads, int max_seq, int n_chunks, float scale,
    int n_batch) {
  static_assert(HS % 16 == 0, "a half row is whole 8-element vectors");
  using kvt = std::conditional_t<KV8 != 0, u8kv, bf16>;
  kvt* kpool = reinterpret_cast<kvt*>(kpool_v);
  kvt* vpool = reinterpret_cast<kvt*>(vpool_v);

  __shared__ __attribute__((aligned(16))) bf16 q_lds[HS];
  __shared__ __attribute__((aligned(16))) bf16 k_cur[HS];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wg_id = blockIdx.x * ATTN_WAVES + wave;
  const int per_b = n_heads * n_chunks;
  const int b = BATCH ? wg_id / per_b : 0;
  const int rem = BATCH ? wg_id % per_b : wg_id;
  const int g = rem / n_chunks;
  const int chunk = rem % n_chunks;
  if (g >= n_heads || b >= n_batch) return;  // block-uniform

  const int pos = pos_p[b];
  const int S = pos + 1;
  const int slot = slot_p[b];
  const int keys_per_chunk = ((S + n_chunks - 1) / n_chunks + 15) & ~15;
  const int k_begin = chunk * keys_per_chunk;
  const int c0 = chunk - wave;  // block's first chunk (uniform)
  if ((long long)c0 * keys_per_chunk >= (long long)S) return;
  if (BATCH) {
    qkv += (size_t)b * n_heads * 3 * HS;
    part_o += (size_t)b * n_heads * n_chunks * HS;
    part_ml += (size_t)b * n_heads * n_chunks * 2;
  }
  const size_t scl_base =
      (((size_t)slot * n_layers_pool + layer) * n_heads + g) *
      (size_t)max_seq;
  const size_t cache_base = scl_base * HS;
  const bf16* qrow = qkv + (size_t)g * 3 * HS;
  const bf16* krow_cur = qrow + HS;
  const bf16* vrow_cur = krow_cur + HS;

  for (int d = threadIdx.x; d < 2 * HS; d += 256) {
    if (d < HS)
      q_lds[d] = f2b(rope_elem(qrow, d, rope_ne, cos_t, sin_t, pos));
    else
      k_cur[d - HS] =
          f2b(rope_elem(krow_cur, d - HS, rope_ne, cos_t, sin_t, pos));
  }
  __syncthreads();  // the only barrier: waves are independent from here
  if (k_begin >= S) return;  // the combine never reads this chunk's slot

  // exactly one chunk's range contains pos; its wave owns the append
  if (k_begin <= pos && pos < k_begin + keys_per_chunk) {
    if constexpr (KV8) {
      float lk = 0.f, lv = 0.f;
      for (int d = lane; d < HS; d += 64) {
        lk = fmaxf(lk, fabsf(b2f(k_cur[d])));
        lv = fmaxf(lv, fabsf(b2f(vrow_cur[d])));
      }
      const float ks = fmaxf(wave_reduce_max(lk), 1e-12f) / 448.f;
      const float vs = fmaxf(wave_reduce_max(lv), 1e-12f) / 448.f;
      for (int d = lane; d < HS; d += 64) {
        kpool[cache_base + (size_t)pos * HS + d] =
            f32_to_fp8(b2f(k_cur[d]) / ks);
        vpool[cache_base + (size_t)pos * HS + d] =
            f32_to_fp8(b2f(vrow_cur[d]) / vs);
      }
      if (lane == 0) {
        kscale[scl_base + pos] = ks;
        vscale[scl_base + pos] = vs;
      }
    } else {
      for (int d = lane; d < HS; d += 64) {
        kpool[cache_base + (size_t)pos * HS + d] = k_cur[d];
        vpool[cache_base + (size_t)pos * HS + d] = vrow_cur[d];
      }
    }
  }

  float o[HS / 2], m_st, l_st;
  mha_wave_core<HS, KV8>(o, m_st, l_st, q_lds, k_cur, vrow_cur, kpool, vpool,
                         kscale, vscale, cache_base, scl_base, pos, k_begin,
                         32, min(k_begin + keys_per_chunk, S), scale, lane);
  const int d0 = mha_fold_keys(o, lane);
  if ((lane & 6) == 0) {
    float* op = part_o + ((size_t)g * n_chunks + chunk) * HS + d0;
#pragma unroll
    for (int i = 0; i < HS / 16; ++i) op[i] = o[i];
  }
  if (lane == 0) {
    part_ml[((size_t)g * n_chunks + chunk) * 2 + 0] = m_st;
    part_ml[((size_t)g * n_chunks + chunk) * 2 + 1] = l_st;
  }
}

template <int HS, int BATCH, int KV8>
static void launch_attn_mha(const AttnArgs& a, float* part_o, float* part_ml,
                            int n_chunks, int n_batch, bool split,
                            hipStream_t stream) {
  const int nb = BATCH ? n_batch : 1;
  if (split) {
    const int blocks = a.n_kv_heads * n_chunks * nb / ATTN_WAVES;
    hipLaunchKernelGGL((attn_mha_split_kernel<HS, BATCH, KV8>), dim3(blocks),
                       dim3(256), 0, stream, part_o, part_ml,
                       (const bf16*)a.qkv, a.kpool, a.vpool, a.kscale,
                       a.vscale, a.cos_t, a.sin_t, a.rope_ne, a.pos, a.slot,
                       a.layer, a.n_layers_pool, a.n_kv_heads, a.max_seq,
                       n_chunks, a.scale, nb);
  } else {
    hipLaunchKernelGGL((attn_mha_block_kernel<HS, BATCH, KV8>),
                       dim3(nb * a.n_kv_heads), dim3(256), 0, stream,
                       (bf16*)a.out, (const bf16*)a.qkv, a.kpool, a.vpool,
                       a.kscale, a.vscale, a.cos_t, a.sin_t, a.rope_ne, a.pos,
                       a.slot, a.layer, a.n_layers_pool, a.n_kv_heads,
                       a.max_seq, a.scale, nb);
  }
}

void launch_attn_mha80(const AttnArgs& a, float* part_o, float* part_ml,
                       int n_chunks, int n_batch, bool split,
                       hipStream_t stream) {
  const bool kv8 = a.kscale != nullptr;
  if (n_batch > 0) {
    if (kv8)
      launch_attn_mha<80, 1, 1>(a, part_o, part_ml, n_chunks, n_batch, split,
                                stream);
    else
      launch_attn_mha<80, 1, 0>(a, part_o, part_ml, n_chunks, n_batch, split,
                                stream);
  } else {
    if (kv8)
      launch_attn_mha<80, 0, 1>(a, part_o, part_ml, n_chunks, n_batch, split,
                                stream);
    else
      launch_attn_mha<80, 0, 0>(a, part_o, part_ml, n_chunks, n_batch, split,
                                stream);
  }
}

// ---------------------------------------------------------------------------
// Prefill flash attention for head size 80, MHA (causal, online softmax,
// QK^T and P.V on MFMA 16x16x32 bf16).  Dispatched by launch_prefill_attn
// for head_size == 80 && qpk == 1; the 64/128/256 template of
// decode_kernels.hip is left alone (its loops run HS/32 times).
//
// Work split: one 256-thread block = one head x 4 consecutive 16-row q tiles
// (64 query rows), one q tile per wave.  Blocks are numbered so that the
// q-tile groups with the longest key range start first.  The block stages
// keys up to the causal bound of its last tile (k_last_blk); a wave stops at
// the bound of its own tile (k_last_w).  A wave whose tile lies past T keeps
// staging and meeting the barriers but does no maths.
//
// Data movement, per 64-key chunk:
//   * global -> registers one chunk AHEAD: the loads of chunk ch+1 are
//     issued right after the staging barrier of chunk ch and are consumed
//     after its maths, so their latency hides behind the MFMA/softmax work
//     (28 VGPRs bf16, 21 fp8).  A row is 160 B (80 B fp8): ten 16-B (8-B)
//     loads, always aligned; a wave reads 6.4 whole rows per instruction.
//   * registers -> LDS: K row-major, V transposed.  fp8 rows are dequantised
//     here through fp8x8_to_bf16, so K and V are rounded to bf16 exactly as
//     in prefill_attn_mfma_kernel (tests/prefill_reference.py).  A thread
//     transposes TWO adjacent keys of one 8-dim group, so V^T is written with
//     8 four-byte stores per key pair instead of 16 two-byte ones.
//   * q never touches LDS: the MFMA B fragment of a q tile (lane = row
//     arow, dims c*32 + sub*8 .. +7) is loop invariant and is loaded once
//     from global into 12 VGPRs.
//
// QK^T pads the depth from 80 to 96: three 16x16x32 steps per 16-key tile.
// The pad is zero on both sides: K columns 80..95 are written once before
// the chunk loop (staging never touches them) and the q fragment of dims
// 80..95 (c == 2, sub >= 2) is the zero vector.  P.V needs no pad: 80 dims
// are five 16-dim output tiles (o_pv[5]); P goes through a per-wave LDS
// tile, rounded to bf16 (four keys packed into one 8-B store), while l sums
// the unrounded p.
//
// LDS layout (39,936 B).  A ds_read_b128 is served in four groups of 16
// lanes, 16 B each, over 64 banks: a group is conflict-free when its lanes
// hit 16 distinct 16-B slots mod 16.  With arow = lane & 15, sub = lane >> 4
// the groups are {sub 0: arow 0-3,12-15; sub 1: arow 4-11}, {sub 0: arow
// 4-11; sub 1: arow 0-3,12-15} and the same two with sub 2/3
// (profiles/prefill_attn_r02.md).  All strides below are in 16-B slots.
//   * k_lds[64][112]: stride 14, slot = 14 row + 4 c + sub.  14 row mod 16
//     over arow 0-3,12-15 is {0,14,12,10,8,6,4,2}: the eight even residues;
//     over arow 4-11 it is the same set, and the partner sub adds 1: the
//     eight odd residues.  16 tile rows are 224 slots = 0 mod 16, so every
//     key tile t4 and every c sees the same picture.  (96 columns unpadded,
//     stride 12, give 12 row mod 16 = four residues only.)
//   * p_t[4][16][80]: stride 10, slot = 10 arow + 4 k2 + sub: 10 arow mod 16
//     over arow 0-3,12-15 is {0,10,4,14,8,2,12,6}, evens again, and the
//     same argument holds.  The 8-B P stores of a wave (128 dwords) land
//     two per bank, the floor.
//   * v_t[80][96]: stride 12 with the key-unit XOR x = (3 (row >> 3)) & 7,
//     slot = 12 row + ((4 k2 + sub) ^ x).  The XOR is there for the
//     transposed stores: rows 8 apart are 384 dwords = 0 mod 32 apart, so
//     the ten dim groups of one key pair would share a bank; x takes all
//     eight values over row >> 3 = 0..7 and moves them 4 dwords apart
//     (2-way left: groups 8, 9 alias 0, 1).  For the reads, stride 12 is
//     the one between 9 and 13 at which some odd multiplier keeps every
//     group conflict-free under the XOR, for all five dim tiles and both
//     k2 (checked exhaustively; stride 10 or 11 with x = row >> 3, the
//     swizzle of the 64/128/256 kernel, leaves 2-way reads).
//
// Softmax state (m, l) is in registers, replicated over the four subs and
// exchanged by shuffles; scores carry scale * log2(e), so p is one v_exp_f32.
// Two barriers per chunk.  `full` (wave-uniform) skips the mask compares of
// chunks that lie wholly below the tile's first row.
// ---------------------------------------------------------------------------
#define PF80_KCH 64    // keys per chunk
#define PF80_KSTR 112  // k_lds row stride (bf16): 96 columns + 16
#define PF80_VSTR 96   // v_t row stride
#define PF80_PSTR 80   // p_t row stride

using bf16x2_t = __attribute__((ext_vector_type(2))) __bf16;
using bf16x4_t = __attribute__((ext_vector_type(4))) __bf16;

// one thread's share of a chunk between the global load and the LDS store
template <int KV8>
struct Pf80Regs {
  using raw_t = std::conditional_t<KV8 != 0, int2, int4>;  // 8 elements
  raw_t k[3];
  raw_t v[2][2];
  float ks[3];  // fp8 row scales
  float vs[2][2];
};

template <int KV8>
DEVINL bf16x8_t pf80_to_bf16(const typename Pf80Regs<KV8>::raw_t& raw,
                             float scl) {
  if constexpr (KV8)
    return fp8x8_to_bf16(reinterpret_cast<const u8kv*>(&raw), scl);
  else
    return *reinterpret_cast<const bf16x8_t*>(&raw);
}

template <int KV8>
__global__ __launch_bounds__(256) void prefill_attn_mha80_kernel(
    bf16* __restrict__ out,        // [T, n_head*80]
    const bf16* __restrict__ qkv,  // [T, n_head*240], q already roped
    const void* __restrict__ kpool_v, const void* __restrict__ vpool_v,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    int pos0, int slot, int layer, int n_layers_pool, int n_head, int max_seq,
    int T, float scale_log2e, int n_qtg) {
  constexpr int HS = 80;
  constexpr int U = HS / 8;  // 16-B (bf16) units per row
  using kvt = std::conditional_t<KV8 != 0, u8kv, bf16>;
  using raw_t = typename Pf80Regs<KV8>::raw_t;
  const kvt* kpool = reinterpret_cast<const kvt*>(kpool_v);
  const kvt* vpool = reinterpret_cast<const kvt*>(vpool_v);
  __shared__ __attribute__((aligned(16))) bf16 k_lds[PF80_KCH][PF80_KSTR];
  __shared__ __attribute__((aligned(16))) bf16 v_t[HS][PF80_VSTR];
  __shared__ __attribute__((aligned(16)))
      bf16 p_t[ATTN_WAVES][16][PF80_PSTR];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int n_qtiles = (T + 15) / 16;
  const int h = blockIdx.x % n_head;
  const int qtg = n_qtg - 1 - blockIdx.x / n_head;  // longest first
  const int qtile = qtg * ATTN_WAVES + wave;
  const bool active = qtile < n_qtiles;
  const int q_base = qtile * 16;
  const int qkv_dim = n_head * 3 * HS;

  const size_t cache_base =
      (((size_t)slot * n_layers_pool + layer) * n_head + h) *
      (size_t)max_seq * HS;
  const size_t scl_base =
      (((size_t)slot * n_layers_pool + layer) * n_head + h) * (size_t)max_seq;

  const int arow = lane & 15;
  const int sub = lane >> 4;
  const int koff = sub * 8;
  const int q_abs = pos0 + q_base + arow;

  // q fragments (rows past T, idle waves and dims 80..95: zero)
  bf16x8_t qf[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    qf[c] = bf16x8_t{};
    const int d = c * 32 + koff;
    if (active && q_base + arow < T && d < HS)
      qf[c] = *reinterpret_cast<const bf16x8_t*>(
          qkv + (size_t)(q_base + arow) * qkv_dim + (size_t)h * 3 * HS + d);
  }
  // K pad columns 80..95, once: 64 rows x 2 units
  if (tid < 2 * PF80_KCH)
    *reinterpret_cast<bf16x8_t*>(&k_lds[tid >> 1][HS + (tid & 1) * 8]) =
        bf16x8_t{};

  // causal bounds: the block stages up to its last tile's, a wave computes
  // up to its own
  const int qt_last = min(qtg * ATTN_WAVES + ATTN_WAVES, n_qtiles) * 16 - 1;
  const int k_last_blk = pos0 + min(qt_last, T - 1) + 1;
  const int k_last_w = active ? (pos0 + min(q_base + 15, T - 1) + 1) : 0;

  Pf80Regs<KV8> st;
  // K: 640 (row, unit) items over 3 passes; V: 320 (key pair, unit) items
  // over 2.  Keys at or past k_last_blk are staged as zeros.
  auto load_chunk = [&](int key0) {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int i = tid + it * 256;
      const int key = key0 + i / U;
      st.k[it] = raw_t{};
      st.ks[it] = 0.f;
      if (i < PF80_KCH * U && key < k_last_blk) {
        st.k[it] = *reinterpret_cast<const raw_t*>(
            kpool + cache_base + (size_t)key * HS + (i % U) * 8);
        if constexpr (KV8) st.ks[it] = kscale[scl_base + key];
      }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + it * 256;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = key0 + 2 * (i / U) + e;
        st.v[it][e] = raw_t{};
        st.vs[it][e] = 0.f;
        if (i < PF80_KCH / 2 * U && key < k_last_blk) {
          st.v[it][e] = *reinterpret_cast<const raw_t*>(
              vpool + cache_base + (size_t)key * HS + (i % U) * 8);
          if constexpr (KV8) st.vs[it][e] = vscale[scl_base + key];
        }
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int i = tid + it * 256;
      if (i < PF80_KCH * U)
        *reinterpret_cast<bf16x8_t*>(&k_lds[i / U][(i % U) * 8]) =
            pf80_to_bf16<KV8>(st.k[it], st.ks[it]);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + it * 256;
      if (i < PF80_KCH / 2 * U) {
        const bf16x8_t v0 = pf80_to_bf16<KV8>(st.v[it][0], st.vs[it][0]);
        const bf16x8_t v1 = pf80_to_bf16<KV8>(st.v[it][1], st.vs[it][1]);
        const int u = i % U;  // = row >> 3 of the eight rows written
        const int kc = (2 * (i / U)) ^ (((3 * u) & 7) << 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bf16x2_t pr;
          pr[0] = v0[j];
          pr[1] = v1[j];
          *reinterpret_cast<bf16x2_t*>(&v_t[u * 8 + j][kc]) = pr;
        }
      }
    }
  };

  float m_r = -1e30f, l_r = 0.f;
  f32x4 o_pv[HS / 16];
#pragma unroll
  for (int s = 0; s < HS / 16; ++s) o_pv[s] = {0.f, 0.f, 0.f, 0.f};

  const int n_ch = (k_last_blk + PF80_KCH - 1) / PF80_KCH;
  load_chunk(0);
  for (int ch = 0; ch < n_ch; ++ch) {
    const int key0 = ch * PF80_KCH;
    __syncthreads();  // readers of the previous chunk are done
    store_chunk();
    __syncthreads();
    if (ch + 1 < n_ch) load_chunk(key0 + PF80_KCH);  // in flight below
    if (!active || key0 >= k_last_w) continue;

    // ---- scores: 4 key tiles x 3 depth steps against the q fragments ----
    const bool full = (key0 + PF80_KCH - 1) <= (pos0 + q_base);
    float sc[PF80_KCH / 16][4];
#pragma unroll
    for (int t4 = 0; t4 < PF80_KCH / 16; ++t4) {
      f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(
            &k_lds[t4 * 16 + arow][c * 32 + koff]);
        a4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, qf[c], a4, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + t4 * 16 + sub * 4 + r;
        sc[t4][r] = (full || (key <= q_abs && key < k_last_w))
                        ? a4[r] * scale_log2e
                        : -1e30f;
      }
    }
    // ---- online softmax in base 2, state per q row arow ----
    float tmax = -1e30f;
#pragma unroll
    for (int t4 = 0; t4 < PF80_KCH / 16; ++t4)
#pragma unroll
      for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, sc[t4][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_r, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_r - m_new);
    m_r = m_new;
    float psum = 0.f;
#pragma unroll
    for (int t4 = 0; t4 < PF80_KCH / 16; ++t4) {
      bf16x4_t pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // masked keys: exp2 of about -1e30, exactly 0
        const float p = __builtin_amdgcn_exp2f(sc[t4][r] - m_new);
        psum += p;
        pk[r] = (__bf16)p;
      }
      *reinterpret_cast<bf16x4_t*>(&p_t[wave][arow][t4 * 16 + sub * 4]) = pk;
    }
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    l_r = l_r * alpha + psum;

    // ---- P.V (A = P rows from p_t, B = V^T slices), o rescaled first ----
    float al[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, sub * 4 + r, 64);
#pragma unroll
    for (int s = 0; s < HS / 16; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_pv[s][r] *= al[r];
    __builtin_amdgcn_wave_barrier();  // p_t: the wave's stores, then loads
#pragma unroll
    for (int k2 = 0; k2 < PF80_KCH / 32; ++k2) {
      const bf16x8_t ap = *reinterpret_cast<const bf16x8_t*>(
          &p_t[wave][arow][k2 * 32 + koff]);
#pragma unroll
      for (int s = 0; s < HS / 16; ++s) {
        const int vrow = s * 16 + arow;
        const int kc = ((k2 * 4 + sub) ^ ((3 * (vrow >> 3)) & 7)) << 3;
        const bf16x8_t vb =
            *reinterpret_cast<const bf16x8_t*>(&v_t[vrow][kc]);
        o_pv[s] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap, vb, o_pv[s], 0, 0, 0);
      }
    }
  }

  // ---- normalise + write (lane: q rows sub*4 + r, dims s*16 + arow) ----
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t_out = q_base + sub * 4 + r;
      const float lq = __shfl(l_r, sub * 4 + r, 64);
      if (t_out >= T) continue;
      const float inv = 1.f / lq;
      bf16* op = out + (size_t)t_out * (n_head * HS) + (size_t)h * HS + arow;
#pragma unroll
      for (int s = 0; s < HS / 16; ++s) op[s * 16] = f2b(o_pv[s][r] * inv);
    }
  }
}

void launch_prefill_attn_mha80(void* out, const void* qkv, const void* kpool,
                               const void* vpool, const float* kscale,
                               const float* vscale, int pos0, int slot,
                               int layer, int n_layers_pool, int n_head,
                               int max_seq, int T, float scale,
                               hipStream_t stream) {
  const int n_qtg = ((T + 15) / 16 + ATTN_WAVES - 1) / ATTN_WAVES;
  const float scale_log2e = scale * 1.44269504088896340736f;
  if (kscale != nullptr)
    hipLaunchKernelGGL((prefill_attn_mha80_kernel<1>), dim3(n_head * n_qtg),
                       dim3(256), 0, stream, (bf16*)out, (const bf16*)qkv,
                       kpool, vpool, kscale, vscale, pos0, slot, layer,
                       n_layers_pool, n_head, max_seq, T, scale_log2e, n_qtg);
  else
    hipLaunchKernelGGL((prefill_attn_mha80_kernel<0>), dim3(n_head * n_qtg),
                       dim3(256), 0, stream, (bf16*)out, (const bf16*)qkv,
                       kpool, vpool, kscale, vscale, pos0, slot, layer,
                       n_layers_pool, n_head, max_seq, T, scale_log2e, n_qtg);
}
