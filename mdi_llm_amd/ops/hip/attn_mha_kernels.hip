// MHA decode attention (q_per_kv == 1) for head sizes the MFMA tile core of
// decode_kernels.hip cannot map.  A translation unit of its own: its inner
// loops scale long fp32 rows by one scalar, and it is built without the
// packed fp32 instruction forms (setup.py).
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
