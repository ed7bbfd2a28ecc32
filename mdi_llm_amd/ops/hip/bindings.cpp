// Torch bindings for the hand-written CDNA4 decode kernels.
// Host-only TU: tensor checks + pointer extraction + launcher calls on the
// current torch HIP stream.

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include "decode_kernels.h"

namespace {

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

inline void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline void check_i32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
}

// Shared GEMV argument checks.  Nothing checks a launch result, so a
// launch that cannot succeed would return stale output: refuse it here.
inline void check_gemv_dims(int64_t M, int64_t K, int64_t epilogue,
                            int64_t norm_kind) {
  TORCH_CHECK(M > 0 && K > 0, "empty GEMV");
  TORCH_CHECK(epilogue >= 0 && epilogue <= 3, "epilogue must be 0..3");
  TORCH_CHECK(norm_kind >= 0 && norm_kind <= 2, "norm_kind must be 0..2");
}

// the staged kernels keep x (K bf16) in dynamic LDS; 64 KiB is what a
// launch gets without opting in to more
inline void check_staged_lds(int64_t K) {
  TORCH_CHECK(K * 2 <= 64 * 1024,
              "K too large for the staged GEMV (x must fit 64 KiB of LDS)");
}

// optional bf16 vector of exactly n elements -> pointer (or nullptr)
inline const void* opt_bf16_vec(const c10::optional<torch::Tensor>& t,
                                int64_t n, const char* name) {
  if (!t.has_value()) return nullptr;
  check_bf16(*t, name);
  TORCH_CHECK(t->numel() == n, name, " size");
  return t->data_ptr();
}

struct NormPtrs {
  const void* w = nullptr;
  const void* b = nullptr;
};

inline NormPtrs check_norm(const c10::optional<torch::Tensor>& norm_w,
                           const c10::optional<torch::Tensor>& norm_b,
                           int64_t norm_kind, int64_t K) {
  NormPtrs p;
  if (norm_kind != 0) {
    TORCH_CHECK(norm_w.has_value(), "norm_w required with norm_kind");
    p.w = opt_bf16_vec(norm_w, K, "norm_w");
    p.b = opt_bf16_vec(norm_b, K, "norm_b");
  }
  return p;
}

inline void check_fp8_weight(const torch::Tensor& W, int64_t M, int64_t K,
                             const char* name) {
  TORCH_CHECK(W.is_cuda() && W.element_size() == 1 && W.is_contiguous(),
              name, " must be contiguous fp8/uint8 on GPU");
  TORCH_CHECK(W.numel() == M * K, name, " shape mismatch");
}

// Expert indirection of the fp8 GEMVs: W holds n stacked [M, K] slabs and
// its scales n * M entries.  Returns n (0 without eidx: plain [M, K]).
inline int64_t check_fp8_stack(const c10::optional<torch::Tensor>& eidx,
                               const torch::Tensor& W, int64_t M, int64_t K,
                               int64_t norm_kind, const char* name) {
  if (!eidx.has_value()) {
    check_fp8_weight(W, M, K, name);
    return 0;
  }
  check_i32(*eidx, "eidx");
  TORCH_CHECK(eidx->numel() > 0, "eidx is empty");
  TORCH_CHECK(norm_kind != 2, "expert indirection: no LayerNorm");
  TORCH_CHECK(W.is_cuda() && W.element_size() == 1 && W.is_contiguous(),
              name, " must be contiguous fp8/uint8 on GPU");
  TORCH_CHECK(W.numel() > 0 && W.numel() % (M * K) == 0, name,
              ": stacked weight shape");
  return W.numel() / (M * K);
}

// Geometry of one prefill call, checked in full before any launch: the
// kernels index the pools with slot, layer and pos0 + t as given, so a
// value out of range would read or write outside the cache.
struct PrefillGeom {
  int n_layers, n_kv, max_seq, hs, qpk, T;
  bool kv8;
};

inline PrefillGeom check_prefill(const char* op, const torch::Tensor& qkv,
                                 const torch::Tensor& kpool,
                                 const torch::Tensor& vpool,
                                 const c10::optional<torch::Tensor>& kscale,
                                 const c10::optional<torch::Tensor>& vscale,
                                 int64_t pos0, int64_t slot, int64_t layer) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(kscale.has_value() == vscale.has_value(), op,
              ": kscale and vscale go together");
  const bool kv8 = kscale.has_value();
  if (kv8) {
    TORCH_CHECK(kpool.scalar_type() == torch::kUInt8 &&
                    vpool.scalar_type() == torch::kUInt8,
                "fp8 KV cache must be uint8 pools");
    TORCH_CHECK(kpool.is_cuda() && vpool.is_cuda() &&
                    kpool.is_contiguous() && vpool.is_contiguous(),
                op, ": pools must be contiguous on GPU");
    check_f32(*kscale, "kscale");
    check_f32(*vscale, "vscale");
  } else {
    check_bf16(kpool, "kpool");
    check_bf16(vpool, "vpool");
  }
  // pool: [slots, layers, kv_heads, max_seq, head_size]
  TORCH_CHECK(kpool.dim() == 5 && vpool.dim() == 5, op,
              ": pools must be 5-D");
  TORCH_CHECK(kpool.sizes() == vpool.sizes(), op,
              ": kpool and vpool differ in shape");
  if (kv8) {
    const auto want = kpool.sizes().slice(0, 4);
    TORCH_CHECK(kscale->sizes() == want && vscale->sizes() == want, op,
                ": scales must be [slots, layers, n_kv, max_seq]");
  }
  const int64_t n_slots = kpool.size(0);
  const int64_t n_layers = kpool.size(1);
  const int64_t n_kv = kpool.size(2);
  const int64_t max_seq = kpool.size(3);
  const int64_t hs = kpool.size(4);
  TORCH_CHECK(n_kv > 0 && hs > 0, op, ": empty pool");
  TORCH_CHECK(qkv.dim() == 2, op, ": qkv must be [T, qkv_dim]");
  const int64_t T = qkv.size(0);
  TORCH_CHECK(T >= 1, op, ": T must be at least 1");
  const int64_t qpk = qkv.size(1) / (n_kv * hs) - 2;
  TORCH_CHECK(qpk >= 1 && qkv.size(1) == n_kv * (qpk + 2) * hs, op,
              ": qkv width must be n_kv * (qpk + 2) * head_size, qpk >= 1");
  TORCH_CHECK(pos0 >= 0 && pos0 + T <= max_seq, op,
              ": pos0 + T overflows the pool (pos0=", pos0, " T=", T,
              " max_seq=", max_seq, ")");
  TORCH_CHECK(slot >= 0 && slot < n_slots, op, ": slot out of range");
  TORCH_CHECK(layer >= 0 && layer < n_layers, op, ": layer out of range");
  return PrefillGeom{(int)n_layers, (int)n_kv, (int)max_seq, (int)hs,
                     (int)qpk, (int)T, kv8};
}

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
             double eps) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  check_bf16(w, "w");
  const int n = (int)w.numel();
  TORCH_CHECK(n > 0 && x.numel() > 0, "empty rmsnorm");
  const int nb = (int)(x.numel() / n);
  TORCH_CHECK(n % 8 == 0, "n must be a multiple of 8");
  TORCH_CHECK(x.numel() == (int64_t)nb * n && out.numel() == x.numel(),
              "size mismatch");
  launch_rmsnorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), n, (float)eps,
                 nb, cur_stream());
}

void layernorm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
               c10::optional<torch::Tensor> b, double eps) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  check_bf16(w, "w");
  const int n = (int)x.numel();
  TORCH_CHECK(n > 0, "empty layernorm");
  TORCH_CHECK(n % 8 == 0, "n must be a multiple of 8");
  TORCH_CHECK(w.numel() == n && out.numel() == n, "size mismatch");
  const void* bp = opt_bf16_vec(b, n, "b");
  launch_layernorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), bp, n,
                   (float)eps, cur_stream());
}

void gemv(torch::Tensor out, torch::Tensor W, torch::Tensor x,
          c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> res,
          int64_t epilogue, c10::optional<torch::Tensor> norm_w,
          c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
          double eps, int64_t rows, c10::optional<torch::Tensor> eidx,
          int64_t estride) {
  check_bf16(out, "out");
  check_bf16(W, "W");
  check_bf16(x, "x");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, epilogue, norm_kind);
  const int* eip = nullptr;
  if (eidx.has_value()) {
    check_i32(*eidx, "eidx");
    TORCH_CHECK(eidx->numel() > 0, "eidx is empty");
    TORCH_CHECK(norm_kind != 2, "expert indirection: no LayerNorm");
    TORCH_CHECK(W.numel() % ((int64_t)M * K) == 0, "stacked W shape");
    eip = eidx->data_ptr<int>();
  } else {
    TORCH_CHECK(W.numel() == (int64_t)M * K, "W shape mismatch");
  }
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  if (norm_kind == 2) check_staged_lds(K);  // 0/1 run the direct kernels
  const void* bp = opt_bf16_vec(bias, M, "bias");
  const void* rp = opt_bf16_vec(res, M, "res");
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv(out.data_ptr(), W.data_ptr(), x.data_ptr(), bp, rp, nwp, nbp,
              (float)eps, M, K, (int)epilogue, (int)norm_kind, (int)rows,
              eip, (long long)estride, cur_stream());
}

void gemv_fp8(torch::Tensor out, torch::Tensor W, torch::Tensor wscale,
              torch::Tensor x, c10::optional<torch::Tensor> bias,
              c10::optional<torch::Tensor> res, int64_t epilogue,
              c10::optional<torch::Tensor> norm_w,
              c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
              double eps, int64_t rows, c10::optional<torch::Tensor> eidx,
              int64_t estride) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  check_f32(wscale, "wscale");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, epilogue, norm_kind);
  const int64_t n_slab = check_fp8_stack(eidx, W, M, K, norm_kind, "W");
  TORCH_CHECK(K % 16 == 0, "K must be a multiple of 16 for fp8 weights");
  TORCH_CHECK(wscale.numel() == (n_slab ? n_slab : 1) * M, "wscale size");
  TORCH_CHECK(n_slab == 0 || estride == (int64_t)M * K,
              "estride must be M * K");
  check_staged_lds(K);
  const void* bp = opt_bf16_vec(bias, M, "bias");
  const void* rp = opt_bf16_vec(res, M, "res");
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv_fp8(out.data_ptr(), W.data_ptr(), wscale.data_ptr<float>(),
                  x.data_ptr(), bp, rp, nwp, nbp, (float)eps, M, K,
                  (int)epilogue, (int)norm_kind, (int)rows,
                  n_slab ? eidx->data_ptr<int>() : nullptr,
                  (long long)estride, (int)n_slab, cur_stream());
}

void gemv_swiglu_fp8(torch::Tensor out, torch::Tensor Wg,
                     torch::Tensor gscale, torch::Tensor Wu,
                     torch::Tensor uscale, torch::Tensor x, bool gelu_gate,
                     c10::optional<torch::Tensor> norm_w,
                     c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
                     double eps, c10::optional<torch::Tensor> eidx,
                     int64_t estride, c10::optional<torch::Tensor> escale) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  check_f32(gscale, "gscale");
  check_f32(uscale, "uscale");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, 0, norm_kind);
  const int64_t n_slab = check_fp8_stack(eidx, Wg, M, K, norm_kind, "Wg");
  TORCH_CHECK(check_fp8_stack(eidx, Wu, M, K, norm_kind, "Wu") == n_slab,
              "Wu: stacked weight shape");
  TORCH_CHECK(K % 16 == 0, "K must be a multiple of 16 for fp8 weights");
  const int64_t n_scale = (n_slab ? n_slab : 1) * M;
  TORCH_CHECK(gscale.numel() == n_scale && uscale.numel() == n_scale,
              "gscale/uscale size");
  TORCH_CHECK(n_slab == 0 || estride == (int64_t)M * K,
              "estride must be M * K");
  const float* esp = nullptr;
  if (escale.has_value()) {
    check_f32(*escale, "escale");
    TORCH_CHECK(escale->numel() > 0, "escale is empty");
    esp = escale->data_ptr<float>();
  }
  check_staged_lds(K);
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv_swiglu_fp8(out.data_ptr(), Wg.data_ptr(),
                         gscale.data_ptr<float>(), Wu.data_ptr(),
                         uscale.data_ptr<float>(), x.data_ptr(), nwp, nbp,
                         (float)eps, M, K, gelu_gate ? 1 : 0,
                         (int)norm_kind,
                         n_slab ? eidx->data_ptr<int>() : nullptr,
                         (long long)estride, (int)n_slab, esp, cur_stream());
}

// packed int4 weights [M, Kp/2] (uint8) + bf16 (scale, zero) [M, Kp/128, 2]
inline void check_int4(const torch::Tensor& W, const torch::Tensor& qparams,
                       int M, int K, const char* name) {
  const int64_t Kp = ((int64_t)K + 127) / 128 * 128;
  TORCH_CHECK(W.is_cuda() && W.scalar_type() == torch::kUInt8 &&
                  W.is_contiguous(),
              name, " must be contiguous uint8 on GPU");
  TORCH_CHECK(W.numel() == (int64_t)M * Kp / 2, name, " shape mismatch");
  check_bf16(qparams, "qparams");
  TORCH_CHECK(qparams.numel() == (int64_t)M * (Kp / 128) * 2,
              "qparams shape mismatch");
  TORCH_CHECK(Kp * 2 + Kp / 128 * 4 <= 64 * 1024,
              "K too large for the staged int4 GEMV");
}

void gemv_int4(torch::Tensor out, torch::Tensor W, torch::Tensor qparams,
               torch::Tensor x, c10::optional<torch::Tensor> bias,
               c10::optional<torch::Tensor> res, int64_t epilogue,
               c10::optional<torch::Tensor> norm_w,
               c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
               double eps, int64_t rows) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, epilogue, norm_kind);
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  check_int4(W, qparams, M, K, "W");
  const void* bp = opt_bf16_vec(bias, M, "bias");
  const void* rp = opt_bf16_vec(res, M, "res");
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv_int4(out.data_ptr(), W.data_ptr(), qparams.data_ptr(),
                   x.data_ptr(), bp, rp, nwp, nbp, (float)eps, M, K,
                   (int)epilogue, (int)norm_kind, (int)rows, cur_stream());
}

void gemv_swiglu_int4(torch::Tensor out, torch::Tensor Wg, torch::Tensor gq,
                      torch::Tensor Wu, torch::Tensor uq, torch::Tensor x,
                      bool gelu_gate, c10::optional<torch::Tensor> norm_w,
                      c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
                      double eps) {
  check_bf16(out, "out");
  check_bf16(x, "x");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, 0, norm_kind);
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  check_int4(Wg, gq, M, K, "Wg");
  check_int4(Wu, uq, M, K, "Wu");
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv_swiglu_int4(out.data_ptr(), Wg.data_ptr(), gq.data_ptr(),
                          Wu.data_ptr(), uq.data_ptr(), x.data_ptr(), nwp,
                          nbp, (float)eps, M, K, gelu_gate ? 1 : 0,
                          (int)norm_kind, cur_stream());
}

void gemv_swiglu(torch::Tensor out, torch::Tensor Wg, torch::Tensor Wu,
                 torch::Tensor x, bool gelu_gate,
                 c10::optional<torch::Tensor> norm_w,
                 c10::optional<torch::Tensor> norm_b, int64_t norm_kind,
                 double eps, c10::optional<torch::Tensor> eidx,
                 int64_t estride, c10::optional<torch::Tensor> escale) {
  check_bf16(out, "out");
  check_bf16(Wg, "Wg");
  check_bf16(Wu, "Wu");
  check_bf16(x, "x");
  const int K = (int)x.numel();
  const int M = (int)out.numel();
  check_gemv_dims(M, K, 0, norm_kind);
  const int* eip = nullptr;
  const float* esp = nullptr;
  if (eidx.has_value()) {
    check_i32(*eidx, "eidx");
    TORCH_CHECK(eidx->numel() > 0, "eidx is empty");
    TORCH_CHECK(Wg.numel() % ((int64_t)M * K) == 0 &&
                    Wu.numel() % ((int64_t)M * K) == 0,
                "stacked weight shape");
    eip = eidx->data_ptr<int>();
  } else {
    TORCH_CHECK(Wg.numel() == (int64_t)M * K && Wu.numel() == (int64_t)M * K,
                "weight shape mismatch");
  }
  if (escale.has_value()) {
    check_f32(*escale, "escale");
    TORCH_CHECK(escale->numel() > 0, "escale is empty");
    esp = escale->data_ptr<float>();
  }
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  check_staged_lds(K);
  const NormPtrs np = check_norm(norm_w, norm_b, norm_kind, K);
  const void* nwp = np.w;
  const void* nbp = np.b;
  launch_gemv_swiglu(out.data_ptr(), Wg.data_ptr(), Wu.data_ptr(),
                     x.data_ptr(), nwp, nbp, (float)eps, M, K,
                     gelu_gate ? 1 : 0, (int)norm_kind, eip,
                     (long long)estride, esp, cur_stream());
}

void swiglu_mul(torch::Tensor out, torch::Tensor g, torch::Tensor u,
                bool gelu_gate) {
  check_bf16(out, "out");
  check_bf16(g, "g");
  check_bf16(u, "u");
  TORCH_CHECK(out.numel() == g.numel() && g.numel() == u.numel() &&
                  g.numel() % 8 == 0,
              "swiglu_mul: equal sizes, multiple of 8");
  launch_swiglu_mul(out.data_ptr(), g.data_ptr(), u.data_ptr(),
                    (long long)g.numel(), gelu_gate ? 1 : 0, cur_stream());
}

void moe_gate_topk(torch::Tensor eidx, torch::Tensor escale,
                   torch::Tensor logits, int64_t k) {
  check_i32(eidx, "eidx");
  check_f32(escale, "escale");
  check_bf16(logits, "logits");
  const int n_e = (int)logits.numel();
  TORCH_CHECK(n_e <= 64 && k <= 8 && k >= 1 && eidx.numel() >= k &&
                  escale.numel() >= k,
              "moe_gate_topk: n_e <= 64, 1 <= k <= 8");
  launch_moe_gate_topk(eidx.data_ptr<int>(), escale.data_ptr<float>(),
                       logits.data_ptr(), n_e, (int)k, cur_stream());
}

inline void check_i32n(const torch::Tensor& t, const char* name,
                       int64_t n) {
  check_i32(t, name);
  TORCH_CHECK(t.is_contiguous() && t.numel() == n, name, ": expected ", n,
              " contiguous int32 elements");
}

void moe_route_group(torch::Tensor eidx, torch::Tensor escale,
                     torch::Tensor count, torch::Tensor offset,
                     torch::Tensor perm, torch::Tensor inv,
                     torch::Tensor logits, int64_t k) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, n_expert]");
  const int64_t B = logits.size(0), n_e = logits.size(1);
  TORCH_CHECK(B >= 1 && B <= 128 && n_e >= 1 && n_e <= 64 && k >= 1 &&
                  k <= 8 && k <= n_e,
              "moe_route_group: B <= 128, n_e <= 64, 1 <= k <= min(8, n_e)");
  check_i32n(eidx, "eidx", B * k);
  check_f32(escale, "escale");
  TORCH_CHECK(escale.numel() == B * k, "escale size");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  check_i32n(perm, "perm", B * k);
  check_i32n(inv, "inv", B * k);
  launch_moe_route_group(eidx.data_ptr<int>(), escale.data_ptr<float>(),
                         count.data_ptr<int>(), offset.data_ptr<int>(),
                         perm.data_ptr<int>(), inv.data_ptr<int>(),
                         logits.data_ptr(), (int)B, (int)n_e, (int)k,
                         cur_stream());
}

void moe_group_swiglu(torch::Tensor act, torch::Tensor Wg, torch::Tensor Wu,
                      torch::Tensor X, torch::Tensor count,
                      torch::Tensor offset, torch::Tensor perm,
                      torch::Tensor escale, int64_t k) {
  check_bf16(act, "act");
  check_bf16(Wg, "Wg");
  check_bf16(Wu, "Wu");
  check_bf16(X, "X");
  TORCH_CHECK(Wg.dim() == 3 && X.dim() == 2 && act.dim() == 2,
              "moe_group_swiglu: Wg [n_e,M,K], X [B,K], act [B*k,M]");
  const int64_t n_e = Wg.size(0), M = Wg.size(1), K = Wg.size(2);
  const int64_t B = X.size(0);
  TORCH_CHECK(Wu.sizes() == Wg.sizes(), "Wu shape");
  TORCH_CHECK(X.size(1) == K && act.size(0) == B * k && act.size(1) == M,
              "moe_group_swiglu: size mismatch");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  check_i32n(perm, "perm", B * k);
  check_f32(escale, "escale");
  TORCH_CHECK(escale.numel() == B * k, "escale size");
  const int rc = launch_moe_group_gemm(
      act.data_ptr(), Wg.data_ptr(), Wu.data_ptr(), X.data_ptr(),
      count.data_ptr<int>(), offset.data_ptr<int>(), perm.data_ptr<int>(),
      escale.data_ptr<float>(), (int)B, (int)n_e, (int)M, (int)K, (int)k, 1,
      cur_stream());
  TORCH_CHECK(rc == 0, "moe_group_swiglu: needs K % 32 == 0, M % 16 == 0, "
                       "B <= 128, n_e <= 64, k <= 8");
}

void moe_group_down(torch::Tensor D, torch::Tensor Wd, torch::Tensor act,
                    torch::Tensor count, torch::Tensor offset,
                    int64_t n_tokens) {
  check_f32(D, "D");
  check_bf16(Wd, "Wd");
  check_bf16(act, "act");
  TORCH_CHECK(Wd.dim() == 3 && act.dim() == 2 && D.dim() == 2,
              "moe_group_down: Wd [n_e,M,K], act [B*k,K], D [B*k,M]");
  const int64_t n_e = Wd.size(0), M = Wd.size(1), K = Wd.size(2);
  const int64_t R = act.size(0);
  TORCH_CHECK(n_tokens >= 1 && R % n_tokens == 0,
              "moe_group_down: rows must be n_tokens * k");
  TORCH_CHECK(act.size(1) == K && D.size(0) == R && D.size(1) == M,
              "moe_group_down: size mismatch");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  const int rc = launch_moe_group_gemm(
      D.data_ptr(), Wd.data_ptr(), nullptr, act.data_ptr(),
      count.data_ptr<int>(), offset.data_ptr<int>(), nullptr, nullptr,
      (int)n_tokens, (int)n_e, (int)M, (int)K, (int)(R / n_tokens), 0,
      cur_stream());
  TORCH_CHECK(rc == 0, "moe_group_down: needs K % 32 == 0, M % 16 == 0, "
                       "B <= 128, n_e <= 64, k <= 8");
}

// fp8 slab [n_e, M, K] + fp32 row scales [n_e, M]
inline void check_fp8_slab(const torch::Tensor& W, const torch::Tensor& s,
                           const char* name) {
  TORCH_CHECK(W.is_cuda() && W.element_size() == 1 && W.is_contiguous() &&
                  W.dim() == 3,
              name, " must be a contiguous fp8/uint8 [n_e, M, K] on GPU");
  check_f32(s, name);
  TORCH_CHECK(s.numel() == W.size(0) * W.size(1), name,
              ": scales must be [n_e, M]");
}

void moe_group_swiglu_fp8(torch::Tensor act, torch::Tensor Wg,
                          torch::Tensor gscale, torch::Tensor Wu,
                          torch::Tensor uscale, torch::Tensor X,
                          torch::Tensor count, torch::Tensor offset,
                          torch::Tensor perm, torch::Tensor escale,
                          int64_t k) {
  check_bf16(act, "act");
  check_fp8_slab(Wg, gscale, "Wg");
  check_fp8_slab(Wu, uscale, "Wu");
  check_bf16(X, "X");
  TORCH_CHECK(X.dim() == 2 && act.dim() == 2,
              "moe_group_swiglu_fp8: X [B,K], act [B*k,M]");
  const int64_t n_e = Wg.size(0), M = Wg.size(1), K = Wg.size(2);
  const int64_t B = X.size(0);
  TORCH_CHECK(Wu.sizes() == Wg.sizes(), "Wu shape");
  TORCH_CHECK(X.size(1) == K && act.size(0) == B * k && act.size(1) == M,
              "moe_group_swiglu_fp8: size mismatch");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  check_i32n(perm, "perm", B * k);
  check_f32(escale, "escale");
  TORCH_CHECK(escale.numel() == B * k, "escale size");
  const int rc = launch_moe_group_gemm_fp8(
      act.data_ptr(), Wg.data_ptr(), gscale.data_ptr<float>(), Wu.data_ptr(),
      uscale.data_ptr<float>(), X.data_ptr(), count.data_ptr<int>(),
      offset.data_ptr<int>(), perm.data_ptr<int>(), escale.data_ptr<float>(),
      (int)B, (int)n_e, (int)M, (int)K, (int)k, 1, cur_stream());
  TORCH_CHECK(rc == 0, "moe_group_swiglu_fp8: needs K % 32 == 0, "
                       "M % 16 == 0, B <= 128, n_e <= 64, k <= 8");
}

void moe_group_down_fp8(torch::Tensor D, torch::Tensor Wd,
                        torch::Tensor dscale, torch::Tensor act,
                        torch::Tensor count, torch::Tensor offset,
                        int64_t n_tokens) {
  check_f32(D, "D");
  check_fp8_slab(Wd, dscale, "Wd");
  check_bf16(act, "act");
  TORCH_CHECK(act.dim() == 2 && D.dim() == 2,
              "moe_group_down_fp8: act [B*k,K], D [B*k,M]");
  const int64_t n_e = Wd.size(0), M = Wd.size(1), K = Wd.size(2);
  const int64_t R = act.size(0);
  TORCH_CHECK(n_tokens >= 1 && R % n_tokens == 0,
              "moe_group_down_fp8: rows must be n_tokens * k");
  TORCH_CHECK(act.size(1) == K && D.size(0) == R && D.size(1) == M,
              "moe_group_down_fp8: size mismatch");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  const int rc = launch_moe_group_gemm_fp8(
      D.data_ptr(), Wd.data_ptr(), dscale.data_ptr<float>(), nullptr,
      nullptr, act.data_ptr(), count.data_ptr<int>(),
      offset.data_ptr<int>(), nullptr, nullptr, (int)n_tokens, (int)n_e,
      (int)M, (int)K, (int)(R / n_tokens), 0, cur_stream());
  TORCH_CHECK(rc == 0, "moe_group_down_fp8: needs K % 32 == 0, M % 16 == 0, "
                       "B <= 128, n_e <= 64, k <= 8");
}

void moe_group_combine(torch::Tensor out, torch::Tensor res, torch::Tensor D,
                       torch::Tensor inv, int64_t k) {
  check_bf16(out, "out");
  check_bf16(res, "res");
  check_f32(D, "D");
  TORCH_CHECK(res.dim() == 2 && D.dim() == 2, "res [B,E], D [B*k,E]");
  const int64_t B = res.size(0), E = res.size(1);
  TORCH_CHECK(out.sizes() == res.sizes() && D.size(0) == B * k &&
                  D.size(1) == E && E % 8 == 0 && k >= 1,
              "moe_group_combine: size mismatch");
  check_i32n(inv, "inv", B * k);
  launch_moe_group_combine(out.data_ptr(), res.data_ptr(),
                           D.data_ptr<float>(), inv.data_ptr<int>(), (int)B,
                           (int)E, (int)k, cur_stream());
}

void moe_route_prefill(torch::Tensor eidx, torch::Tensor escale,
                       torch::Tensor count, torch::Tensor offset,
                       torch::Tensor perm, torch::Tensor inv,
                       torch::Tensor logits, int64_t k) {
  check_bf16(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
              "logits must be a contiguous [T, n_expert]");
  const int64_t T = logits.size(0), n_e = logits.size(1);
  TORCH_CHECK(T >= 1 && n_e >= 1 && n_e <= 64 && k >= 1 && k <= 8 &&
                  k <= n_e && T * k <= 65536,
              "moe_route_prefill: T*k <= 65536, n_e <= 64, "
              "1 <= k <= min(8, n_e)");
  check_i32n(eidx, "eidx", T * k);
  check_f32(escale, "escale");
  TORCH_CHECK(escale.is_contiguous() && escale.numel() == T * k,
              "escale size");
  check_i32n(count, "count", n_e);
  check_i32n(offset, "offset", n_e + 1);
  check_i32n(perm, "perm", T * k);
  check_i32n(inv, "inv", T * k);
  auto segcnt = torch::empty(
      {(int64_t)moe_prefill_route_workspace((int)T, (int)n_e, (int)k)},
      count.options());
  const int rc = launch_moe_route_prefill(
      eidx.data_ptr<int>(), escale.data_ptr<float>(), count.data_ptr<int>(),
      offset.data_ptr<int>(), perm.data_ptr<int>(), inv.data_ptr<int>(),
      segcnt.data_ptr<int>(), logits.data_ptr(), (int)T, (int)n_e, (int)k,
      cur_stream());
  TORCH_CHECK(rc == 0, "moe_route_prefill: size out of range");
}

inline void check_bf16_rows(const torch::Tensor& t, const char* name,
                            int64_t rows, int64_t cols) {
  check_bf16(t, name);
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.size(0) == rows &&
                  t.size(1) == cols,
              name, ": expected a contiguous [", rows, ", ", cols, "]");
}

void moe_prefill_gather(torch::Tensor XG, torch::Tensor hn,
                        torch::Tensor perm, int64_t k) {
  check_bf16(hn, "hn");
  TORCH_CHECK(hn.dim() == 2 && hn.is_contiguous(), "hn must be [T, E]");
  const int64_t T = hn.size(0), E = hn.size(1);
  TORCH_CHECK(k >= 1 && T >= 1 && T * k <= 65536 && E % 8 == 0,
              "moe_prefill_gather: T*k <= 65536, E % 8 == 0");
  check_bf16_rows(XG, "XG", T * k, E);
  check_i32n(perm, "perm", T * k);
  launch_moe_prefill_gather(XG.data_ptr(), hn.data_ptr(),
                            perm.data_ptr<int>(), (int)(T * k), (int)E,
                            (int)k, cur_stream());
}

void moe_prefill_act(torch::Tensor ACT, torch::Tensor G, torch::Tensor U,
                     torch::Tensor escale, torch::Tensor perm) {
  check_bf16(G, "G");
  TORCH_CHECK(G.dim() == 2 && G.is_contiguous(), "G must be [T*k, I]");
  const int64_t R = G.size(0), I = G.size(1);
  TORCH_CHECK(R >= 1 && R <= 65536 && I % 8 == 0,
              "moe_prefill_act: T*k <= 65536, I % 8 == 0");
  check_bf16_rows(U, "U", R, I);
  check_bf16_rows(ACT, "ACT", R, I);
  check_f32(escale, "escale");
  TORCH_CHECK(escale.is_contiguous() && escale.numel() == R, "escale size");
  check_i32n(perm, "perm", R);
  launch_moe_prefill_act(ACT.data_ptr(), G.data_ptr(), U.data_ptr(),
                         escale.data_ptr<float>(), perm.data_ptr<int>(),
                         (int)R, (int)I, cur_stream());
}

void moe_prefill_combine(torch::Tensor out, torch::Tensor res,
                         torch::Tensor D, torch::Tensor inv, int64_t k) {
  check_bf16(res, "res");
  TORCH_CHECK(res.dim() == 2 && res.is_contiguous(), "res must be [T, E]");
  const int64_t T = res.size(0), E = res.size(1);
  TORCH_CHECK(k >= 1 && T >= 1 && T * k <= 65536 && E % 8 == 0,
              "moe_prefill_combine: T*k <= 65536, E % 8 == 0");
  check_bf16_rows(out, "out", T, E);
  check_bf16_rows(D, "D", T * k, E);
  check_i32n(inv, "inv", T * k);
  launch_moe_prefill_combine(out.data_ptr(), res.data_ptr(), D.data_ptr(),
                             inv.data_ptr<int>(), (int)T, (int)E, (int)k,
                             cur_stream());
}

void embed(torch::Tensor out, torch::Tensor wte, torch::Tensor token,
           double scale) {
  check_bf16(out, "out");
  check_bf16(wte, "wte");
  check_i32(token, "token");
  const int n = (int)out.numel();
  TORCH_CHECK(n % 8 == 0, "n_embd must be a multiple of 8");
  launch_embed(out.data_ptr(), wte.data_ptr(), token.data_ptr<int>(), n,
               (float)scale, cur_stream());
}

void rope_kv_append(torch::Tensor qkv, torch::Tensor kpool,
                    torch::Tensor vpool, torch::Tensor cos_t,
                    torch::Tensor sin_t, torch::Tensor pos,
                    torch::Tensor slot, int64_t layer) {
  check_bf16(qkv, "qkv");
  check_bf16(kpool, "kpool");
  check_bf16(vpool, "vpool");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  check_i32(pos, "pos");
  check_i32(slot, "slot");
  // pool: [slots, layers, kv_heads, max_seq, head_size]
  TORCH_CHECK(kpool.dim() == 5, "kpool must be 5-D");
  const int n_layers_pool = (int)kpool.size(1);
  const int n_kv = (int)kpool.size(2);
  const int max_seq = (int)kpool.size(3);
  const int hs = (int)kpool.size(4);
  const int rope_n_elem = (int)cos_t.size(1);
  const int qkv_dim = (int)qkv.numel();
  const int qpk = qkv_dim / (n_kv * hs) - 2;
  TORCH_CHECK(qpk >= 1, "bad qkv length");
  launch_rope_kv_append(qkv.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
                        cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                        pos.data_ptr<int>(), slot.data_ptr<int>(),
                        (int)layer, n_layers_pool, n_kv, max_seq, hs,
                        rope_n_elem, qpk, cur_stream());
}

void attn_decode(torch::Tensor out, torch::Tensor part_o,
                 torch::Tensor part_ml, torch::Tensor qkv,
                 torch::Tensor kpool, torch::Tensor vpool,
                 torch::Tensor cos_t, torch::Tensor sin_t, torch::Tensor pos,
                 torch::Tensor slot, int64_t layer, int64_t n_chunks,
                 double scale, int64_t n_batch,
                 c10::optional<torch::Tensor> kscale,
                 c10::optional<torch::Tensor> vscale,
                 int64_t force_split) {
  check_bf16(out, "out");
  check_f32(part_o, "part_o");
  check_f32(part_ml, "part_ml");
  check_bf16(qkv, "qkv");
  const bool kv8 = kscale.has_value();
  if (kv8) {
    TORCH_CHECK(kpool.scalar_type() == torch::kUInt8 &&
                    vpool.scalar_type() == torch::kUInt8,
                "fp8 KV cache must be uint8 pools");
    check_f32(*kscale, "kscale");
    check_f32(*vscale, "vscale");
  } else {
    check_bf16(kpool, "kpool");
    check_bf16(vpool, "vpool");
  }
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  check_i32(pos, "pos");
  check_i32(slot, "slot");
  const int n_layers_pool = (int)kpool.size(1);
  const int n_kv = (int)kpool.size(2);
  const int max_seq = (int)kpool.size(3);
  const int hs = (int)kpool.size(4);
  const int rope_ne = cos_t.dim() > 1 ? (int)cos_t.size(1) : 0;
  const int nb = (int)n_batch;
  const int beff = nb > 0 ? nb : 1;
  const int qkv_dim = (int)(qkv.numel() / beff);
  const int qpk = qkv_dim / (n_kv * hs) - 2;
  const int n_head = n_kv * qpk;
  // the split-S kernel stages q once per 4-wave block (needs n_chunks % 4
  // == 0 so a block's waves share one (batch, kv head)) and the combine
  // keeps chunk weights in 4 registers x 64 lanes (chunks >= 256 would be
  // silently ignored)
  TORCH_CHECK(n_chunks >= 4 && n_chunks % 4 == 0 && n_chunks <= 256,
              "attn_decode: n_chunks must be a multiple of 4 in [4, 256], "
              "got ", n_chunks);
  if (nb > 0) {
    TORCH_CHECK(pos.numel() >= nb && slot.numel() >= nb,
                "pos/slot arrays too small for batch");
  }
  TORCH_CHECK(part_o.numel() >= (int64_t)beff * n_head * n_chunks * hs,
              "part_o too small");
  TORCH_CHECK(part_ml.numel() >= (int64_t)beff * n_head * n_chunks * 2,
              "part_ml too small");
  TORCH_CHECK(out.numel() == (int64_t)beff * n_head * hs, "out size");
  int rc = launch_attn_decode(
      out.data_ptr(), part_o.data_ptr<float>(), part_ml.data_ptr<float>(),
      qkv.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
      kv8 ? kscale->data_ptr<float>() : nullptr,
      kv8 ? vscale->data_ptr<float>() : nullptr,
      rope_ne ? cos_t.data_ptr<float>() : nullptr,
      rope_ne ? sin_t.data_ptr<float>() : nullptr, rope_ne,
      pos.data_ptr<int>(), slot.data_ptr<int>(), (int)layer, n_layers_pool,
      n_kv, max_seq, hs, qpk, (int)n_chunks, (float)scale, nb,
      (int)force_split, cur_stream());
  TORCH_CHECK(rc == 0, "attn_decode: unsupported geometry qpk=", qpk,
              " head_size=", hs);
}

void attn_proj(torch::Tensor out, torch::Tensor qkv, torch::Tensor kpool,
               torch::Tensor vpool, torch::Tensor cos_t,
               torch::Tensor sin_t, torch::Tensor pos, torch::Tensor slot,
               int64_t layer, double scale, torch::Tensor W,
               c10::optional<torch::Tensor> bias,
               c10::optional<torch::Tensor> res, torch::Tensor gran) {
  check_bf16(out, "out");
  check_bf16(qkv, "qkv");
  check_bf16(kpool, "kpool");
  check_bf16(vpool, "vpool");
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  check_i32(pos, "pos");
  check_i32(slot, "slot");
  check_bf16(W, "W");
  TORCH_CHECK(gran.is_cuda() && gran.scalar_type() == torch::kInt32,
              "gran must be int32 on GPU");
  const int n_layers_pool = (int)kpool.size(1);
  const int n_kv = (int)kpool.size(2);
  const int max_seq = (int)kpool.size(3);
  const int hs = (int)kpool.size(4);
  const int rope_ne = cos_t.dim() > 1 ? (int)cos_t.size(1) : 0;
  const int qkv_dim = (int)qkv.numel();
  const int qpk = qkv_dim / (n_kv * hs) - 2;
  const int K = n_kv * qpk * hs;
  const int M = (int)W.size(0);
  TORCH_CHECK((int)W.size(1) == K, "proj W inner dim mismatch");
  TORCH_CHECK(out.numel() >= M, "out too small");
  TORCH_CHECK(gran.numel() >= K / 2 + 16, "y/flag scratch too small");
  TORCH_CHECK(K % 128 == 0 && K / 2 <= 4096,
              "attn_proj: unsupported K for granule sweep");
  int rc = launch_attn_proj(
      out.data_ptr(), qkv.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
      rope_ne ? cos_t.data_ptr<float>() : nullptr,
      rope_ne ? sin_t.data_ptr<float>() : nullptr, rope_ne,
      pos.data_ptr<int>(), slot.data_ptr<int>(), (int)layer, n_layers_pool,
      n_kv, max_seq, hs, qpk, (float)scale, W.data_ptr(),
      bias.has_value() ? bias->data_ptr() : nullptr,
      res.has_value() ? res->data_ptr() : nullptr, gran.data_ptr(), M,
      cur_stream());
  TORCH_CHECK(rc == 0, "attn_proj: unsupported geometry qpk=", qpk,
              " head_size=", hs, " max_seq=", max_seq);
}

void sample(torch::Tensor out_token, torch::Tensor logits,
            torch::Tensor scratch, double temperature, int64_t top_k,
            bool noise, int64_t seed, c10::optional<torch::Tensor> pos,
            c10::optional<torch::Tensor> slot, int64_t n_batch,
            double top_p, c10::optional<torch::Tensor> token_table,
            c10::optional<torch::Tensor> pos_table,
            c10::optional<torch::Tensor> adv_slot, int64_t adv_pos,
            int64_t pos_bias) {
  check_i32(out_token, "out_token");
  check_bf16(logits, "logits");
  const int nb = n_batch > 0 ? (int)n_batch : 1;
  TORCH_CHECK(scratch.is_cuda() && scratch.scalar_type() == torch::kInt32 &&
                  scratch.numel() >= 520 * nb,
              "scratch must be >=520 int32 per sample on GPU");
  TORCH_CHECK(out_token.numel() >= nb, "out_token too small");
  const int* pp = nullptr;
  const int* sp = nullptr;
  if (pos.has_value()) {
    check_i32(*pos, "pos");
    TORCH_CHECK(pos->numel() >= nb, "pos too small");
    pp = pos->data_ptr<int>();
  }
  if (slot.has_value()) {
    check_i32(*slot, "slot");
    TORCH_CHECK(slot->numel() >= nb, "slot too small");
    sp = slot->data_ptr<int>();
  }
  int* ttp = nullptr;
  int* ptp = nullptr;
  const int* asp = nullptr;
  if (token_table.has_value()) {
    check_i32(*token_table, "token_table");
    ttp = token_table->data_ptr<int>();
  }
  if (pos_table.has_value()) {
    check_i32(*pos_table, "pos_table");
    ptp = pos_table->data_ptr<int>();
  }
  if (adv_slot.has_value()) {
    check_i32(*adv_slot, "adv_slot");
    asp = adv_slot->data_ptr<int>();
  }
  const int V = (int)(logits.numel() / nb);
  launch_sample(out_token.data_ptr(), logits.data_ptr(), V,
                scratch.data_ptr(), (float)temperature, (int)top_k,
                (float)top_p, noise ? 1 : 0, (unsigned)(int64_t)seed, pp, sp,
                (int)n_batch, ttp, ptp, asp, (int)adv_pos, (int)pos_bias,
                cur_stream());
}

void mtile_gemm(torch::Tensor Y, torch::Tensor W, torch::Tensor X,
                c10::optional<torch::Tensor> bias,
                c10::optional<torch::Tensor> res) {
  check_bf16(Y, "Y");
  check_bf16(W, "W");
  check_bf16(X, "X");
  TORCH_CHECK(W.dim() == 2 && X.dim() == 2,
              "mtile_gemm: W and X must be 2-D");
  const int Bsz = (int)X.size(0);
  const int K = (int)X.size(1);
  const int M = (int)W.size(0);
  TORCH_CHECK((int)W.size(1) == K, "mtile_gemm: K mismatch");
  TORCH_CHECK(Y.numel() >= (int64_t)Bsz * M, "mtile_gemm: Y too small");
  // the epilogue reads bias[m] and res[b * M + m] unconditionally
  const void* bp = opt_bf16_vec(bias, M, "bias");
  const void* rp = opt_bf16_vec(res, (int64_t)Bsz * M, "res");
  const auto dev = Y.device();
  TORCH_CHECK(W.device() == dev && X.device() == dev &&
                  (!bias.has_value() || bias->device() == dev) &&
                  (!res.has_value() || res->device() == dev),
              "mtile_gemm: all tensors must be on one device");
  int rc = launch_mtile_gemm(
      Y.data_ptr(), W.data_ptr(), X.data_ptr(), bp, rp, Bsz, M, K,
      cur_stream());
  TORCH_CHECK(rc == 0, "mtile_gemm: unsupported shape B=", Bsz, " K=", K,
              " M=", M);
}

void route_env(torch::Tensor hdr, torch::Tensor slot_out,
               torch::Tensor pos_table, int64_t dummy_slot) {
  check_i32(hdr, "hdr");
  check_i32(slot_out, "slot_out");
  check_i32(pos_table, "pos_table");
  launch_route_env(hdr.data_ptr<int>(), slot_out.data_ptr<int>(),
                   pos_table.data_ptr<int>(), (int)dummy_slot, cur_stream());
}

void stage_slot(torch::Tensor slot, c10::optional<torch::Tensor> pos_out,
                c10::optional<torch::Tensor> token_out,
                c10::optional<torch::Tensor> pos_table,
                c10::optional<torch::Tensor> token_table,
                c10::optional<torch::Tensor> pos_table_mut,
                int64_t adv_pos) {
  check_i32(slot, "slot");
  int* po = pos_out.has_value() ? pos_out->data_ptr<int>() : nullptr;
  int* to = token_out.has_value() ? token_out->data_ptr<int>() : nullptr;
  const int* pt =
      pos_table.has_value() ? pos_table->data_ptr<int>() : nullptr;
  const int* tt =
      token_table.has_value() ? token_table->data_ptr<int>() : nullptr;
  int* ptm =
      pos_table_mut.has_value() ? pos_table_mut->data_ptr<int>() : nullptr;
  launch_stage_slot(po, to, pt, tt, ptm, slot.data_ptr<int>(),
                    (int)adv_pos, cur_stream());
}

void rope_prefill_append(torch::Tensor qkv, torch::Tensor kpool,
                         torch::Tensor vpool, torch::Tensor cos_t,
                         torch::Tensor sin_t, int64_t pos0, int64_t slot,
                         int64_t layer,
                         c10::optional<torch::Tensor> kscale,
                         c10::optional<torch::Tensor> vscale) {
  const PrefillGeom g =
      check_prefill("rope_prefill_append", qkv, kpool, vpool, kscale, vscale,
                    pos0, slot, layer);
  check_f32(cos_t, "cos");
  check_f32(sin_t, "sin");
  TORCH_CHECK(cos_t.sizes() == sin_t.sizes(),
              "rope_prefill_append: cos and sin differ in shape");
  // a 1-D (or zero-width) table switches rope off
  const int64_t rope_ne = cos_t.dim() > 1 ? cos_t.size(1) : 0;
  if (rope_ne > 0) {
    TORCH_CHECK(cos_t.dim() == 2, "rope_prefill_append: cos must be 2-D");
    TORCH_CHECK(rope_ne % 2 == 0 && rope_ne <= g.hs,
                "rope_prefill_append: rope_ne must be even and <= head_size");
    TORCH_CHECK(cos_t.size(0) >= pos0 + g.T,
                "rope_prefill_append: the rope table has ", cos_t.size(0),
                " rows, pos0 + T = ", pos0 + g.T);
  }
  launch_rope_prefill_append(
      qkv.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
      g.kv8 ? kscale->data_ptr<float>() : nullptr,
      g.kv8 ? vscale->data_ptr<float>() : nullptr,
      rope_ne ? cos_t.data_ptr<float>() : nullptr,
      rope_ne ? sin_t.data_ptr<float>() : nullptr, (int)pos0, (int)slot,
      (int)layer, g.n_layers, g.n_kv, g.max_seq, g.hs, (int)rope_ne, g.qpk,
      g.T, cur_stream());
}

void prefill_attn(torch::Tensor out, torch::Tensor qkv, torch::Tensor kpool,
                  torch::Tensor vpool, int64_t pos0, int64_t slot,
                  int64_t layer, double scale,
                  c10::optional<torch::Tensor> kscale,
                  c10::optional<torch::Tensor> vscale) {
  check_bf16(out, "out");
  const PrefillGeom g = check_prefill("prefill_attn", qkv, kpool, vpool,
                                      kscale, vscale, pos0, slot, layer);
  TORCH_CHECK(out.numel() == (int64_t)g.T * g.n_kv * g.qpk * g.hs,
              "out size");
  int rc = launch_prefill_attn(
      out.data_ptr(), qkv.data_ptr(), kpool.data_ptr(), vpool.data_ptr(),
      g.kv8 ? kscale->data_ptr<float>() : nullptr,
      g.kv8 ? vscale->data_ptr<float>() : nullptr,
      (int)pos0, (int)slot, (int)layer, g.n_layers, g.n_kv, g.max_seq, g.hs,
      g.qpk, g.T, (float)scale, cur_stream());
  TORCH_CHECK(rc == 0, "prefill_attn: unsupported head_size ", g.hs);
}

void add(torch::Tensor out, torch::Tensor a, torch::Tensor b) {
  check_bf16(out, "out");
  check_bf16(a, "a");
  check_bf16(b, "b");
  const int n = (int)a.numel();
  TORCH_CHECK(n % 8 == 0, "n must be a multiple of 8");
  launch_add(out.data_ptr(), a.data_ptr(), b.data_ptr(), n, cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "mdi_llm_amd hand-written CDNA4 (gfx950) decode kernels";
  m.def("rmsnorm", &rmsnorm, "RMSNorm (decode, bf16)");
  m.def("layernorm", &layernorm, "LayerNorm (decode, bf16)");
  m.def("gemv", &gemv, "decode GEMV out = W@norm?(x) (+bias)(+res)(act)",
        py::arg("out"), py::arg("W"), py::arg("x"), py::arg("bias"),
        py::arg("res"), py::arg("epilogue"),
        py::arg("norm_w") = c10::nullopt, py::arg("norm_b") = c10::nullopt,
        py::arg("norm_kind") = 0, py::arg("eps") = 1e-5,
        py::arg("rows") = 0, py::arg("eidx") = c10::nullopt,
        py::arg("estride") = 0);
  m.def("gemv_fp8", &gemv_fp8,
        "decode GEMV with fp8(e4m3) weights + per-row scales",
        py::arg("out"), py::arg("W"), py::arg("wscale"), py::arg("x"),
        py::arg("bias"), py::arg("res"), py::arg("epilogue"),
        py::arg("norm_w") = c10::nullopt, py::arg("norm_b") = c10::nullopt,
        py::arg("norm_kind") = 0, py::arg("eps") = 1e-5,
        py::arg("rows") = 0, py::arg("eidx") = c10::nullopt,
        py::arg("estride") = 0);
  m.def("gemv_swiglu_fp8", &gemv_swiglu_fp8,
        "fused SwiGLU pair GEMV with fp8 weights",
        py::arg("out"), py::arg("Wg"), py::arg("gscale"), py::arg("Wu"),
        py::arg("uscale"), py::arg("x"), py::arg("gelu_gate"),
        py::arg("norm_w") = c10::nullopt, py::arg("norm_b") = c10::nullopt,
        py::arg("norm_kind") = 0, py::arg("eps") = 1e-5,
        py::arg("eidx") = c10::nullopt, py::arg("estride") = 0,
        py::arg("escale") = c10::nullopt);
  m.def("gemv_int4", &gemv_int4,
        "decode GEMV with int4 group-quantized weights (128-group bf16 "
        "scale/zero)",
        py::arg("out"), py::arg("W"), py::arg("qparams"), py::arg("x"),
        py::arg("bias"), py::arg("res"), py::arg("epilogue"),
        py::arg("norm_w") = c10::nullopt, py::arg("norm_b") = c10::nullopt,
        py::arg("norm_kind") = 0, py::arg("eps") = 1e-5,
        py::arg("rows") = 0);
  m.def("gemv_swiglu_int4", &gemv_swiglu_int4,
        "fused SwiGLU pair GEMV with int4 group-quantized weights",
        py::arg("out"), py::arg("Wg"), py::arg("gq"), py::arg("Wu"),
        py::arg("uq"), py::arg("x"), py::arg("gelu_gate"),
        py::arg("norm_w") = c10::nullopt, py::arg("norm_b") = c10::nullopt,
        py::arg("norm_kind") = 0, py::arg("eps") = 1e-5);
  m.def("gemv_swiglu", &gemv_swiglu, "fused SwiGLU pair GEMV (+pre-norm)",
        py::arg("out"), py::arg("Wg"), py::arg("Wu"), py::arg("x"),
        py::arg("gelu_gate"), py::arg("norm_w") = c10::nullopt,
        py::arg("norm_b") = c10::nullopt, py::arg("norm_kind") = 0,
        py::arg("eps") = 1e-5, py::arg("eidx") = c10::nullopt,
        py::arg("estride") = 0, py::arg("escale") = c10::nullopt);
  m.def("swiglu_mul", &swiglu_mul,
        "batched act(gate)*up elementwise (out may alias up)",
        py::arg("out"), py::arg("g"), py::arg("u"), py::arg("gelu_gate"));
  m.def("moe_gate_topk", &moe_gate_topk,
        "MoE router: top-k experts + softmax weights over the k",
        py::arg("eidx"), py::arg("escale"), py::arg("logits"), py::arg("k"));
  m.def("moe_route_group", &moe_route_group,
        "grouped MoE router: per-token top-k + softmax and the "
        "expert-major row layout (count/offset/perm/inv)",
        py::arg("eidx"), py::arg("escale"), py::arg("count"),
        py::arg("offset"), py::arg("perm"), py::arg("inv"),
        py::arg("logits"), py::arg("k"));
  m.def("moe_group_swiglu", &moe_group_swiglu,
        "grouped MoE gate/up MFMA GEMM pair + SwiGLU * routing weight over "
        "the permuted rows",
        py::arg("act"), py::arg("Wg"), py::arg("Wu"), py::arg("X"),
        py::arg("count"), py::arg("offset"), py::arg("perm"),
        py::arg("escale"), py::arg("k"));
  m.def("moe_group_down", &moe_group_down,
        "grouped MoE down MFMA GEMM over the permuted rows (fp32 out)",
        py::arg("D"), py::arg("Wd"), py::arg("act"), py::arg("count"),
        py::arg("offset"), py::arg("n_tokens"));
  m.def("moe_group_swiglu_fp8", &moe_group_swiglu_fp8,
        "moe_group_swiglu with fp8(e4m3) slabs + fp32 row scales [n_e, M]",
        py::arg("act"), py::arg("Wg"), py::arg("gscale"), py::arg("Wu"),
        py::arg("uscale"), py::arg("X"), py::arg("count"),
        py::arg("offset"), py::arg("perm"), py::arg("escale"), py::arg("k"));
  m.def("moe_group_down_fp8", &moe_group_down_fp8,
        "moe_group_down with an fp8(e4m3) slab + fp32 row scales [n_e, M]",
        py::arg("D"), py::arg("Wd"), py::arg("dscale"), py::arg("act"),
        py::arg("count"), py::arg("offset"), py::arg("n_tokens"));
  m.def("moe_group_combine", &moe_group_combine,
        "out[b] = res[b] + sum over ranks of the token's expert rows",
        py::arg("out"), py::arg("res"), py::arg("D"), py::arg("inv"),
        py::arg("k"));
  m.def("moe_route_prefill", &moe_route_prefill,
        "MoE prefill router: moe_route_group's outputs and layout for any "
        "T with T*k <= 65536 (multi-block)",
        py::arg("eidx"), py::arg("escale"), py::arg("count"),
        py::arg("offset"), py::arg("perm"), py::arg("inv"),
        py::arg("logits"), py::arg("k"));
  m.def("moe_prefill_gather", &moe_prefill_gather,
        "XG[s] = hn[perm[s] / k]",
        py::arg("XG"), py::arg("hn"), py::arg("perm"), py::arg("k"));
  m.def("moe_prefill_act", &moe_prefill_act,
        "ACT[s] = silu(G[s]) * U[s] * escale[perm[s]], one bf16 rounding",
        py::arg("ACT"), py::arg("G"), py::arg("U"), py::arg("escale"),
        py::arg("perm"));
  m.def("moe_prefill_combine", &moe_prefill_combine,
        "out[t] = res[t] + sum over ranks of the token's bf16 expert rows",
        py::arg("out"), py::arg("res"), py::arg("D"), py::arg("inv"),
        py::arg("k"));
  m.def("embed", &embed, "embedding row gather");
  m.def("rope_kv_append", &rope_kv_append,
        "RoPE on interleaved qkv + KV cache append");
  m.def("attn_decode", &attn_decode,
        "GQA flash-decode attention (split-S, fused rope+append)",
        py::arg("out"), py::arg("part_o"), py::arg("part_ml"),
        py::arg("qkv"), py::arg("kpool"), py::arg("vpool"), py::arg("cos"),
        py::arg("sin"), py::arg("pos"), py::arg("slot"), py::arg("layer"),
        py::arg("n_chunks"), py::arg("scale"), py::arg("n_batch") = 0,
        py::arg("kscale") = c10::nullopt, py::arg("vscale") = c10::nullopt,
        py::arg("force_split") = 0);
  m.def("add", &add, "bf16 residual add");
  m.def("rope_prefill_append", &rope_prefill_append,
        "prefill: rope q/k for T positions + append k/v to the pool",
        py::arg("qkv"), py::arg("kpool"), py::arg("vpool"), py::arg("cos"),
        py::arg("sin"), py::arg("pos0"), py::arg("slot"), py::arg("layer"),
        py::arg("kscale") = c10::nullopt, py::arg("vscale") = c10::nullopt);
  m.def("prefill_attn", &prefill_attn,
        "causal GQA prefill flash attention (MFMA, online softmax)",
        py::arg("out"), py::arg("qkv"), py::arg("kpool"), py::arg("vpool"),
        py::arg("pos0"), py::arg("slot"), py::arg("layer"),
        py::arg("scale"), py::arg("kscale") = c10::nullopt,
        py::arg("vscale") = c10::nullopt);
  m.def("attn_proj", &attn_proj,
        "fused GQA flash-decode attention + output projection (one "
        "launch; in-launch granule hand-off overlaps the proj weight "
        "stream with attention)",
        py::arg("out"), py::arg("qkv"), py::arg("kpool"), py::arg("vpool"),
        py::arg("cos"), py::arg("sin"), py::arg("pos"), py::arg("slot"),
        py::arg("layer"), py::arg("scale"), py::arg("W"),
        py::arg("bias"), py::arg("res"), py::arg("gran"));
  m.def("sample", &sample,
        "fused temperature/top-k/gumbel token sampling (128k vocab ~15us)",
        py::arg("out_token"), py::arg("logits"), py::arg("scratch"),
        py::arg("temperature"), py::arg("top_k"), py::arg("noise"),
        py::arg("seed"), py::arg("pos") = c10::nullopt,
        py::arg("slot") = c10::nullopt, py::arg("n_batch") = 0,
        py::arg("top_p") = 1.0, py::arg("token_table") = c10::nullopt,
        py::arg("pos_table") = c10::nullopt,
        py::arg("adv_slot") = c10::nullopt, py::arg("adv_pos") = 0,
        py::arg("pos_bias") = 0);
  m.def("mtile_gemm", &mtile_gemm,
        "grouped-decode M-tile MFMA GEMM (bulk LDS-staged X, nt W stream)",
        py::arg("Y"), py::arg("W"), py::arg("X"), py::arg("bias"),
        py::arg("res"));
  m.def("route_env", &route_env,
        "device-side envelope routing (slot from header, dummy on stop)",
        py::arg("hdr"), py::arg("slot_out"), py::arg("pos_table"),
        py::arg("dummy_slot"));
  m.def("stage_slot", &stage_slot,
        "one-launch step staging/bookkeeping on device scalars",
        py::arg("slot"), py::arg("pos_out") = c10::nullopt,
        py::arg("token_out") = c10::nullopt,
        py::arg("pos_table") = c10::nullopt,
        py::arg("token_table") = c10::nullopt,
        py::arg("pos_table_mut") = c10::nullopt, py::arg("adv_pos") = 0);
}
