// PyTorch-ROCm custom-op layer over the C ABI (include/tooncrafter_hip.h):  TORCH_LIBRARY(tooncrafter, ...)
//
// The reference binds ATen / xformers operators from Python (utils/utils.py:27-42 instantiates lvdm classes whose
// forward methods call torch ops); this registers the MI355X kernels as first-class torch operators instead:
//   torch.ops.tooncrafter.gemm / quant_mxfp8 / gemm_mx / attention / attention_temporal(_rel) / groupnorm(_pf) / layernorm(_pf) / ddim_step(_eps) / ddim_step_ms(_eps) / ddim_blend /
//   frames_from_u8 / frames_from_yuv / frames_to_u8 / frames_to_yuv / colour_stats / colour_match / colour_hist / colour_transfer / colour_match_knots / colour_transfer_knots / clip_patches / randn_clips /
//   ff_geglu_fused / temporal_attn_fused / temporal_qkv_attn / attention_q8
// Every operator is ONE function, registered under the CUDA(HIP) key and the Meta key alike (register_ops below).  In order, it
//   1. runs every check that needs only sizes, strides, dtypes, devices and host scalars (pure host calls of the C ABI included),
//   2. allocates its result(s) from the options of its first tensor: the caching allocator on the device, a meta tensor on Meta,
//   3. returns here if that tensor is meta: shape / dtype inference, so the ops trace, export and shape-check without a GPU and the
//      Meta key refuses, in the same words, exactly what the CUDA key refuses,
//   4. marshals the pointers, runs the checks that need a pointer or ask the library (alignment, tc_gemm_ws_eligible, tc_*_workspace),
//      picks up the CURRENT stream and calls the same extern "C" entry point the ctypes binding calls.
// Host C++ only: the kernels live in libtooncrafter_hip.so, which this library links.
// Built by tooncrafter_amd/build.py (build_torch_ops) with the host compiler.  This is the default binding
// (tooncrafter_amd/torch_ops.py; TC_BINDING=ctypes selects the other): DESIGN.md section 1 measures the two launch paths as
// equivalent at these shapes.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "tooncrafter_hip.h"

namespace {

using at::Tensor;
using c10::optional;

void* cur_stream() { return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream().stream()); }

void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed with code ", rc,
              rc < 0 ? " (TC_E*: -1 invalid, -2 alignment, -3 unsupported shape, -4 workspace)" : " (hipError_t)");
}

const tc_bf16* bf(const Tensor& t) { return reinterpret_cast<const tc_bf16*>(t.data_ptr()); }
float* f32_or_null(const optional<Tensor>& t) { return t.has_value() ? t->data_ptr<float>() : nullptr; }

// stream-ordered scratch of nbytes on the device of `like`: never empty, so that its pointer is one
Tensor workspace(int64_t nbytes, const Tensor& like) {
  return at::empty({nbytes > 16 ? nbytes : 16}, like.options().dtype(at::kByte));
}

// "ask for the workspace bytes, allocate, set the pointer, launch, check" for a params struct that carries its workspace
template <typename P>
void launch_ws(P& p, const Tensor& like, int64_t (*bytes)(const P*), int (*entry)(const P*, void*), const char* what) {
  p.workspace_bytes = bytes(&p);
  Tensor ws = workspace(p.workspace_bytes, like);
  p.workspace = ws.data_ptr();
  check_rc(entry(&p, cur_stream()), what);
}

// The device rule of every operator: a tensor is on the device of the operator's first tensor, and that device is CUDA, or meta for
// shape inference.  (The dispatcher refuses CPU tensors alone; one CPU tensor among CUDA ones reaches the CUDA key.)
bool on_device(const Tensor& t, const Tensor& first) { return t.device() == first.device() && (first.is_cuda() || first.is_meta()); }

// The one "on the device, of dtype dt, with this layout" statement; an absent optional tensor fits.
enum Layout { kRows, kDense };   // 2-D with unit column stride (column slices of a wider tensor do) / contiguous
bool fits1(const Tensor& t, const Tensor& first, at::ScalarType dt, Layout lay) {
  return on_device(t, first) && t.scalar_type() == dt && (lay == kRows ? t.dim() == 2 && t.stride(1) == 1 : t.is_contiguous());
}
bool fits1(const optional<Tensor>& t, const Tensor& first, at::ScalarType dt, Layout lay) {
  return !t.has_value() || fits1(*t, first, dt, lay);
}
template <typename... T>
bool fits(const Tensor& first, at::ScalarType dt, Layout lay, const T&... ts) { return (fits1(ts, first, dt, lay) && ...); }

void check_fits(const Tensor& t, const Tensor& first, const char* name, at::ScalarType dt = at::kBFloat16, Layout lay = kRows) {
  TORCH_CHECK(on_device(t, first), name, ": expected a CUDA tensor (the product path is GPU-only)");
  TORCH_CHECK(fits(first, dt, lay, t), name,
              lay == kRows ? ": expected a 2-D rows tensor with unit column stride and dtype " : ": expected a contiguous CUDA tensor of dtype ", dt);
}

// rows [m, c] in, rows [m, c] out: a packed result whatever the row stride of x (empty_like would keep it)
Tensor rows_like(const Tensor& x) { return at::empty({x.size(0), x.size(1)}, x.options()); }

// conv = [] (linear) or [kind (1 = 3x3, 2 = t3), cin, frames, t_len, h_in, w_in, h_out, w_out, stride, upsample, pad]
struct GemmGeom { int64_t m, n, n_out, k; };

// every check of a GEMM request but those of a and w themselves (their dtype differs between the bf16 and the MXFP8 op), which
// come first: the geometry is read off their two dimensions
GemmGeom gemm_request(const Tensor& a, const Tensor& w, const optional<Tensor>& bias, const optional<Tensor>& residual,
                      const optional<Tensor>& row_bias, int64_t row_div, int64_t act, at::IntArrayRef conv) {
  TORCH_CHECK(conv.empty() || conv.size() == 11, "gemm: conv must be empty or 11 integers");
  GemmGeom g;
  g.n = w.size(0);
  g.k = w.size(1);
  g.n_out = act == TC_ACT_GEGLU ? g.n / 2 : g.n;
  g.m = conv.empty() ? a.size(0) : conv[2] * conv[6] * conv[7];
  TORCH_CHECK(fits(a, at::kFloat, kDense, bias) && (!bias.has_value() || bias->numel() == g.n), "gemm: bias must be a contiguous fp32 CUDA [N]");
  if (row_bias.has_value()) {
    check_fits(*row_bias, a, "gemm: row_bias", at::kFloat);
    TORCH_CHECK(row_div > 0 && row_bias->size(1) == g.n && row_bias->size(0) * row_div >= g.m, "gemm: row_bias / row_div do not cover M");
  }
  if (residual.has_value()) {
    check_fits(*residual, a, "gemm: residual");
    TORCH_CHECK(residual->size(1) == g.n_out && residual->size(0) >= g.m, "gemm: residual shape mismatch");
  }
  TORCH_CHECK(!conv.empty() || a.size(1) >= g.k, "gemm: A has fewer columns than the weight's K");
  TORCH_CHECK(conv.empty() || (a.size(0) >= conv[2] * conv[4] * conv[5] && a.size(1) >= conv[1]), "gemm: conv source too small for its geometry");
  return g;
}

// fills everything of TcGemmParams except a / w / lda / ldw (operand dtype differs between the bf16 and MXFP8 ops)
void fill_gemm(TcGemmParams& p, const GemmGeom& g, Tensor& out, const optional<Tensor>& bias, const optional<Tensor>& residual,
               const optional<Tensor>& row_bias, int64_t row_div, int64_t act, double alpha, double out_scale, bool out_f32,
               at::IntArrayRef conv) {
  p.c = out.data_ptr();
  p.m = (int32_t)g.m; p.n = (int32_t)g.n; p.k = (int32_t)g.k;
  p.ldc = (int32_t)out.stride(0);
  p.alpha = (float)alpha; p.out_scale = (float)out_scale; p.act = (int32_t)act; p.out_f32 = out_f32 ? 1 : 0;
  p.batch = 1;
  if (bias.has_value()) p.bias = bias->data_ptr<float>();
  if (row_bias.has_value()) {
    p.row_bias = row_bias->data_ptr<float>(); p.ldrb = (int32_t)row_bias->stride(0); p.row_div = (int32_t)row_div;
  }
  if (residual.has_value()) {
    p.residual = bf(*residual); p.ldr = (int32_t)residual->stride(0);
  }
  if (conv.empty()) {
    p.gather = TC_GATHER_LINEAR;
  } else {
    p.gather = conv[0] == 1 ? TC_GATHER_CONV3x3 : TC_GATHER_CONVT3;
    p.cin = (int32_t)conv[1]; p.frames = (int32_t)conv[2]; p.t_len = (int32_t)conv[3];
    p.h_in = (int32_t)conv[4]; p.w_in = (int32_t)conv[5]; p.h_out = (int32_t)conv[6]; p.w_out = (int32_t)conv[7];
    p.stride = (int32_t)conv[8]; p.upsample = (int32_t)conv[9]; p.pad = (int32_t)conv[10];
  }
}

Tensor gemm(const Tensor& a, const Tensor& w, const optional<Tensor>& bias, const optional<Tensor>& residual,
            const optional<Tensor>& row_bias, int64_t row_div, int64_t act, double alpha, double out_scale, bool out_f32,
            at::IntArrayRef conv, double a_norm_eps) {
  check_fits(a, a, "gemm: a");
  check_fits(w, a, "gemm: w");
  const GemmGeom g = gemm_request(a, w, bias, residual, row_bias, row_div, act, conv);
  Tensor out = at::empty({g.m, g.n_out}, a.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  if (a.is_meta()) return out;
  TcGemmParams p = {};
  p.a = bf(a); p.w = bf(w);
  p.lda = (int32_t)a.stride(0); p.ldw = (int32_t)w.stride(0);
  fill_gemm(p, g, out, bias, residual, row_bias, row_div, act, alpha, out_scale, out_f32, conv);
  if (a_norm_eps >= 0.0) {                 // ABI 8: LayerNorm of the A rows as a prologue (affine part folded into w / bias)
    p.a_norm = 1; p.a_norm_eps = (float)a_norm_eps;
    TORCH_CHECK(tc_gemm_ws_eligible(&p) == 1, "gemm: a_norm_eps needs a problem the weight-stationary kernel takes");
  }
  Tensor ws;                               // only where the route asks for one: a null workspace otherwise, as through ctypes
  const int64_t nbytes = tc_gemm_workspace(&p);
  if (nbytes > 0) {
    ws = at::empty({nbytes}, a.options().dtype(at::kByte));
    p.workspace = ws.data_ptr(); p.workspace_bytes = nbytes;
  }
  check_rc(tc_gemm_bf16(&p, cur_stream()), "tc_gemm_bf16");
  return out;
}

// MXFP8 pair (ABI 7, BASELINE.json configs[4]): bf16 rows -> (e4m3 bytes, E8M0 scales); GEMM over such operands
std::tuple<Tensor, Tensor> quant_mxfp8(const Tensor& x, int64_t k) {
  check_fits(x, x, "quant_mxfp8: x");
  TORCH_CHECK(k > 0 && k % 32 == 0 && x.size(1) >= k, "quant_mxfp8: k must be a multiple of 32 and <= the columns of x");
  const int64_t rows = x.size(0), lds = (k + 127) / 128 * 4;
  Tensor q = at::empty({rows, k}, x.options().dtype(at::kByte));
  Tensor s = at::empty({rows, lds}, x.options().dtype(at::kByte));
  if (x.is_meta()) return {q, s};
  check_rc(tc_quant_mxfp8(bf(x), rows, (int32_t)k, (int32_t)x.stride(0), q.data_ptr<uint8_t>(), (int32_t)q.stride(0),
                          s.data_ptr<uint8_t>(), (int32_t)lds, cur_stream()), "tc_quant_mxfp8");
  return {q, s};
}

Tensor gemm_mx(const Tensor& aq, const Tensor& a_scale, const Tensor& wq, const Tensor& w_scale, const optional<Tensor>& bias,
               const optional<Tensor>& residual, const optional<Tensor>& row_bias, int64_t row_div, int64_t act, double alpha,
               double out_scale, bool out_f32, at::IntArrayRef conv) {
  check_fits(aq, aq, "gemm_mx: a", at::kByte); check_fits(wq, aq, "gemm_mx: w", at::kByte);
  check_fits(a_scale, aq, "gemm_mx: a_scale", at::kByte); check_fits(w_scale, aq, "gemm_mx: w_scale", at::kByte);
  TORCH_CHECK(a_scale.size(0) == aq.size(0) && w_scale.size(0) == wq.size(0), "gemm_mx: one scale row per operand row");
  const GemmGeom g = gemm_request(aq, wq, bias, residual, row_bias, row_div, act, conv);
  Tensor out = at::empty({g.m, g.n_out}, aq.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  if (aq.is_meta()) return out;
  TcGemmMxParams px = {};
  px.g.a = bf(aq); px.g.w = bf(wq);
  px.g.lda = (int32_t)aq.stride(0); px.g.ldw = (int32_t)wq.stride(0);
  fill_gemm(px.g, g, out, bias, residual, row_bias, row_div, act, alpha, out_scale, out_f32, conv);
  px.a_scale = a_scale.data_ptr<uint8_t>(); px.lda_s = (int32_t)a_scale.stride(0);
  px.w_scale = w_scale.data_ptr<uint8_t>(); px.ldw_s = (int32_t)w_scale.stride(0);
  check_rc(tc_gemm_mxfp8(&px, cur_stream()), "tc_gemm_mxfp8");
  return out;
}

// what TcAttnParams and TcAttnQ8Params share: the q / k / v / o pointers with their row and batch strides, the problem, the scale
template <typename P>
void attn_fill(P& p, const Tensor& q, const Tensor& k, const Tensor& v, Tensor& out, int64_t batch, int64_t heads, int64_t lq,
               int64_t lk, double scale) {
  p.q = bf(q); p.k = bf(k); p.v = bf(v); p.o = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.batch = (int32_t)batch; p.heads = (int32_t)heads; p.lq = (int32_t)lq; p.lk = (int32_t)lk;
  p.q_ss = (int32_t)q.stride(0); p.k_ss = (int32_t)k.stride(0); p.v_ss = (int32_t)v.stride(0); p.o_ss = (int32_t)out.stride(0);
  p.q_sb = lq * q.stride(0); p.k_sb = lk * k.stride(0); p.v_sb = lk * v.stride(0); p.o_sb = lq * out.stride(0);
  p.scale = (float)scale;
}

Tensor attention(const Tensor& q, const Tensor& k, const Tensor& v, int64_t batch, int64_t heads, int64_t lq, int64_t lk,
                 int64_t kv_bdiv, double scale, const optional<Tensor>& k2, const optional<Tensor>& v2, int64_t lk2, int64_t kv2_bdiv) {
  check_fits(q, q, "attention: q"); check_fits(k, q, "attention: k"); check_fits(v, q, "attention: v");
  const int64_t hd = heads * 64;
  TORCH_CHECK(q.size(0) == batch * lq && q.size(1) == hd && k.size(1) == hd && v.size(1) == hd, "attention: head layout mismatch");
  TORCH_CHECK(kv_bdiv > 0, "attention: kv_bdiv ", kv_bdiv);
  const int64_t kvb = (batch + kv_bdiv - 1) / kv_bdiv;
  TORCH_CHECK(k.size(0) == kvb * lk && v.size(0) == kvb * lk, "attention: K/V rows != kv_batches * lk");
  if (k2.has_value()) {
    TORCH_CHECK(v2.has_value() && lk2 > 0 && kv2_bdiv > 0, "attention: second K/V set incomplete");
    check_fits(*k2, q, "attention: k2"); check_fits(*v2, q, "attention: v2");
    const int64_t kvb2 = (batch + kv2_bdiv - 1) / kv2_bdiv;
    TORCH_CHECK(k2->size(0) == kvb2 * lk2 && v2->size(0) == kvb2 * lk2 && k2->size(1) == hd && v2->size(1) == hd,
                "attention: second K/V set must be [(batch / kv2_bdiv) * lk2, heads * 64]");
  }
  Tensor out = at::empty({batch * lq, hd}, q.options());
  if (q.is_meta()) return out;
  TcAttnParams p = {};
  attn_fill(p, q, k, v, out, batch, heads, lq, lk, scale);
  p.kv_bdiv = (int32_t)kv_bdiv;
  if (k2.has_value()) {
    p.k2 = bf(*k2); p.v2 = bf(*v2); p.lk2 = (int32_t)lk2; p.kv2_bdiv = (int32_t)kv2_bdiv;
    p.k2_ss = (int32_t)k2->stride(0); p.v2_ss = (int32_t)v2->stride(0);
    p.k2_sb = lk2 * k2->stride(0); p.v2_sb = lk2 * v2->stride(0);
  }
  check_rc(tc_attn_d64(&p, cur_stream()), "tc_attn_d64");
  return out;
}

// ABI 14: the 8-bit self-attention -- K / V quantised into a workspace from the caching allocator, then the attention
Tensor attention_q8(const Tensor& q, const Tensor& k, const Tensor& v, int64_t batch, int64_t heads, int64_t lq, int64_t lk,
                    double scale) {
  check_fits(q, q, "attention_q8: q"); check_fits(k, q, "attention_q8: k"); check_fits(v, q, "attention_q8: v");
  const int64_t hd = heads * 64;
  TORCH_CHECK(q.size(0) == batch * lq && q.size(1) == hd && k.size(0) == batch * lk && k.size(1) == hd &&
              v.size(0) == batch * lk && v.size(1) == hd,
              "attention_q8: q must be [batch*lq, heads*64], k and v [batch*lk, heads*64]");
  Tensor out = at::empty({batch * lq, hd}, q.options());
  if (q.is_meta()) return out;
  TcAttnQ8Params p = {};
  attn_fill(p, q, k, v, out, batch, heads, lq, lk, scale);
  const int64_t nbytes = tc_attn_q8_workspace(&p);
  Tensor ws = workspace(nbytes, q);        // two launches share it, so not launch_ws
  p.workspace = ws.data_ptr(); p.workspace_bytes = ws.numel();
  check_rc(tc_attn_q8_quant_kv(&p, cur_stream()), "tc_attn_q8_quant_kv");
  check_rc(tc_attn_d64_q8(&p, cur_stream()), "tc_attn_d64_q8");
  return out;
}

Tensor attention_temporal(const Tensor& qkv, int64_t b, int64_t t, int64_t hw, int64_t heads, double scale) {
  check_fits(qkv, qkv, "attention_temporal: qkv");
  TORCH_CHECK(qkv.is_contiguous() && qkv.size(0) == b * t * hw && qkv.size(1) == 3 * heads * 64,
              "attention_temporal: qkv must be contiguous [b*t*hw, 3*heads*64]");
  Tensor out = at::empty({b * t * hw, heads * 64}, qkv.options());
  if (qkv.is_meta()) return out;
  check_rc(tc_attn_temporal(bf(qkv), reinterpret_cast<tc_bf16*>(out.data_ptr()), (int32_t)b, (int32_t)t, (int32_t)hw,
                            (int32_t)heads, (float)scale, cur_stream()), "tc_attn_temporal");
  return out;
}

// tc_attn_temporal_rel: relative position and / or a causal mask on the temporal attention (reference attention.py:20-39,
// 103-124, 343-345, 376-390).  rel_k / rel_v: [2*max_rel + 1, 64] bf16, or both absent.
Tensor attention_temporal_rel(const Tensor& qkv, const optional<Tensor>& rel_k, const optional<Tensor>& rel_v, int64_t b, int64_t t,
                              int64_t hw, int64_t heads, int64_t max_rel, bool causal, double scale) {
  check_fits(qkv, qkv, "attention_temporal_rel: qkv");
  TORCH_CHECK(qkv.is_contiguous() && qkv.size(0) == b * t * hw && qkv.size(1) == 3 * heads * 64,
              "attention_temporal_rel: qkv must be contiguous [b*t*hw, 3*heads*64]");
  for (const optional<Tensor>* tab : {&rel_k, &rel_v})
    if (tab->has_value()) {
      check_fits(**tab, qkv, "attention_temporal_rel: table");
      TORCH_CHECK((*tab)->is_contiguous() && (*tab)->size(0) == 2 * max_rel + 1 && (*tab)->size(1) == 64,
                  "attention_temporal_rel: a table must be contiguous [2*max_rel + 1, 64]");
    }
  Tensor out = at::empty({b * t * hw, heads * 64}, qkv.options());
  if (qkv.is_meta()) return out;
  TcAttnTemporalRelParams p{};
  p.qkv = bf(qkv);
  p.out = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.rel_k = rel_k.has_value() ? bf(*rel_k) : nullptr;
  p.rel_v = rel_v.has_value() ? bf(*rel_v) : nullptr;
  p.b = (int32_t)b; p.t = (int32_t)t; p.hw = (int32_t)hw; p.heads = (int32_t)heads;
  p.max_rel = (int32_t)max_rel; p.causal = causal ? 1 : 0;
  p.scale = (float)scale;
  check_rc(tc_attn_temporal_rel(&p, cur_stream()), "tc_attn_temporal_rel");
  return out;
}

// ABI 12: the consumer's weights (read-only tensors on the device, contiguous) as a prefetch list for the norm's extra blocks
void prefetch_check(at::TensorList ts, const Tensor& first, const char* what) {
  TORCH_CHECK((int64_t)ts.size() <= TC_PREFETCH_MAX, what, ": at most ", TC_PREFETCH_MAX, " prefetch tensors");
  for (const Tensor& t : ts)
    TORCH_CHECK(on_device(t, first) && t.is_contiguous(), what, ": prefetch tensors must be contiguous CUDA tensors");
}

TcPrefetch prefetch_of(at::TensorList ts) {
  TcPrefetch pf = {};
  for (const Tensor& t : ts) {
    pf.ptr[pf.n] = t.data_ptr();
    pf.bytes[pf.n] = (int64_t)t.numel() * (int64_t)t.element_size();
    ++pf.n;
  }
  return pf;
}

Tensor groupnorm_pf(const Tensor& x, const Tensor& gamma, const Tensor& beta, int64_t samples, int64_t rows, double eps, bool silu,
                    at::TensorList prefetch) {
  check_fits(x, x, "groupnorm_pf: x");
  const int64_t c = x.size(1);
  TORCH_CHECK(x.is_contiguous() && x.size(0) == samples * rows, "groupnorm_pf: x must be contiguous [samples*rows, C]");
  TORCH_CHECK(fits(x, at::kFloat, kDense, gamma, beta) && gamma.numel() == c && beta.numel() == c,
              "groupnorm_pf: gamma / beta must be contiguous fp32 CUDA [C]");
  prefetch_check(prefetch, x, "groupnorm_pf");
  Tensor y = at::empty_like(x);
  if (x.is_meta()) return y;
  const TcPrefetch pf = prefetch_of(prefetch);
  const int64_t nbytes = tc_groupnorm_workspace((int32_t)samples, (int32_t)rows, (int32_t)c);
  Tensor ws = workspace(nbytes, x);
  check_rc(tc_groupnorm_pf(bf(x), reinterpret_cast<tc_bf16*>(y.data_ptr()), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                           (int32_t)samples, (int32_t)rows, (int32_t)c, (float)eps, silu ? 1 : 0, ws.data_ptr(), nbytes, &pf, cur_stream()),
           "tc_groupnorm_pf");
  return y;
}

Tensor layernorm_pf(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps, at::TensorList prefetch) {
  check_fits(x, x, "layernorm_pf: x");
  const int64_t c = x.size(1);
  TORCH_CHECK(x.is_contiguous(), "layernorm_pf: x must be contiguous");
  TORCH_CHECK(fits(x, at::kFloat, kDense, gamma, beta) && gamma.numel() == c && beta.numel() == c,
              "layernorm_pf: gamma / beta must be contiguous fp32 CUDA [C]");
  prefetch_check(prefetch, x, "layernorm_pf");
  Tensor y = at::empty_like(x);
  if (x.is_meta()) return y;
  const TcPrefetch pf = prefetch_of(prefetch);
  check_rc(tc_layernorm_pf(bf(x), reinterpret_cast<tc_bf16*>(y.data_ptr()), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                           (int32_t)x.size(0), (int32_t)c, (float)eps, &pf, cur_stream()), "tc_layernorm_pf");
  return y;
}

// groupnorm / layernorm are their _pf forms with an empty list: an empty TcPrefetch launches what a NULL one launches
Tensor groupnorm(const Tensor& x, const Tensor& gamma, const Tensor& beta, int64_t samples, int64_t rows, double eps, bool silu) {
  return groupnorm_pf(x, gamma, beta, samples, rows, eps, silu, {});
}

Tensor layernorm(const Tensor& x, const Tensor& gamma, const Tensor& beta, double eps) {
  return layernorm_pf(x, gamma, beta, eps, {});
}

// ---- the level-0 one-launch operators (ABI 9): LayerNorm + GEGLU feed-forward + residual; LayerNorm + temporal self-attention +
// residual (lvdm/modules/attention.py:81-144,225-246,415-442).  ln_eps < 0: x is taken as already normalised.
Tensor ff_geglu_fused(const Tensor& x, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2, double ln_eps) {
  check_fits(x, x, "ff_geglu_fused: x");
  check_fits(w1, x, "ff_geglu_fused: w1", at::kBFloat16, kDense); check_fits(w2, x, "ff_geglu_fused: w2", at::kBFloat16, kDense);
  check_fits(b1, x, "ff_geglu_fused: b1", at::kFloat, kDense); check_fits(b2, x, "ff_geglu_fused: b2", at::kFloat, kDense);
  const int64_t m = x.size(0), c = x.size(1);
  TORCH_CHECK(w2.dim() == 2 && w1.dim() == 2, "ff_geglu_fused: w1 [2 hidden, c], w2 [c, hidden]");
  const int64_t hidden = w2.size(1);
  TORCH_CHECK(w1.size(0) == 2 * hidden && w1.size(1) == c && w2.size(0) == c && b1.numel() == 2 * hidden && b2.numel() == c,
              "ff_geglu_fused: x [m, c] rows, w1 [2 hidden, c], b1 [2 hidden], w2 [c, hidden], b2 [c]");
  Tensor out = rows_like(x);
  if (x.is_meta()) return out;
  TcFfParams p{};
  p.x = bf(x); p.w1 = bf(w1); p.b1 = b1.data_ptr<float>(); p.w2 = bf(w2); p.b2 = b2.data_ptr<float>();
  p.out = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.m = (int32_t)m; p.c = (int32_t)c; p.hidden = (int32_t)hidden; p.ldx = (int32_t)x.stride(0); p.ldo = (int32_t)c;
  p.ln = ln_eps >= 0.0 ? 1 : 0; p.ln_eps = ln_eps >= 0.0 ? (float)ln_eps : 0.f;
  check_rc(tc_ff_geglu_fused(&p, cur_stream()), "tc_ff_geglu_fused");
  return out;
}

Tensor temporal_attn_fused(const Tensor& x, const Tensor& wqkv, const Tensor& bqkv, const Tensor& wo, const Tensor& bo, int64_t b,
                           int64_t t, int64_t hw, int64_t heads, double ln_eps, double scale) {
  check_fits(x, x, "temporal_attn_fused: x");
  check_fits(wqkv, x, "temporal_attn_fused: wqkv", at::kBFloat16, kDense); check_fits(wo, x, "temporal_attn_fused: wo", at::kBFloat16, kDense);
  check_fits(bqkv, x, "temporal_attn_fused: bqkv", at::kFloat, kDense); check_fits(bo, x, "temporal_attn_fused: bo", at::kFloat, kDense);
  const int64_t m = x.size(0), c = x.size(1);
  TORCH_CHECK(m == b * t * hw && wqkv.dim() == 2 && wqkv.size(0) == 3 * c && wqkv.size(1) == c && wo.dim() == 2 && wo.size(0) == c &&
              wo.size(1) == c && bqkv.numel() == 3 * c && bo.numel() == c && c == heads * 64,
              "temporal_attn_fused: x [b*t*hw, c] rows, wqkv [3c, c], bqkv [3c], wo [c, c], bo [c], c = heads * 64");
  Tensor out = rows_like(x);
  if (x.is_meta()) return out;
  TcTbParams p{};
  p.x = bf(x); p.wqkv = bf(wqkv); p.bqkv = bqkv.data_ptr<float>(); p.wo = bf(wo); p.bo = bo.data_ptr<float>();
  p.out = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.b = (int32_t)b; p.t = (int32_t)t; p.hw = (int32_t)hw; p.c = (int32_t)c; p.heads = (int32_t)heads;
  p.ldx = (int32_t)x.stride(0); p.ldo = (int32_t)c;
  p.ln = ln_eps >= 0.0 ? 1 : 0; p.ln_eps = ln_eps >= 0.0 ? (float)ln_eps : 0.f; p.scale = (float)scale;
  check_rc(tc_temporal_attn_fused(&p, cur_stream()), "tc_temporal_attn_fused");
  return out;
}

// ABI 13: the temporal q / k / v projection and its attention as one launch (csrc/qkv_attn.hip; 17 .. 64 frames: csrc/qkv_attn_long.hip -- any t is passed through, the library decides)
Tensor temporal_qkv_attn(const Tensor& x, const Tensor& wqkv, const optional<Tensor>& bqkv, int64_t b, int64_t t, int64_t hw,
                         int64_t heads, double scale) {
  check_fits(x, x, "temporal_qkv_attn: x");
  check_fits(wqkv, x, "temporal_qkv_attn: wqkv", at::kBFloat16, kDense);
  if (bqkv.has_value()) check_fits(*bqkv, x, "temporal_qkv_attn: bqkv", at::kFloat, kDense);
  const int64_t m = x.size(0), c = x.size(1);
  TORCH_CHECK(m == b * t * hw && wqkv.dim() == 2 && wqkv.size(0) == 3 * c && wqkv.size(1) == c && c == heads * 64 &&
              (!bqkv.has_value() || bqkv->numel() == 3 * c),
              "temporal_qkv_attn: x [b*t*hw, c] rows, wqkv [3c, c], bqkv [3c] or None, c = heads * 64");
  Tensor out = rows_like(x);
  if (x.is_meta()) return out;
  TcTqaParams p{};
  p.x = bf(x); p.wqkv = bf(wqkv); p.bqkv = f32_or_null(bqkv);
  p.out = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.b = (int32_t)b; p.t = (int32_t)t; p.hw = (int32_t)hw; p.c = (int32_t)c; p.heads = (int32_t)heads;
  p.ldx = (int32_t)x.stride(0); p.ldo = (int32_t)c;
  p.scale = (float)scale;
  check_rc(tc_temporal_qkv_attn(&p, cur_stream()), "tc_temporal_qkv_attn");
  return out;
}

// The one step implementation; x_prev and pred_x0 are its two results.  x0_hist is the previous step's pred_x0 or None, and
// without one (or with corr 0) the step is first order (the multistep term is additive within ABI 14).
template <bool EPS>
std::tuple<Tensor, Tensor> ddim_step_ms_any(const Tensor& x, const Tensor& e_cond, const optional<Tensor>& e_uncond,
                                            const optional<Tensor>& noise, const optional<Tensor>& e_uncond_img,
                                            const optional<Tensor>& x0_hist, double corr, double cfg_scale, double cfg_img,
                                            double guidance_rescale, double sqrt_ac, double sqrt_1m_ac, double sqrt_a_prev,
                                            double dir_coef, double sigma, double x0_rescale) {
  TORCH_CHECK(fits(x, at::kFloat, kDense, x, e_cond, e_uncond, noise, e_uncond_img, x0_hist), "ddim_step: contiguous fp32 CUDA tensors");
  TORCH_CHECK(!x0_hist.has_value() || x0_hist->sizes() == x.sizes(), "ddim_step: x0_hist must have the shape of x");
  Tensor x_prev = at::empty_like(x), x0 = at::empty_like(x);
  if (x.is_meta()) return {x_prev, x0};
  TcDdimMsParams mp = {};
  TcDdimParams& p = mp.base;
  p.x = x.data_ptr<float>(); p.e_cond = e_cond.data_ptr<float>();
  p.e_uncond = f32_or_null(e_uncond); p.noise = f32_or_null(noise); p.e_uncond_img = f32_or_null(e_uncond_img);
  p.x_prev = x_prev.data_ptr<float>(); p.pred_x0 = x0.data_ptr<float>();
  p.b = (int32_t)x.size(0); p.n = x.numel() / x.size(0);
  p.cfg_scale = (float)cfg_scale; p.cfg_img = (float)cfg_img; p.guidance_rescale = (float)guidance_rescale;
  p.sqrt_ac = (float)sqrt_ac; p.sqrt_1m_ac = (float)sqrt_1m_ac; p.sqrt_a_prev = (float)sqrt_a_prev;
  p.dir_coef = (float)dir_coef; p.sigma = (float)sigma; p.x0_rescale = (float)x0_rescale;
  mp.x0_hist = f32_or_null(x0_hist);
  mp.corr = (float)corr;
  const int64_t nbytes = tc_ddim_workspace(p.b);
  Tensor ws = workspace(nbytes, x);
  if (EPS)
    check_rc(tc_ddim_step_ms_eps(&mp, ws.data_ptr(), nbytes, cur_stream()), "tc_ddim_step_ms_eps");
  else
    check_rc(tc_ddim_step_ms(&mp, ws.data_ptr(), nbytes, cur_stream()), "tc_ddim_step_ms");
  return {x_prev, x0};
}

// ddim_step / ddim_step_eps: the schema without the two history operands
template <bool EPS>
std::tuple<Tensor, Tensor> ddim_step_any(const Tensor& x, const Tensor& e_cond, const optional<Tensor>& e_uncond,
                                         const optional<Tensor>& noise, const optional<Tensor>& e_uncond_img, double cfg_scale,
                                         double cfg_img, double guidance_rescale, double sqrt_ac, double sqrt_1m_ac,
                                         double sqrt_a_prev, double dir_coef, double sigma, double x0_rescale) {
  return ddim_step_ms_any<EPS>(x, e_cond, e_uncond, noise, e_uncond_img, c10::nullopt, 0.0, cfg_scale, cfg_img, guidance_rescale,
                               sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef, sigma, x0_rescale);
}

// x is optional, so x0 is the operator's first tensor
Tensor ddim_blend(const optional<Tensor>& x, const Tensor& x0, const optional<Tensor>& noise, const optional<Tensor>& mask,
                  double sqrt_ac, double sqrt_1m_ac) {
  auto shaped = [&](const optional<Tensor>& t) { return !t.has_value() || t->sizes() == x0.sizes(); };
  TORCH_CHECK(x0.dim() >= 1 && fits(x0, at::kFloat, kDense, x0, x, noise, mask) && shaped(x) && shaped(noise) && shaped(mask),
              "ddim_blend: contiguous fp32 CUDA tensors of one shape (B, ...)");
  Tensor out = at::empty_like(x0);
  if (x0.is_meta()) return out;
  TcDdimBlendParams p = {};
  p.x = f32_or_null(x); p.x0 = x0.data_ptr<float>(); p.noise = f32_or_null(noise); p.mask = f32_or_null(mask);
  p.out = out.data_ptr<float>();
  p.b = (int32_t)x0.size(0); p.n = p.b ? x0.numel() / x0.size(0) : 0;
  p.sqrt_ac = (float)sqrt_ac; p.sqrt_1m_ac = (float)sqrt_1m_ac;
  check_rc(tc_ddim_blend(&p, cur_stream()), "tc_ddim_blend");
  return out;
}

// Pixel path (additive within ABI 14).  A resample request: per axis the tables of n_in -> n_out (tc_resize_tables /
// tc_resize_tables_filter), on the device, as the C ABI takes them.  n_in == n_out: the pass does not run, its tables are not
// looked at.  Checked in front of the allocation (resize_request), set in the params struct behind it (resize_fill).
struct Resize {   // the tables of the passes that run, null for one that does not
  const Tensor *h_bounds = nullptr, *h_coefs = nullptr, *v_bounds = nullptr, *v_coefs = nullptr;
};

bool resize_axis(const optional<Tensor>& bounds, const optional<Tensor>& coefs, const Tensor& first, int64_t n_in, int64_t n_out,
                 const char* name, const char* axis) {
  if (n_in == n_out) return false;
  for (const auto* t : {&bounds, &coefs})
    TORCH_CHECK(fits(first, at::kInt, kDense, *t) && (!t->has_value() || (*t)->dim() == 2), name, ": ", axis,
                " tables: contiguous int32 CUDA [out, k]");
  // the tables must be the ones of this size: their rows are indexed by the output index
  TORCH_CHECK(bounds.has_value() && coefs.has_value() && bounds->size(0) == n_out && bounds->size(1) == 2 && coefs->size(0) == n_out &&
              coefs->size(1) >= 1, name, ": ", axis, " tables of ", n_in, " -> ", n_out, " expected");
  return true;
}

Resize resize_request(const optional<Tensor>& h_bounds, const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds,
                      const optional<Tensor>& v_coefs, const Tensor& first, int64_t w_in, int64_t w_out, int64_t h_in, int64_t h_out,
                      const char* name) {
  Resize r;
  if (resize_axis(h_bounds, h_coefs, first, w_in, w_out, name, "horizontal")) { r.h_bounds = &*h_bounds; r.h_coefs = &*h_coefs; }
  if (resize_axis(v_bounds, v_coefs, first, h_in, h_out, name, "vertical")) { r.v_bounds = &*v_bounds; r.v_coefs = &*v_coefs; }
  return r;
}

template <typename P>
void resize_fill(P& p, const Resize& r) {
  if (r.h_bounds) {
    p.h_bounds = r.h_bounds->data_ptr<int32_t>(); p.h_coefs = r.h_coefs->data_ptr<int32_t>(); p.h_kmax = (int32_t)r.h_coefs->size(1);
  }
  if (r.v_bounds) {
    p.v_bounds = r.v_bounds->data_ptr<int32_t>(); p.v_coefs = r.v_coefs->data_ptr<int32_t>(); p.v_kmax = (int32_t)r.v_coefs->size(1);
  }
}

// What the two front ends ask besides their source: n images of (sh, sw), image i into frame slots[i] = batch * t + frame of a new
// (b, 3, t, h, w) fp32 clip tensor on the device of `src`, zero elsewhere (reference scripts/evaluation/inference.py:64-69 on the
// device); the tables are tc_resize_tables' for sw -> rw and sh -> rh (None when nothing is resized).  front_request checks that
// and returns the tables; front_fill sets those fields of p, which points at the caller's `slot`.
Resize front_request(const char* name, const Tensor& src, int64_t n, int64_t sh, int64_t sw, at::IntArrayRef slots, int64_t b, int64_t t,
                     int64_t h, int64_t w, const optional<Tensor>& h_bounds, const optional<Tensor>& h_coefs,
                     const optional<Tensor>& v_bounds, const optional<Tensor>& v_coefs) {
  TORCH_CHECK(n >= 1 && n <= TC_FRAMES_U8_MAX && (int64_t)slots.size() == n, name, ": 1 .. ", TC_FRAMES_U8_MAX, " images, one slot each");
  TORCH_CHECK(b > 0 && t > 0 && h > 0 && w > 0, name, ": b, t, h, w must be positive");
  for (int64_t s : slots) TORCH_CHECK(s >= 0 && s < b * t, name, ": slot ", s, " outside the clip tensor");
  int32_t rh = 0, rw = 0;
  check_rc(tc_frames_from_u8_resized((int32_t)sh, (int32_t)sw, (int32_t)h, (int32_t)w, &rh, &rw), "tc_frames_from_u8_resized");
  return resize_request(h_bounds, h_coefs, v_bounds, v_coefs, src, sw, rw, sh, rh, name);
}

template <typename Params>
void front_fill(Params& p, int32_t (&slot)[TC_FRAMES_U8_MAX], Tensor& out, int64_t sh, int64_t sw, at::IntArrayRef slots, const Resize& rs) {
  for (size_t i = 0; i < slots.size(); ++i) slot[i] = (int32_t)slots[i];
  p.n = (int32_t)slots.size(); p.sh = (int32_t)sh; p.sw = (int32_t)sw;
  p.slots = slot;
  p.out = out.data_ptr<float>();
  p.b = (int32_t)out.size(0); p.t = (int32_t)out.size(2); p.h = (int32_t)out.size(3); p.w = (int32_t)out.size(4);
  resize_fill(p, rs);
}

Tensor frames_from_u8(const Tensor& images, at::IntArrayRef slots, int64_t b, int64_t t, int64_t h, int64_t w,
                      const optional<Tensor>& h_bounds, const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds,
                      const optional<Tensor>& v_coefs) {
  TORCH_CHECK(on_device(images, images), "frames_from_u8: expected a CUDA tensor (the product path is GPU-only)");
  TORCH_CHECK(images.scalar_type() == at::kByte && images.dim() == 4 && images.size(3) == 3 && images.stride(3) == 1 &&
              images.stride(2) == 3, "frames_from_u8: uint8 (n, h, w, 3) images with packed pixels");
  const int64_t sh = images.size(1), sw = images.size(2);
  const Resize rs = front_request("frames_from_u8", images, images.size(0), sh, sw, slots, b, t, h, w, h_bounds, h_coefs, v_bounds, v_coefs);
  Tensor out = at::zeros({b, 3, t, h, w}, images.options().dtype(at::kFloat));
  if (images.is_meta()) return out;
  TcFramesU8Params p = {};
  int32_t slot[TC_FRAMES_U8_MAX];
  front_fill(p, slot, out, sh, sw, slots, rs);
  p.src = images.data_ptr<uint8_t>();
  p.pitch = (int32_t)images.stride(1);
  p.image_stride = p.n > 1 ? images.stride(0) : (int64_t)p.sh * p.pitch;
  launch_ws(p, images, tc_frames_from_u8_workspace, tc_frames_from_u8, "tc_frames_from_u8");
  return out;
}

// frames_from_yuv: n planar 4:2:0 images -> a new (b, 3, t, h, w) fp32 clip tensor (tc_frames_from_yuv).  y (n, sh, sw), c0 / c1
// (n, ch, cw) for I420, c0 (n, ch, cw, 2) for NV12 and P010 (2-byte elements); pitches and image strides are the tensors' strides.
std::pair<int64_t, int64_t> plane_rows(const Tensor& p, int64_t row_elems, const char* what) {   // (pitch, image stride) in bytes
  const int64_t es = p.element_size(), n = p.size(0);
  TORCH_CHECK(p.stride(p.dim() - 1) == 1 && (p.dim() == 3 || p.stride(2) == 2) && p.stride(1) >= row_elems &&
              (n == 1 || p.stride(0) >= p.size(1) * p.stride(1)), what, ": rows with unit stride inside that do not overlap");
  return {p.stride(1) * es, (n > 1 ? p.stride(0) : p.size(1) * p.stride(1)) * es};
}

Tensor frames_from_yuv(const Tensor& y, const Tensor& c0, const optional<Tensor>& c1, int64_t format, at::IntArrayRef m, int64_t siting,
                       at::IntArrayRef slots, int64_t b, int64_t t, int64_t h, int64_t w, const optional<Tensor>& h_bounds,
                       const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds, const optional<Tensor>& v_coefs) {
  TORCH_CHECK(on_device(y, y) && on_device(c0, y) && (!c1.has_value() || on_device(*c1, y)),
              "frames_from_yuv: expected CUDA tensors (the product path is GPU-only)");
  TORCH_CHECK(format == TC_PIXFMT_I420 || format == TC_PIXFMT_NV12 || format == TC_PIXFMT_P010, "frames_from_yuv: format ", format);
  const bool planar = format == TC_PIXFMT_I420, wide = format == TC_PIXFMT_P010;
  auto sample_type = [&](const Tensor& p) {
    return wide ? p.scalar_type() == at::kShort || p.scalar_type() == at::kUInt16 : p.scalar_type() == at::kByte;
  };
  TORCH_CHECK(y.dim() == 3 && y.numel() > 0 && sample_type(y) && sample_type(c0), "frames_from_yuv: y (n, h, w) of ",
              wide ? "2-byte" : "uint8", " samples");
  const int64_t n = y.size(0), sh = y.size(1), sw = y.size(2), ch = (sh + 1) / 2, cw = (sw + 1) / 2;
  TORCH_CHECK(planar == c1.has_value(), "frames_from_yuv: a Cr plane for I420 only");
  if (planar) {
    TORCH_CHECK(c0.sizes() == at::IntArrayRef({n, ch, cw}) && c1->sizes() == c0.sizes() && c1->strides() == c0.strides() &&
                sample_type(*c1), "frames_from_yuv: I420 chroma planes (n, (h + 1) / 2, (w + 1) / 2) with one pitch");
  } else {
    TORCH_CHECK(c0.sizes() == at::IntArrayRef({n, ch, cw, 2}), "frames_from_yuv: an interleaved chroma plane (n, (h + 1) / 2, (w + 1) / 2, 2)");
  }
  TORCH_CHECK(m.size() == 7, "frames_from_yuv: the matrix has seven entries");
  TORCH_CHECK(siting == TC_CHROMA_NEAREST || siting == TC_CHROMA_CENTER || siting == TC_CHROMA_LEFT, "frames_from_yuv: siting ", siting);
  const Resize rs = front_request("frames_from_yuv", y, n, sh, sw, slots, b, t, h, w, h_bounds, h_coefs, v_bounds, v_coefs);
  const auto ry = plane_rows(y, sw, "frames_from_yuv: y"), rc = plane_rows(c0, planar ? cw : 2 * cw, "frames_from_yuv: chroma");
  Tensor out = at::zeros({b, 3, t, h, w}, y.options().dtype(at::kFloat));
  if (y.is_meta()) return out;
  TcFramesYuvParams p = {};
  int32_t slot[TC_FRAMES_U8_MAX];
  front_fill(p, slot, out, sh, sw, slots, rs);
  p.y = y.data_ptr(); p.c0 = c0.data_ptr(); p.c1 = planar ? c1->data_ptr() : nullptr;
  p.pitch_y = (int32_t)ry.first; p.image_stride_y = ry.second;
  p.pitch_c = (int32_t)rc.first; p.image_stride_c = rc.second;
  p.format = (int32_t)format; p.siting = (int32_t)siting;
  for (int i = 0; i < 7; ++i) p.m[i] = (int32_t)m[i];
  launch_ws(p, y, tc_frames_from_yuv_workspace, tc_frames_from_yuv, "tc_frames_from_yuv");
  return out;
}

// Pixel back end (additive within ABI 14): the one body of frames_to_u8 and frames_to_yuv.  Frames f0 .. f0 + nf - 1 of every clip
// of x (b, 3, t, h, w) fp32 -> a new packed uint8 tensor; the tables are tc_resize_tables_filter's for w -> ow and h -> oh, on the
// device (None for an axis that keeps its size).  Each operator checks its own format set and says what follows from the format:
// `sample`, the bytes of a sample of a planar 4:2:0 format, (b, nf, oh * ow * 3 / 2 * sample) with rows of sample * ow bytes, or 0
// for RGB24, (b, nf, oh, ow, 3); and `rest`, which sets the fields that only its params struct has.  Writing into a caller's
// buffer with strides is the C ABI's (HipOps.frames_to_u8 with out=): an op returns its result.
template <typename P, typename Rest>
Tensor frames_out(const char* what, int64_t (*bytes)(const P*), int (*entry)(const P*, void*), const Tensor& x, int64_t oh, int64_t ow,
                  int64_t format, int64_t f0, int64_t nf, int64_t sample, const optional<Tensor>& h_bounds,
                  const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds, const optional<Tensor>& v_coefs, Rest rest) {
  TORCH_CHECK(on_device(x, x), what, ": expected a CUDA tensor (the product path is GPU-only)");
  TORCH_CHECK(x.dim() == 5 && x.size(1) == 3 && x.numel() > 0, what, ": x must be (b, 3, t, h, w)");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous(), what, ": contiguous fp32 (b, 3, t, h, w)");
  TORCH_CHECK(oh > 0 && ow > 0 && oh <= INT32_MAX && ow <= INT32_MAX, what, ": output size (", oh, ", ", ow, ")");
  TORCH_CHECK(f0 >= 0 && nf >= 1 && f0 + nf <= x.size(2), what, ": frames ", f0, " .. ", f0 + nf - 1, " outside a clip of ", x.size(2));
  TORCH_CHECK(sample == 0 || (oh % 2 == 0 && ow % 2 == 0), what, ": planar frames need an even size, got (", oh, ", ", ow, ")");
  const Resize rs = resize_request(h_bounds, h_coefs, v_bounds, v_coefs, x, x.size(4), ow, x.size(3), oh, what);
  Tensor out = at::empty(sample ? std::vector<int64_t>{x.size(0), nf, oh * ow * 3 / 2 * sample} : std::vector<int64_t>{x.size(0), nf, oh, ow, 3},
                         x.options().dtype(at::kByte));
  if (x.is_meta()) return out;
  P p = {};
  p.x = x.data_ptr<float>(); p.out = static_cast<decltype(p.out)>(out.data_ptr());
  p.b = (int32_t)x.size(0); p.t = (int32_t)x.size(2); p.h = (int32_t)x.size(3); p.w = (int32_t)x.size(4);
  p.f0 = (int32_t)f0; p.nf = (int32_t)nf; p.oh = (int32_t)oh; p.ow = (int32_t)ow; p.format = (int32_t)format;
  p.pitch = (int32_t)(sample ? sample * ow : 3 * ow);
  p.frame_stride = out.stride(1); p.clip_stride = out.stride(0);
  resize_fill(p, rs);
  rest(p);
  launch_ws(p, x, bytes, entry, (std::string("tc_") + what).c_str());
  return out;
}

// frames_to_u8: RGB24, or I420 / NV12 in the fixed colour of tc_frames_to_u8
Tensor frames_to_u8(const Tensor& x, int64_t oh, int64_t ow, int64_t format, int64_t f0, int64_t nf, const optional<Tensor>& h_bounds,
                    const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds, const optional<Tensor>& v_coefs) {
  TORCH_CHECK(format == TC_PIXFMT_RGB24 || format == TC_PIXFMT_I420 || format == TC_PIXFMT_NV12, "frames_to_u8: format ", format);
  return frames_out("frames_to_u8", tc_frames_to_u8_workspace, tc_frames_to_u8, x, oh, ow, format, f0, nf, format == TC_PIXFMT_RGB24 ? 0 : 1,
                    h_bounds, h_coefs, v_bounds, v_coefs, [](TcFramesOutParams&) {});
}

// frames_to_yuv: planar frames in a caller's colour (tc_frames_to_yuv): format I420 / NV12 / P010 (2-byte samples), the siting code
// and the eleven integers of the RGB -> YCbCr matrix
Tensor frames_to_yuv(const Tensor& x, int64_t oh, int64_t ow, int64_t format, int64_t f0, int64_t nf, int64_t siting, at::IntArrayRef m,
                     const optional<Tensor>& h_bounds, const optional<Tensor>& h_coefs, const optional<Tensor>& v_bounds,
                     const optional<Tensor>& v_coefs) {
  TORCH_CHECK(format == TC_PIXFMT_I420 || format == TC_PIXFMT_NV12 || format == TC_PIXFMT_P010, "frames_to_yuv: format ", format);
  TORCH_CHECK(siting == TC_CHROMA_CENTER || siting == TC_CHROMA_LEFT, "frames_to_yuv: siting ", siting);
  TORCH_CHECK(m.size() == 11, "frames_to_yuv: the matrix has eleven entries");
  return frames_out("frames_to_yuv", tc_frames_to_yuv_workspace, tc_frames_to_yuv, x, oh, ow, format, f0, nf, format == TC_PIXFMT_P010 ? 2 : 1,
                    h_bounds, h_coefs, v_bounds, v_coefs, [&](TcFramesYuvOutParams& p) {
                      p.siting = (int32_t)siting;
                      for (int i = 0; i < 11; ++i) p.m[i] = (int32_t)m[i];
                    });
}

// Colour match and histogram transfer (additive within ABI 14): six ops, every check sentence once with the op's name in front.
// colour_stats / colour_hist: the nine float64 sums / the 3 x 1024 int32 counts of frames f0, f0 + fstep, ... (nf of them) of every
// clip of x (b, 3, t, h, w) fp32 -> (b, nf, 9) / (b, nf, 3, 1024).  colour_match / colour_transfer: x matched frame by frame to the
// course between the two reference images of its clip, linearly from the sums src (b, t, 9) and ref (b, 2, 9) -> (the matched clip,
// the (b, t, 12) fp32 coefficients), or channel by channel from the counts src (b, t, 3, 1024) and ref (b, 2, 3, 1024), blended by
// strength against clamp(x) or clamp(base) -> (the clip, the (b, t, 3, 1024) fp32 tables).  Their *_knots forms: towards the nk
// reference images of ref (b, nk, ...) at `knots` (strictly increasing frame indices, host integers that travel in the params
// struct), the match with the gain limit max_gain (0: none).  Each op is the C entry point tc_<its name>; matching in place is the
// C ABI's (HipOps.colour_match with out=): an op returns its result.
void colour_clip_check(const Tensor& x, const char* what) {
  TORCH_CHECK(x.dim() == 5 && x.size(1) == 3 && x.numel() > 0, what, ": x must be (b, 3, t, h, w)");
  for (int d : {0, 2, 3, 4}) TORCH_CHECK(x.size(d) <= INT32_MAX, what, ": dimension ", d, " of x");
}

void colour_hw_check(const Tensor& x, const char* what) {
  TORCH_CHECK(x.size(3) * x.size(4) <= (int64_t(1) << 26), what, ": h * w ", x.size(3) * x.size(4), " above 2^26");
}

// colour_stats / colour_hist: P the params struct, `result` its field for the op's tensor
template <typename P, typename R>
Tensor colour_frames(const Tensor& x, int64_t f0, int64_t nf, int64_t fstep, R* P::*result, int64_t (*bytes)(const P*),
                     int (*entry)(const P*, void*)) {
  constexpr bool hist = std::is_same_v<P, TcColourHistParams>;
  const char* what = hist ? "colour_hist" : "colour_stats";
  TORCH_CHECK(on_device(x, x), what, ": expected a CUDA tensor (the product path is GPU-only)");
  colour_clip_check(x, what);
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous(), what, ": contiguous fp32 (b, 3, t, h, w)");
  const int64_t t = x.size(2);
  TORCH_CHECK(nf >= 1 && f0 >= 0 && f0 < t && (nf == 1 || (fstep >= 1 && fstep <= INT32_MAX && f0 + (nf - 1) * fstep <= t - 1)),
              what, ": frames (", f0, ", ", nf, ", ", fstep, ") outside a clip of ", t);
  if (hist) colour_hw_check(x, what);
  Tensor res = at::empty(hist ? std::vector<int64_t>{x.size(0), nf, 3, TC_COLOUR_BINS} : std::vector<int64_t>{x.size(0), nf, TC_COLOUR_STATS},
                         x.options().dtype(c10::CppTypeToScalarType<R>::value));
  if (x.is_meta()) return res;
  P p = {};
  p.x = x.data_ptr<float>();
  p.b = (int32_t)x.size(0); p.t = (int32_t)x.size(2); p.h = (int32_t)x.size(3); p.w = (int32_t)x.size(4);
  p.f0 = (int32_t)f0; p.nf = (int32_t)nf; p.fstep = nf == 1 ? 1 : (int32_t)fstep;
  p.*result = res.data_ptr<R>();
  launch_ws(p, x, bytes, entry, hist ? "tc_colour_hist" : "tc_colour_stats");
  return res;
}

Tensor colour_stats(const Tensor& x, int64_t f0, int64_t nf, int64_t fstep) {
  return colour_frames(x, f0, nf, fstep, &TcColourStatsParams::stats, tc_colour_stats_workspace, tc_colour_stats);
}

Tensor colour_hist(const Tensor& x, int64_t f0, int64_t nf, int64_t fstep) {
  return colour_frames(x, f0, nf, fstep, &TcColourHistParams::hist, tc_colour_hist_workspace, tc_colour_hist);
}

// What the match and the transfer family share.  An op is the old one (knots null: two reference images per clip) or its knots form.
using Knots = const at::IntArrayRef*;
using Pair = std::tuple<Tensor, Tensor>;                     // (the result clip, its coefficients or tables)

int64_t colour_ref_rows(Knots knots) { return knots ? (int64_t)knots->size() : 2; }

void colour_knots_check(const char* what, const Tensor& x, Knots knots) {
  if (!knots) return;
  const int64_t t = x.size(2), nk = (int64_t)knots->size();
  TORCH_CHECK(nk >= 1 && nk <= TC_TEMPORAL_MAX_FRAMES, what, ": ", nk, " knots outside [1, ", TC_TEMPORAL_MAX_FRAMES, "]");
  for (int64_t i = 0; i < nk; ++i)
    TORCH_CHECK((*knots)[i] >= 0 && (*knots)[i] < t && (i == 0 || (*knots)[i] > (*knots)[i - 1]), what,
                ": knots must be strictly increasing frame indices in [0, ", t, ")");
}

void colour_strength_check(const char* what, double strength) {
  TORCH_CHECK(strength >= 0.0 && strength <= 1.0, what, ": strength ", strength, " outside [0, 1]");
}

void colour_device_check(const char* what, const Tensor& x, const Tensor& src, const Tensor& ref, const optional<Tensor>& base) {
  TORCH_CHECK(on_device(x, x) && on_device(src, x) && on_device(ref, x) && (!base.has_value() || on_device(*base, x)), what,
              ": expected CUDA tensors (the product path is GPU-only)");
}

// the fields that the four params structs of the two families share, and the knots of the two that have them
template <typename P>
void colour_clip_fill(P& p, const Tensor& x, const Tensor& out, const Tensor& src, const Tensor& ref, int64_t ref_pixels,
                      double strength, Knots knots) {
  p.x = x.data_ptr<float>(); p.out = out.data_ptr<float>();
  p.b = (int32_t)x.size(0); p.t = (int32_t)x.size(2); p.h = (int32_t)x.size(3); p.w = (int32_t)x.size(4);
  p.src = static_cast<decltype(p.src)>(src.data_ptr()); p.ref = static_cast<decltype(p.ref)>(ref.data_ptr());
  p.ref_pixels = ref_pixels; p.strength = (float)strength;
  if constexpr (std::is_same_v<P, TcColourMatchKnotsParams> || std::is_same_v<P, TcColourTransferKnotsParams>) {
    p.nk = (int32_t)knots->size();
    for (size_t i = 0; i < knots->size(); ++i) p.knot[i] = (int32_t)(*knots)[i];
  }
}

// The match family.
template <typename P>
Pair colour_match_any(const char* what, int (*entry)(const P*, void*), const Tensor& x, const Tensor& src, const Tensor& ref,
                      int64_t ref_pixels, int64_t method, double strength, Knots knots, double max_gain) {
  colour_device_check(what, x, src, ref, optional<Tensor>());
  colour_clip_check(x, what);
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous(), what, ": x: contiguous fp32 (b, 3, t, h, w)");
  TORCH_CHECK(src.scalar_type() == at::kDouble && src.is_contiguous() && ref.scalar_type() == at::kDouble && ref.is_contiguous(), what,
              ": src / ref: contiguous float64");
  const int64_t b = x.size(0), t = x.size(2);
  TORCH_CHECK(src.dim() == 3 && src.size(0) == b && src.size(1) == t && src.size(2) == TC_COLOUR_STATS, what, ": src must be (b, t, 9)");
  TORCH_CHECK(ref.dim() == 3 && ref.size(0) == b && ref.size(1) == colour_ref_rows(knots) && ref.size(2) == TC_COLOUR_STATS, what,
              ": ref must be (b, ", knots ? "nk" : "2", ", 9)");
  colour_knots_check(what, x, knots);
  TORCH_CHECK(method == TC_COLOUR_MEAN_STD || method == TC_COLOUR_MKL, what, ": method ", method);
  colour_strength_check(what, strength);
  TORCH_CHECK(ref_pixels > 0, what, ": ref_pixels ", ref_pixels);
  TORCH_CHECK(max_gain == 0.0 || (max_gain >= 1.0 && std::isfinite(max_gain)), what, ": max_gain ", max_gain,
              ": 0 (no limit) or a finite number >= 1");
  Tensor out = at::empty_like(x), coefs = at::empty({b, t, 12}, x.options());
  if (x.is_meta()) return {out, coefs};
  P p = {};
  colour_clip_fill(p, x, out, src, ref, ref_pixels, strength, knots);
  p.method = (int32_t)method;
  p.coefs = coefs.data_ptr<float>();
  if constexpr (std::is_same_v<P, TcColourMatchKnotsParams>) p.max_gain = (float)max_gain;
  check_rc(entry(&p, cur_stream()), (std::string("tc_") + what).c_str());
  return {out, coefs};
}

Pair colour_match(const Tensor& x, const Tensor& src, const Tensor& ref, int64_t ref_pixels, int64_t method, double strength) {
  return colour_match_any("colour_match", tc_colour_match, x, src, ref, ref_pixels, method, strength, nullptr, 0.0);
}

Pair colour_match_knots(const Tensor& x, const Tensor& src, const Tensor& ref, int64_t ref_pixels, int64_t method, double strength,
                        at::IntArrayRef knots, double max_gain) {
  return colour_match_any("colour_match_knots", tc_colour_match_knots, x, src, ref, ref_pixels, method, strength, &knots, max_gain);
}

// The transfer family.
template <typename P>
Pair colour_transfer_any(const char* what, int (*entry)(const P*, void*), const Tensor& x, const optional<Tensor>& base,
                         const Tensor& src, const Tensor& ref, int64_t ref_pixels, double strength, Knots knots) {
  colour_device_check(what, x, src, ref, base);
  colour_clip_check(x, what);
  const int64_t b = x.size(0), t = x.size(2);
  TORCH_CHECK(x.scalar_type() == at::kFloat, what, ": x: fp32 (b, 3, t, h, w)");
  TORCH_CHECK(!base.has_value() || (base->sizes() == x.sizes() && base->scalar_type() == at::kFloat), what,
              ": base must be fp32 of the shape of x");
  TORCH_CHECK(src.dim() == 4 && src.size(0) == b && src.size(1) == t && src.size(2) == 3 && src.size(3) == TC_COLOUR_BINS &&
                  src.scalar_type() == at::kInt, what, ": src must be int32 (b, t, 3, 1024)");
  TORCH_CHECK(ref.dim() == 4 && ref.size(0) == b && ref.size(1) == colour_ref_rows(knots) && ref.size(2) == 3 &&
                  ref.size(3) == TC_COLOUR_BINS && ref.scalar_type() == at::kInt, what, ": ref must be int32 (b, ", knots ? "nk" : "2",
              ", 3, 1024)");
  colour_knots_check(what, x, knots);
  colour_strength_check(what, strength);
  TORCH_CHECK(ref_pixels > 0 && ref_pixels <= (int64_t(1) << 26), what, ": ref_pixels ", ref_pixels, " outside [1, 2^26]");
  colour_hw_check(x, what);
  TORCH_CHECK(x.is_contiguous() && src.is_contiguous() && ref.is_contiguous() && (!base.has_value() || base->is_contiguous()), what,
              ": contiguous tensors");
  Tensor out = at::empty_like(x), table = at::empty({b, t, 3, TC_COLOUR_BINS}, x.options());
  if (x.is_meta()) return {out, table};
  P p = {};
  colour_clip_fill(p, x, out, src, ref, ref_pixels, strength, knots);
  p.base = f32_or_null(base);
  p.table = table.data_ptr<float>();
  check_rc(entry(&p, cur_stream()), (std::string("tc_") + what).c_str());
  return {out, table};
}

Pair colour_transfer(const Tensor& x, const optional<Tensor>& base, const Tensor& src, const Tensor& ref, int64_t ref_pixels,
                     double strength) {
  return colour_transfer_any("colour_transfer", tc_colour_transfer, x, base, src, ref, ref_pixels, strength, nullptr);
}

Pair colour_transfer_knots(const Tensor& x, const optional<Tensor>& base, const Tensor& src, const Tensor& ref, int64_t ref_pixels,
                           double strength, at::IntArrayRef knots) {
  return colour_transfer_any("colour_transfer_knots", tc_colour_transfer_knots, x, base, src, ref, ref_pixels, strength, &knots);
}

// clip_patches: (B, 3, H, W) fp32 -> the bf16 A operand [B * (size / patch)^2, ld] of the CLIP image tower's patch-embedding GEMM
// (reference condition.py:322-330: kornia resize, (x + 1) / 2, CLIP mean / std; then open_clip's conv1 unfold)
Tensor clip_patches(const Tensor& x, int64_t size, int64_t patch, int64_t ld, at::ArrayRef<double> mean, at::ArrayRef<double> std,
                    bool antialias) {
  TORCH_CHECK(on_device(x, x), "clip_patches: expected a CUDA tensor (the product path is GPU-only)");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 4 && x.size(1) == 3, "clip_patches: contiguous fp32 (B, 3, H, W)");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "clip_patches: mean and std have three entries");
  TORCH_CHECK(size > 0 && patch > 0 && size % patch == 0 && ld >= 3 * patch * patch, "clip_patches: size ", size, ", patch ", patch, ", ld ", ld);
  const int64_t g = size / patch;
  Tensor out = at::empty({x.size(0) * g * g, ld}, x.options().dtype(at::kBFloat16));
  if (x.is_meta()) return out;
  TcClipPatchesParams p = {};
  p.x = x.data_ptr<float>(); p.out = reinterpret_cast<tc_bf16*>(out.data_ptr());
  p.b = (int32_t)x.size(0); p.h = (int32_t)x.size(2); p.w = (int32_t)x.size(3);
  p.size = (int32_t)size; p.patch = (int32_t)patch; p.ld = (int32_t)ld; p.antialias = antialias ? 1 : 0;
  for (int i = 0; i < 3; ++i) { p.mean[i] = (float)mean[i]; p.std[i] = (float)std[i]; }
  launch_ws(p, x, tc_clip_patches_workspace, tc_clip_patches, "tc_clip_patches");
  return out;
}

// Per-clip Philox noise (tc_randn_clips, additive within ABI 14): (b, ...) fp32 on the current device, clip i from seeds[i] alone;
// raw: the Philox words as int32 bit patterns.  A seed from 2^63 on arrives as its two's-complement int64.  The op takes no
// tensor, so the dispatcher cannot read a backend off its arguments: the BackendSelect kernel below sends it to the CUDA key, and
// the one body takes its device from the key it was reached by (Meta: by naming that key in a redispatch).
Tensor randn_clips(c10::DispatchKeySet keys, at::IntArrayRef seeds, at::IntArrayRef shape, int64_t stream, double scale, bool raw) {
  TORCH_CHECK(!shape.empty() && (int64_t)seeds.size() == shape[0], "randn_clips: shape (b, ...) with one seed per clip");
  for (int64_t v : shape) TORCH_CHECK(v > 0, "randn_clips: sizes must be positive");
  TORCH_CHECK(shape[0] <= INT32_MAX, "randn_clips: b ", shape[0]);
  TORCH_CHECK(stream >= 0 && stream <= (int64_t)UINT32_MAX, "randn_clips: stream ", stream, " outside [0, 2^32)");
  const bool meta = keys.has_backend(c10::BackendComponent::MetaBit);
  Tensor out = at::empty(shape, at::TensorOptions().device(meta ? at::kMeta : at::kCUDA).dtype(raw ? at::kInt : at::kFloat));
  if (meta) return out;
  std::vector<uint64_t> held(seeds.begin(), seeds.end());
  TcRandnParams p = {};
  p.out = reinterpret_cast<float*>(out.data_ptr());
  p.seeds = held.data();
  p.b = (int32_t)shape[0]; p.n = out.numel() / shape[0];
  p.stream = (uint32_t)stream; p.scale = (float)scale; p.raw = raw ? 1 : 0;
  check_rc(tc_randn_clips(&p, cur_stream()), "tc_randn_clips");
  return out;
}

Tensor randn_clips_select(at::IntArrayRef seeds, at::IntArrayRef shape, int64_t stream, double scale, bool raw) {
  static auto op = c10::Dispatcher::singleton().findSchemaOrThrow("tooncrafter::randn_clips", "")
                       .typed<Tensor(at::IntArrayRef, at::IntArrayRef, int64_t, double, bool)>();
  return op.redispatch(c10::DispatchKeySet(c10::DispatchKey::CUDA), seeds, shape, stream, scale, raw);
}

// The operators, named once: the same function under the CUDA key and under the Meta key.
void register_ops(torch::Library& m) {
  m.impl("gemm", gemm);
  m.impl("quant_mxfp8", quant_mxfp8);
  m.impl("gemm_mx", gemm_mx);
  m.impl("attention", attention);
  m.impl("attention_temporal", attention_temporal);
  m.impl("attention_temporal_rel", attention_temporal_rel);
  m.impl("attention_q8", attention_q8);
  m.impl("groupnorm", groupnorm);
  m.impl("layernorm", layernorm);
  m.impl("groupnorm_pf", groupnorm_pf);
  m.impl("layernorm_pf", layernorm_pf);
  m.impl("ddim_step", ddim_step_any<false>);
  m.impl("ddim_step_eps", ddim_step_any<true>);
  m.impl("ddim_step_ms", ddim_step_ms_any<false>);
  m.impl("ddim_step_ms_eps", ddim_step_ms_any<true>);
  m.impl("ddim_blend", ddim_blend);
  m.impl("frames_from_u8", frames_from_u8);
  m.impl("frames_from_yuv", frames_from_yuv);
  m.impl("frames_to_u8", frames_to_u8);
  m.impl("frames_to_yuv", frames_to_yuv);
  m.impl("colour_stats", colour_stats);
  m.impl("colour_match", colour_match);
  m.impl("colour_hist", colour_hist);
  m.impl("colour_transfer", colour_transfer);
  m.impl("colour_match_knots", colour_match_knots);
  m.impl("colour_transfer_knots", colour_transfer_knots);
  m.impl("clip_patches", clip_patches);
  m.impl("randn_clips", randn_clips);
  m.impl("ff_geglu_fused", ff_geglu_fused);
  m.impl("temporal_attn_fused", temporal_attn_fused);
  m.impl("temporal_qkv_attn", temporal_qkv_attn);
}

}  // namespace

TORCH_LIBRARY(tooncrafter, m) {
  m.def("gemm(Tensor a, Tensor w, Tensor? bias, Tensor? residual, Tensor? row_bias, int row_div, int act, float alpha, "
        "float out_scale, bool out_f32, int[] conv, float a_norm_eps=-1.0) -> Tensor");
  m.def("quant_mxfp8(Tensor x, int k) -> (Tensor, Tensor)");
  m.def("gemm_mx(Tensor aq, Tensor a_scale, Tensor wq, Tensor w_scale, Tensor? bias, Tensor? residual, Tensor? row_bias, "
        "int row_div, int act, float alpha, float out_scale, bool out_f32, int[] conv) -> Tensor");
  m.def("attention(Tensor q, Tensor k, Tensor v, int batch, int heads, int lq, int lk, int kv_bdiv, float scale, "
        "Tensor? k2, Tensor? v2, int lk2, int kv2_bdiv) -> Tensor");
  m.def("attention_temporal(Tensor qkv, int b, int t, int hw, int heads, float scale) -> Tensor");
  m.def("attention_temporal_rel(Tensor qkv, Tensor? rel_k, Tensor? rel_v, int b, int t, int hw, int heads, int max_rel, "
        "bool causal, float scale) -> Tensor");
  m.def("attention_q8(Tensor q, Tensor k, Tensor v, int batch, int heads, int lq, int lk, float scale) -> Tensor");
  m.def("groupnorm(Tensor x, Tensor gamma, Tensor beta, int samples, int rows, float eps, bool silu) -> Tensor");
  m.def("ff_geglu_fused(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, float ln_eps) -> Tensor");
  m.def("temporal_attn_fused(Tensor x, Tensor wqkv, Tensor bqkv, Tensor wo, Tensor bo, int b, int t, int hw, int heads, float ln_eps, float scale) -> Tensor");
  m.def("temporal_qkv_attn(Tensor x, Tensor wqkv, Tensor? bqkv, int b, int t, int hw, int heads, float scale) -> Tensor");
  m.def("layernorm(Tensor x, Tensor gamma, Tensor beta, float eps) -> Tensor");
  m.def("groupnorm_pf(Tensor x, Tensor gamma, Tensor beta, int samples, int rows, float eps, bool silu, Tensor[] prefetch) -> Tensor");
  m.def("layernorm_pf(Tensor x, Tensor gamma, Tensor beta, float eps, Tensor[] prefetch) -> Tensor");
  m.def("ddim_step(Tensor x, Tensor e_cond, Tensor? e_uncond, Tensor? noise, Tensor? e_uncond_img, float cfg_scale, "
        "float cfg_img, float guidance_rescale, float sqrt_ac, float sqrt_1m_ac, float sqrt_a_prev, float dir_coef, "
        "float sigma, float x0_rescale) -> (Tensor, Tensor)");
  m.def("ddim_step_eps(Tensor x, Tensor e_cond, Tensor? e_uncond, Tensor? noise, Tensor? e_uncond_img, float cfg_scale, "
        "float cfg_img, float guidance_rescale, float sqrt_ac, float sqrt_1m_ac, float sqrt_a_prev, float dir_coef, "
        "float sigma, float x0_rescale) -> (Tensor, Tensor)");
  m.def("ddim_step_ms(Tensor x, Tensor e_cond, Tensor? e_uncond, Tensor? noise, Tensor? e_uncond_img, Tensor? x0_hist, float corr, "
        "float cfg_scale, float cfg_img, float guidance_rescale, float sqrt_ac, float sqrt_1m_ac, float sqrt_a_prev, "
        "float dir_coef, float sigma, float x0_rescale) -> (Tensor, Tensor)");
  m.def("ddim_step_ms_eps(Tensor x, Tensor e_cond, Tensor? e_uncond, Tensor? noise, Tensor? e_uncond_img, Tensor? x0_hist, float corr, "
        "float cfg_scale, float cfg_img, float guidance_rescale, float sqrt_ac, float sqrt_1m_ac, float sqrt_a_prev, "
        "float dir_coef, float sigma, float x0_rescale) -> (Tensor, Tensor)");
  m.def("ddim_blend(Tensor? x, Tensor x0, Tensor? noise, Tensor? mask, float sqrt_ac, float sqrt_1m_ac) -> Tensor");
  m.def("frames_from_u8(Tensor images, int[] slots, int b, int t, int h, int w, Tensor? h_bounds, Tensor? h_coefs, "
        "Tensor? v_bounds, Tensor? v_coefs) -> Tensor");
  m.def("frames_from_yuv(Tensor y, Tensor c0, Tensor? c1, int format, int[] m, int siting, int[] slots, int b, int t, int h, int w, "
        "Tensor? h_bounds, Tensor? h_coefs, Tensor? v_bounds, Tensor? v_coefs) -> Tensor");
  m.def("frames_to_u8(Tensor x, int oh, int ow, int format, int f0, int nf, Tensor? h_bounds, Tensor? h_coefs, Tensor? v_bounds, "
        "Tensor? v_coefs) -> Tensor");
  m.def("frames_to_yuv(Tensor x, int oh, int ow, int format, int f0, int nf, int siting, int[] m, Tensor? h_bounds, Tensor? h_coefs, "
        "Tensor? v_bounds, Tensor? v_coefs) -> Tensor");
  m.def("colour_stats(Tensor x, int f0, int nf, int fstep) -> Tensor");
  m.def("colour_match(Tensor x, Tensor src, Tensor ref, int ref_pixels, int method, float strength) -> (Tensor, Tensor)");
  m.def("colour_hist(Tensor x, int f0, int nf, int fstep) -> Tensor");
  m.def("colour_transfer(Tensor x, Tensor? base, Tensor src, Tensor ref, int ref_pixels, float strength) -> (Tensor, Tensor)");
  m.def("colour_match_knots(Tensor x, Tensor src, Tensor ref, int ref_pixels, int method, float strength, int[] knots, float max_gain) -> (Tensor, Tensor)");
  m.def("colour_transfer_knots(Tensor x, Tensor? base, Tensor src, Tensor ref, int ref_pixels, float strength, int[] knots) -> (Tensor, Tensor)");
  m.def("clip_patches(Tensor x, int size, int patch, int ld, float[] mean, float[] std, bool antialias) -> Tensor");
  m.def("randn_clips(int[] seeds, int[] shape, int stream, float scale, bool raw) -> Tensor");
  m.def("abi_version() -> int");
}

TORCH_LIBRARY_IMPL(tooncrafter, CUDA, m) { register_ops(m); }

TORCH_LIBRARY_IMPL(tooncrafter, Meta, m) { register_ops(m); }

TORCH_LIBRARY_IMPL(tooncrafter, BackendSelect, m) {
  m.impl("randn_clips", randn_clips_select);
}

TORCH_LIBRARY_IMPL(tooncrafter, CompositeExplicitAutograd, m) {
  m.impl("abi_version", []() -> int64_t { return tc_abi_version(); });
}
