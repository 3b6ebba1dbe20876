// Python bindings of the gfx950 kernels (module jax_llama_amd._C).
//
// Thin: validate dtypes/shapes/contiguity on the host (a wrong shape must never reach a kernel),
// take raw pointers and launch on torch's current HIP stream (so hipGraph capture through
// torch.cuda.graph records these launches). Kernel code lives in csrc/kernels/*.hip.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/launchers.h"

namespace {

using torch::Tensor;

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check(bool cond, const char* msg) { TORCH_CHECK(cond, "jax_llama_amd._C: ", msg); }

void check_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "jax_llama_amd._C: ", name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), "jax_llama_amd._C: ", name, " must be contiguous");
}

void rc(int r, const char* what) {
  TORCH_CHECK(r == 0, "jax_llama_amd._C: ", what, " failed (code ", r, ")");
}

// jla::gemm's return codes (kernels/gemm_plan.h: the one place that decides them) in words
void gemm_rc(int r, const char* what) {
  const char* why = r == -1   ? "no legal plan for this shape / tile id / epilogue / fused norm / K split"
                    : r == -3 ? "the slab workspace is missing or too small"
                    : r == -5 ? "fused RMS is not available in residual mode"
                    : r == -6 ? "this tile takes the fused norm only from rms_ws and without a K split"
                    : r == -7 ? "tiles 18 / 19: no tail split beats the uniform grid for this shape (gemm_tail_split)"
                              : "HIP error";
  TORCH_CHECK(r == 0, "jax_llama_amd._C: ", what, " failed (code ", r, ": ", why, "; see gemm_plan.h)");
}
bool is_g5(int64_t tile) { return tile == jla::G5_TILE || tile == jla::G5N_TILE; }  // slabs for any split

template <typename T>
T* ptr(const Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

const jla::bf16_t* cbf(const Tensor& t) { return reinterpret_cast<const jla::bf16_t*>(t.data_ptr()); }
jla::bf16_t* bf(const Tensor& t) { return reinterpret_cast<jla::bf16_t*>(t.data_ptr()); }

// optional bf16 mirror of an fp32 residual-stream tensor (same element count)
jla::bf16_t* mirror_ptr(const c10::optional<Tensor>& mirror, int64_t numel) {
  if (!mirror.has_value()) return nullptr;
  check_gpu(*mirror, "mirror");
  check(mirror->scalar_type() == torch::kBFloat16 && mirror->numel() == numel, "mirror must be bf16, same shape");
  return bf(*mirror);
}

void embedding(Tensor ids, Tensor table, Tensor out, c10::optional<Tensor> mirror) {
  check_gpu(ids, "ids");
  check_gpu(table, "table");
  check_gpu(out, "out");
  check(ids.scalar_type() == torch::kInt32 && table.scalar_type() == torch::kBFloat16 &&
            out.scalar_type() == torch::kFloat32,
        "embedding dtypes");
  const int M = ids.numel(), D = table.size(1), V = table.size(0);
  check(out.numel() == (int64_t)M * D, "embedding out shape");
  rc(jla::embedding(ptr<int32_t>(ids), cbf(table), ptr<float>(out), mirror_ptr(mirror, out.numel()), M, D, V,
                    stream()),
     "embedding");
}

void rms_scale(Tensor x, Tensor out, double eps) {
  check_gpu(x, "x");
  check_gpu(out, "out");
  check((x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kBFloat16) &&
            out.scalar_type() == torch::kBFloat16,
        "rms_scale dtypes");
  const int D = x.size(-1), M = x.numel() / D;
  check(out.numel() == x.numel(), "rms_scale out shape");
  if (x.scalar_type() == torch::kBFloat16)
    rc(jla::rms_scale_bf16(cbf(x), bf(out), M, D, (float)eps, stream()), "rms_scale_bf16");
  else
    rc(jla::rms_scale(ptr<float>(x), bf(out), M, D, (float)eps, stream()), "rms_scale");
}

void rmsnorm(Tensor x, Tensor w, Tensor out, double eps) {
  check_gpu(x, "x");
  check_gpu(w, "w");
  check_gpu(out, "out");
  check(x.scalar_type() == torch::kFloat32 && w.scalar_type() == torch::kFloat32 &&
            out.scalar_type() == torch::kFloat32,
        "rmsnorm dtypes");
  const int D = x.size(-1), M = x.numel() / D;
  check(w.numel() == D && out.numel() == x.numel(), "rmsnorm shapes");
  rc(jla::rmsnorm(ptr<float>(x), ptr<float>(w), ptr<float>(out), M, D, (float)eps, stream()), "rmsnorm");
}

// h (fp32) += p (bf16 / fp32, same element count); hb = bf16(h)
void residual_add(Tensor h, Tensor p, Tensor hb) {
  check_gpu(h, "h");
  check_gpu(p, "p");
  check_gpu(hb, "hb");
  check(h.scalar_type() == torch::kFloat32 && hb.scalar_type() == torch::kBFloat16 &&
            (p.scalar_type() == torch::kBFloat16 || p.scalar_type() == torch::kFloat32),
        "residual_add dtypes");
  check(p.numel() == h.numel() && hb.numel() == h.numel() && h.numel() % 8 == 0, "residual_add shapes");
  rc(jla::residual_add(ptr<float>(h), p.data_ptr(), p.scalar_type() == torch::kBFloat16, bf(hb), h.numel(), stream()),
     "residual_add");
}

// load every byte of t with the default cache policy (Infinity Cache warm-up of the next projection's weights)
void prefetch(Tensor t, int64_t grid) {
  check(t.is_cuda() && t.is_contiguous(), "prefetch: contiguous GPU tensor");
  static unsigned* sink = nullptr;  // allocated at the first (eager) call: never inside a graph capture
  if (!sink) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream(), &st);
    check(st == hipStreamCaptureStatusNone, "prefetch: first call under graph capture");
    rc((int)hipMalloc(reinterpret_cast<void**>(&sink), 64), "prefetch sink");
  }
  const int64_t nbytes = t.numel() * t.element_size() / 16 * 16;
  if (grid < 0) {  // the sequential streaming-read probe (calibration): each wave one contiguous range, -grid blocks
    rc(jla::stream_probe(t.data_ptr(), nbytes, (int)-grid, sink, stream()), "stream_probe");
    return;
  }
  rc(jla::prefetch(t.data_ptr(), nbytes, (int)grid, sink, stream()), "prefetch");
}

// y [M, N] = x [M, K] @ w [N, K]^T, all fp32 (precision='highest' lm_head)
void gemm_f32(Tensor x, Tensor w, Tensor y) {
  check_gpu(x, "x");
  check_gpu(w, "w");
  check_gpu(y, "y");
  check(x.scalar_type() == torch::kFloat32 && w.scalar_type() == torch::kFloat32 && y.scalar_type() == torch::kFloat32,
        "gemm_f32 dtypes");
  check(x.dim() == 2 && w.dim() == 2 && y.dim() == 2 && x.size(1) == w.size(1) && y.size(0) == x.size(0) &&
            y.size(1) == w.size(0),
        "gemm_f32 shapes");
  rc(jla::gemm_f32(ptr<float>(x), ptr<float>(w), ptr<float>(y), x.size(0), w.size(0), x.size(1), stream()), "gemm_f32");
}

void check_packed(const Tensor& w, int64_t n, int64_t k) {
  check_gpu(w, "weight");
  check(w.scalar_type() == torch::kBFloat16, "weight must be bf16");
  check(w.dim() == 4 && w.size(0) == n / 16 && w.size(1) == k / 32 && w.size(2) == 64 && w.size(3) == 8,
        "weight must be fragment-packed [N/16, K/32, 64, 8]");
}

void check_linear_out(const Tensor& out, int64_t m, int64_t n, int64_t mode) {
  check_gpu(out, "out");
  const int64_t ncols = (mode == 2) ? n / 2 : n;
  check(out.numel() == m * ncols, "linear out shape");
  if (mode == 1) check(out.scalar_type() == torch::kFloat32, "residual must be fp32");
  if (mode == 2) check(out.scalar_type() == torch::kBFloat16, "swiglu out must be bf16");
  if (mode == 0)
    check(out.scalar_type() == torch::kBFloat16 || out.scalar_type() == torch::kFloat32, "out must be bf16/fp32");
}

// packed-layout activation copy (common.h pack_off): bf16, >= the GEMV's m-tiles (1, 2 or 4) * 16 rows of `cols`
int64_t packed_rows(int64_t m) { return 16 * jla::gemv_m_tiles((int)m); }
jla::bf16_t* packed_ptr(const c10::optional<Tensor>& t, int64_t m, int64_t cols, const char* what) {
  if (!t.has_value()) return nullptr;
  check_gpu(*t, what);
  check(t->scalar_type() == torch::kBFloat16 && t->numel() >= packed_rows(m) * cols && cols % 32 == 0,
        "packed activation: bf16 [padded rows, cols], cols % 32 == 0");
  return bf(*t);
}

// The plan of a decode-GEMV call, or the rule that refuses it (kernels/gemv_plan.h: the variant table and every rule)
jla::GemvPlan skinny_plan(int64_t m, int64_t n, int64_t k, int64_t mode, bool f32, bool x_packed, int64_t variant) {
  const jla::GemvPlanResult r = jla::gemv_plan((int)m, (int)n, (int)k, (int)mode, f32, x_packed, (int)variant);
  TORCH_CHECK(r.rc == 0, "jax_llama_amd._C: decode GEMV variant ", variant, ": ", r.why, " (see gemv_plan.h)");
  return r.plan;
}

// Decode linear dispatch (gemv.hip linear_skinny); the variant ids: kernels/gemv_plan.h
void run_skinny(const Tensor& x, const Tensor& w, int64_t n, int64_t k, void* out, int64_t mode, double rms_eps,
                bool accumulate, bool out_f32, const jla::QKVArgs* qa, int64_t variant, const Tensor& ws,
                const Tensor& tickets, const jla::bf16_t* x_packed = nullptr) {
  const int64_t m = x.size(0);
  const bool f32 = x.scalar_type() == torch::kFloat32;
  const jla::GemvPlan p = skinny_plan(m, n, k, mode, f32, x_packed != nullptr, variant);
  jla::QKVArgs qs = *qa;
  if (p.split) {
    // split-K GEMV: partial slabs + self-resetting tickets (the shared skinny workspace, sized for both)
    check_gpu(ws, "ws");
    check_gpu(tickets, "tickets");
    check(ws.scalar_type() == torch::kFloat32 && tickets.scalar_type() == torch::kInt32, "ws/tickets dtypes");
    check((size_t)ws.numel() >= jla::gemv_split_workspace_floats(m, n) && ws.numel() < (1LL << 29) &&
              tickets.numel() >= jla::gemv_split_tickets(n),
          "split-K GEMV: workspace / tickets too small");
    qs.sk_ws = ptr<float>(ws);
    qs.sk_tk = ptr<int32_t>(tickets);
    qs.sk_ws_floats = (int)ws.numel();
  }
  rc(jla::linear_skinny(x_packed ? (const void*)x_packed : x.data_ptr(), f32, w.data_ptr(), out, m, n, k, mode,
                        (float)rms_eps, accumulate, out_f32, &qs, variant, stream()),
     "linear_skinny");
}

void linear_skinny(Tensor x, Tensor w, int64_t n, int64_t k, Tensor out, int64_t mode, double rms_eps,
                   bool accumulate, int64_t variant, Tensor ws, Tensor tickets, c10::optional<Tensor> mirror,
                   c10::optional<Tensor> x_packed, c10::optional<Tensor> pack_out) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  check(x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kBFloat16, "x must be fp32/bf16");
  check(mode >= 0 && mode <= 2, "linear_skinny mode");
  const int64_t m = x.size(0);
  check(m <= SKINNY_MAX_M, "linear_skinny: M too large");
  check_linear_out(out, m, n, mode);
  jla::QKVArgs qa{};
  qa.res_bf16 = mode == 1 ? mirror_ptr(mirror, out.numel()) : nullptr;
  // packed copy of the bf16 output (the residual's mirror / the SwiGLU activation): GEMV variants only
  qa.pack = packed_ptr(pack_out, m, mode == 2 ? n / 2 : n, "pack_out");
  check(!qa.pack || (mode == 1 || mode == 2), "pack_out: residual (mirror) or SwiGLU output only");
  check(!qa.pack || variant != 0, "pack_out: name a GEMV variant");
  check(!qa.pack || mode != 1 || qa.res_bf16, "pack_out of a residual needs the mirror");
  run_skinny(x, w, n, k, out.data_ptr(), mode, rms_eps, accumulate, out.scalar_type() == torch::kFloat32, &qa,
             variant, ws, tickets, packed_ptr(x_packed, m, k, "x_packed"));
}

// greedy lm_head at decode M (<= 64): GEMV with a first-max epilogue -> [M][N / 16] (value, index) partials in
// `part`, then one wave per row picks the first maximum (the fp32 logits are never written)
void linear_skinny_argmax(Tensor x, Tensor w, int64_t n, int64_t k, double rms_eps, int64_t variant, Tensor part,
                          Tensor idx, Tensor val) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && (x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kBFloat16),
        "x must be fp32/bf16 [M, K]");
  const int64_t m = x.size(0);
  check(m <= SKINNY_MAX_M, "linear_skinny_argmax: M too large");
  skinny_plan(m, n, k, MODE_ARGMAX, x.scalar_type() == torch::kFloat32, false, variant);
  check_gpu(part, "part");
  check(part.scalar_type() == torch::kFloat32 && part.numel() >= m * (n / 16) * 2, "argmax partials too small");
  check_gpu(idx, "idx");
  check_gpu(val, "val");
  check(idx.scalar_type() == torch::kInt32 && val.scalar_type() == torch::kFloat32 && idx.numel() == m &&
            val.numel() == m,
        "argmax outputs");
  jla::QKVArgs qa{};
  rc(jla::linear_skinny(x.data_ptr(), x.scalar_type() == torch::kFloat32, w.data_ptr(), part.data_ptr(), m, n, k,
                        MODE_ARGMAX, (float)rms_eps, 0, 1, &qa, variant, stream()),
     "linear_skinny_argmax");
  rc(jla::argmax_partials(ptr<float>(part), n / 16, m, ptr<int32_t>(idx), ptr<float>(val), stream()), "argmax_partials");
}

// the decode workspace of the split-K GEMV variants: partial slabs + tickets
py::tuple skinny_workspace(int64_t m, int64_t n) {
  return py::make_tuple((int64_t)jla::gemv_split_workspace_floats(m, n), (int64_t)jla::gemv_split_tickets(n));
}

// RoPE + KV-cache epilogue arguments of the fused qkv projection (validated here)
jla::QKVArgs qkv_args(int64_t m, int64_t n, const Tensor& table, const Tensor& positions, const Tensor& kc,
                      const Tensor& vc, const Tensor& slot, int64_t seq_len, int64_t h, int64_t hkv, int64_t dh,
                      const Tensor& q) {
  for (auto* t : {&table, &positions, &kc, &vc, &slot, &q}) check_gpu(*t, "linear_qkv arg");
  check(n == (h + 2 * hkv) * dh && dh % 16 == 0, "qkv width");
  check(table.scalar_type() == torch::kFloat32 && table.dim() == 3 && table.size(1) == dh / 2 && table.size(2) == 2,
        "rope table must be fp32 [L, Dh/2, 2]");
  check(positions.scalar_type() == torch::kInt32 && positions.numel() == m && slot.scalar_type() == torch::kInt32,
        "positions/slot");
  check(m % seq_len == 0, "M must be B * seq_len");
  const int64_t b = m / seq_len;
  check(kc.scalar_type() == torch::kBFloat16 && kc.dim() == 4 && kc.size(0) == b && kc.size(1) == hkv &&
            kc.size(3) == dh && vc.sizes() == kc.sizes() && vc.scalar_type() == torch::kBFloat16,
        "cache shape [B, Hkv, T, Dh]");
  check(q.scalar_type() == torch::kBFloat16 && q.numel() == m * h * dh, "q out");
  jla::QKVArgs qa;
  qa.table = reinterpret_cast<const float2*>(table.data_ptr());
  qa.table_len = table.size(0);
  qa.positions = ptr<int32_t>(positions);
  qa.kc = bf(kc);
  qa.vc = bf(vc);
  qa.slot = ptr<int32_t>(slot);
  qa.S = seq_len;
  qa.H = h;
  qa.Hkv = hkv;
  qa.Dh = dh;
  qa.T = kc.size(2);
  qa.q = bf(q);
  qa.res_bf16 = nullptr;
  qa.pack = nullptr;
  return qa;
}

// fused qkv projection + RoPE + KV-cache write (decode / small M)
void linear_qkv(Tensor x, Tensor w, int64_t n, int64_t k, double rms_eps, Tensor table, Tensor positions, Tensor kc,
                Tensor vc, Tensor slot, int64_t seq_len, int64_t h, int64_t hkv, int64_t dh, Tensor q,
                int64_t variant, Tensor ws, Tensor tickets, c10::optional<Tensor> x_packed) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  check(x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kBFloat16, "x must be fp32/bf16");
  const int64_t m = x.size(0);
  check(m <= SKINNY_MAX_M, "linear_qkv: M too large");
  jla::QKVArgs qa = qkv_args(m, n, table, positions, kc, vc, slot, seq_len, h, hkv, dh, q);
  run_skinny(x, w, n, k, nullptr, MODE_QKV, rms_eps, false, false, &qa, variant, ws, tickets,
             packed_ptr(x_packed, m, k, "x_packed"));
}

// ---- FP8 (e4m3) weight-only linears (gemv.hip): w8 uint8 [N/16, K/64, 64, 16], scale fp32 [N]
void check_packed_w8(const Tensor& w8, const Tensor& scale, int64_t n, int64_t k) {
  check_gpu(w8, "fp8 weight");
  check_gpu(scale, "fp8 scale");
  check(n > 0 && k > 0 && n % 16 == 0 && k % 64 == 0, "fp8 weight: N % 16 == 0, K % 64 == 0");
  check(w8.scalar_type() == torch::kUInt8 && w8.dim() == 4 && w8.size(0) == n / 16 && w8.size(1) == k / 64 &&
            w8.size(2) == 64 && w8.size(3) == 16,
        "fp8 weight must be uint8 [N/16, K/64, 64, 16]");
  check(scale.scalar_type() == torch::kFloat32 && scale.numel() == n, "fp8 scale must be fp32 [N]");
}

// out = W_deq in the bf16 fragment-packed layout
void dequant_fp8(Tensor w8, Tensor scale, int64_t n, int64_t k, Tensor out) {
  check_packed_w8(w8, scale, n, k);
  check_packed(out, n, k);
  rc(jla::dequant_fp8(w8.data_ptr(), ptr<float>(scale), out.data_ptr(), n, k, stream()), "dequant_fp8");
}

// The plan of an FP8-weight decode-GEMV call, or the rule that refuses it (kernels/gemv_plan.h gemv_w8_plan)
void skinny_w8_plan(int64_t m, int64_t n, int64_t k, int64_t mode, bool f32) {
  const jla::GemvPlanResult r = jla::gemv_w8_plan((int)m, (int)n, (int)k, (int)mode, f32);
  TORCH_CHECK(r.rc == 0, "jax_llama_amd._C: FP8-weight decode GEMV: ", r.why, " (see gemv_plan.h)");
}

void linear_skinny_w8(Tensor x, Tensor w8, Tensor scale, int64_t n, int64_t k, Tensor out, int64_t mode,
                      double rms_eps, bool accumulate, c10::optional<Tensor> mirror, c10::optional<Tensor> pack_out) {
  check_gpu(x, "x");
  check_packed_w8(w8, scale, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  check(mode >= 0 && mode <= 2, "linear_skinny_w8 mode");
  const int64_t m = x.size(0);
  skinny_w8_plan(m, n, k, mode, x.scalar_type() != torch::kBFloat16);
  check_linear_out(out, m, n, mode);
  jla::QKVArgs qa{};
  qa.res_bf16 = mode == 1 ? mirror_ptr(mirror, out.numel()) : nullptr;
  qa.pack = packed_ptr(pack_out, m, mode == 2 ? n / 2 : n, "pack_out");
  check(!qa.pack || (mode == 1 || mode == 2), "pack_out: residual (mirror) or SwiGLU output only");
  check(!qa.pack || mode != 1 || qa.res_bf16, "pack_out of a residual needs the mirror");
  rc(jla::linear_skinny_w8(x.data_ptr(), 0, w8.data_ptr(), ptr<float>(scale), out.data_ptr(), m, n, k, mode,
                           (float)rms_eps, accumulate, out.scalar_type() == torch::kFloat32, &qa, stream()),
     "linear_skinny_w8");
}

void linear_qkv_w8(Tensor x, Tensor w8, Tensor scale, int64_t n, int64_t k, double rms_eps, Tensor table,
                   Tensor positions, Tensor kc, Tensor vc, Tensor slot, int64_t seq_len, int64_t h, int64_t hkv,
                   int64_t dh, Tensor q) {
  check_gpu(x, "x");
  check_packed_w8(w8, scale, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  const int64_t m = x.size(0);
  skinny_w8_plan(m, n, k, MODE_QKV, x.scalar_type() != torch::kBFloat16);
  jla::QKVArgs qa = qkv_args(m, n, table, positions, kc, vc, slot, seq_len, h, hkv, dh, q);
  rc(jla::linear_skinny_w8(x.data_ptr(), 0, w8.data_ptr(), ptr<float>(scale), nullptr, m, n, k, MODE_QKV,
                           (float)rms_eps, 0, 0, &qa, stream()),
     "linear_qkv_w8");
}

// ---- MXFP4 weight-only linears (gemv.hip): w4 uint8 [N/16, K/128, 64, 16] (two e2m1 codes per byte), s4 uint8
// [N/16, K/128, 16, 4] (e8m0 bytes)
void check_packed_w4(const Tensor& w4, const Tensor& s4, int64_t n, int64_t k) {
  check_gpu(w4, "mxfp4 weight");
  check_gpu(s4, "mxfp4 scale");
  check(n > 0 && k > 0 && n % 16 == 0 && k % 128 == 0, "mxfp4 weight: N % 16 == 0, K % 128 == 0");
  check(w4.scalar_type() == torch::kUInt8 && w4.dim() == 4 && w4.size(0) == n / 16 && w4.size(1) == k / 128 &&
            w4.size(2) == 64 && w4.size(3) == 16,
        "mxfp4 weight must be uint8 [N/16, K/128, 64, 16]");
  check(s4.scalar_type() == torch::kUInt8 && s4.dim() == 4 && s4.size(0) == n / 16 && s4.size(1) == k / 128 &&
            s4.size(2) == 16 && s4.size(3) == 4,
        "mxfp4 scale must be uint8 [N/16, K/128, 16, 4]");
  check(w4.device() == s4.device(), "mxfp4 weight and scale on one device");
}

// out = W_deq in the bf16 fragment-packed layout
void dequant_fp4(Tensor w4, Tensor s4, int64_t n, int64_t k, Tensor out) {
  check_packed_w4(w4, s4, n, k);
  check_packed(out, n, k);
  rc(jla::dequant_fp4(w4.data_ptr(), s4.data_ptr(), out.data_ptr(), n, k, stream()), "dequant_fp4");
}

// The plan of an MXFP4-weight decode-GEMV call, or the rule that refuses it (kernels/gemv_plan.h gemv_w4_plan)
void skinny_w4_plan(int64_t m, int64_t n, int64_t k, int64_t mode, bool f32) {
  const jla::GemvPlanResult r = jla::gemv_w4_plan((int)m, (int)n, (int)k, (int)mode, f32);
  TORCH_CHECK(r.rc == 0, "jax_llama_amd._C: MXFP4-weight decode GEMV: ", r.why, " (see gemv_plan.h)");
}

void linear_skinny_w4(Tensor x, Tensor w4, Tensor s4, int64_t n, int64_t k, Tensor out, int64_t mode, double rms_eps,
                      bool accumulate, c10::optional<Tensor> mirror, c10::optional<Tensor> pack_out) {
  check_gpu(x, "x");
  check_packed_w4(w4, s4, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  check(mode >= 0 && mode <= 2, "linear_skinny_w4 mode");
  const int64_t m = x.size(0);
  skinny_w4_plan(m, n, k, mode, x.scalar_type() != torch::kBFloat16);
  check_linear_out(out, m, n, mode);
  jla::QKVArgs qa{};
  qa.res_bf16 = mode == 1 ? mirror_ptr(mirror, out.numel()) : nullptr;
  qa.pack = packed_ptr(pack_out, m, mode == 2 ? n / 2 : n, "pack_out");
  check(!qa.pack || (mode == 1 || mode == 2), "pack_out: residual (mirror) or SwiGLU output only");
  check(!qa.pack || mode != 1 || qa.res_bf16, "pack_out of a residual needs the mirror");
  rc(jla::linear_skinny_w4(x.data_ptr(), 0, w4.data_ptr(), s4.data_ptr(), out.data_ptr(), m, n, k, mode,
                           (float)rms_eps, accumulate, out.scalar_type() == torch::kFloat32, &qa, stream()),
     "linear_skinny_w4");
}

void linear_qkv_w4(Tensor x, Tensor w4, Tensor s4, int64_t n, int64_t k, double rms_eps, Tensor table,
                   Tensor positions, Tensor kc, Tensor vc, Tensor slot, int64_t seq_len, int64_t h, int64_t hkv,
                   int64_t dh, Tensor q) {
  check_gpu(x, "x");
  check_packed_w4(w4, s4, n, k);
  check(x.dim() == 2 && x.size(1) == k, "x must be [M, K]");
  const int64_t m = x.size(0);
  skinny_w4_plan(m, n, k, MODE_QKV, x.scalar_type() != torch::kBFloat16);
  jla::QKVArgs qa = qkv_args(m, n, table, positions, kc, vc, slot, seq_len, h, hkv, dh, q);
  rc(jla::linear_skinny_w4(x.data_ptr(), 0, w4.data_ptr(), s4.data_ptr(), nullptr, m, n, k, MODE_QKV, (float)rms_eps,
                           0, 0, &qa, stream()),
     "linear_qkv_w4");
}

// fused small-batch qkv projection + decode attention (gemv.hip qkv_attn_kernel): q [M, H, Dh] (scratch the
// attention workgroups read), the attention output out [M, H * Dh] (+ its packed copy); splits from qkv_attn_splits
void linear_qkv_attn(Tensor x, Tensor w, int64_t n, int64_t k, double rms_eps, Tensor table, Tensor positions,
                     Tensor kc, Tensor vc, Tensor slot, int64_t h, int64_t hkv, int64_t dh, Tensor q, Tensor kv_start,
                     Tensor out, c10::optional<Tensor> out_pack, Tensor ws, Tensor tickets, Tensor sync, int64_t t_cap,
                     int64_t splits, c10::optional<Tensor> x_packed, int64_t spl, c10::optional<Tensor> sk_ws,
                     c10::optional<Tensor> sk_tk, c10::optional<Tensor> o_w, int64_t o_n, int64_t o_k,
                     c10::optional<Tensor> o_h, c10::optional<Tensor> o_hb, c10::optional<Tensor> o_hb_pack,
                     int64_t tp_state) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "linear_qkv_attn: x bf16 [M, K]");
  const int64_t m = x.size(0);
  check(m <= 32, "linear_qkv_attn: M <= 32");
  jla::QKVArgs qa = qkv_args(m, n, table, positions, kc, vc, slot, 1, h, hkv, dh, q);
  for (auto* t : {&kv_start, &out, &ws, &tickets, &sync}) check_gpu(*t, "linear_qkv_attn arg");
  check(kv_start.scalar_type() == torch::kInt32 && kv_start.numel() == m, "kv_start int32 [B]");
  check(out.scalar_type() == torch::kBFloat16 && out.numel() == m * h * dh, "out bf16 [B, H * Dh]");
  check(ws.scalar_type() == torch::kFloat32 && ws.numel() >= m * hkv * splits * (h / hkv) * (dh + 4), "ws too small");
  check(tickets.scalar_type() == torch::kInt32 && tickets.numel() >= m * hkv, "tickets int32 [pairs]");
  check(sync.scalar_type() == torch::kInt32 && (size_t)sync.numel() >= jla::qkv_attn_sync_ints(),
        "sync int32 [qkv_attn_sync_ints()]");
  check(t_cap <= kc.size(2), "t_cap <= cache length");
  const jla::bf16_t* xp = packed_ptr(x_packed, m, k, "x_packed");
  check(spl == 1 || spl == 2, "linear_qkv_attn: spl 1 or 2");
  if (spl > 1) {  // the split qkv GEMV's slabs + tickets (skinny_workspace)
    check(sk_ws.has_value() && sk_tk.has_value(), "linear_qkv_attn spl 2: sk_ws and sk_tk (skinny_workspace)");
    check_gpu(*sk_ws, "sk_ws");
    check_gpu(*sk_tk, "sk_tk");
    check(sk_ws->scalar_type() == torch::kFloat32 && sk_tk->scalar_type() == torch::kInt32 &&
              sk_tk->numel() >= n / 16,
          "linear_qkv_attn: sk_ws fp32, sk_tk int32 [N / 16]");
    qa.sk_ws = ptr<float>(*sk_ws);
    qa.sk_tk = ptr<int32_t>(*sk_tk);
    qa.sk_ws_floats = (int)sk_ws->numel();
  }
  // the fused o projection (o_w): h += out @ Wo^T with the residual epilogue (tp_state 0) or the TP exchange
  jla::QKVArgs qo{};
  float* oh = nullptr;
  int o_mode = 0;
  if (o_w.has_value()) {
    check_packed(*o_w, o_n, o_k);
    check(o_k == h * dh, "linear_qkv_attn: Wo has H * Dh input columns");
    check(o_h.has_value() && o_hb.has_value(), "linear_qkv_attn: the fused o projection needs h and hb");
    check_gpu(*o_h, "h");
    check_gpu(*o_hb, "hb");
    check(o_h->scalar_type() == torch::kFloat32 && o_h->numel() == m * o_n && o_hb->scalar_type() == torch::kBFloat16 &&
              o_hb->numel() == m * o_n, "linear_qkv_attn: h fp32 / hb bf16 [M, N_o]");
    const int og = jla::qkv_attn_o_groups((int)m, (int)(h / hkv), (int)o_n, (int)o_k);
    check(og > 0, "linear_qkv_attn: the o projection cannot be fused at this shape (qkv_attn_o_groups)");
    oh = ptr<float>(*o_h);
    qo.res_bf16 = bf(*o_hb);
    qo.pack = packed_ptr(o_hb_pack, m, o_n, "o_hb_pack");
    o_mode = MODE_RESIDUAL;
    if (tp_state) {
      void* st = reinterpret_cast<void*>(tp_state);
      check(og <= jla::CAR_WG_COUNTERS && og * jla::TPRES_REGION <= jla::car_max_bytes(st),
            "linear_qkv_attn: too many o workgroups for the TP buffer");
      qo.tp = jla::car_device(st);
      o_mode = MODE_TPRESID;
    }
  }
  rc(jla::linear_qkv_attn(xp ? xp : cbf(x), w.data_ptr(), m, n, k, (float)rms_eps, qa, xp != nullptr, bf(out),
                          packed_ptr(out_pack, m, h * dh, "out_pack"), ptr<int32_t>(kv_start), ptr<float>(ws),
                          ptr<int32_t>(tickets), ptr<int32_t>(sync), (int)t_cap, (int)splits, (int)spl, stream(),
                          o_w.has_value() ? o_w->data_ptr() : nullptr, oh, (int)o_n, (int)o_k, o_mode,
                          o_w.has_value() ? &qo : nullptr),
     "linear_qkv_attn");
}

// The slab workspace of a K split -- [ks][M][N] (+ [ks][M] norm partials); gemm5: for any split, ks its effective
// split over 64-deep stages. False: this call needs none.
bool check_gemm_ws(const c10::optional<Tensor>& ws, int64_t k, int64_t ksplit, int64_t m, int64_t n, bool rms,
                   int64_t tile) {
  if (!is_g5(tile) && ksplit <= 1) return false;
  check(ws.has_value(), "gemm: a K split (gemm5: any plan) needs the slab workspace");
  check_gpu(*ws, "gemm ws");
  const int64_t ks = is_g5(tile) ? jla::gemm5_ksplit((int)k, (int)ksplit) : ksplit;
  check(ws->scalar_type() == torch::kFloat32 && ws->numel() >= ks * m * (n + (rms ? 1 : 0)), "gemm ws too small");
  return true;
}

// Tiled MFMA GEMM; ksplit > 1 -> split-K partials in ws + fixed-order reduce/epilogue kernel.
// rms_ws: optional fp32 scratch (>= M floats) for the row statistic of the fused norm on gemm4 plans without a K
// split (computed ahead of the GEMM by rms_rowinv); absent: the statistic is summed inside the main loop.
static float* rms_ws_ptr(const c10::optional<Tensor>& rws, int64_t m, size_t* floats) {
  *floats = 0;
  if (!rws.has_value()) return nullptr;
  check_gpu(*rws, "rms_ws");
  check(rws->scalar_type() == torch::kFloat32 && rws->numel() >= m, "rms_ws: fp32, >= M floats");
  *floats = rws->numel();
  return ptr<float>(*rws);
}

void gemm(Tensor x, Tensor w, int64_t n, int64_t k, Tensor out, int64_t mode, bool accumulate,
          c10::optional<Tensor> mirror, int64_t ksplit, c10::optional<Tensor> ws, double rms_eps, int64_t tile,
          c10::optional<Tensor> pack_out, c10::optional<Tensor> rms_ws, int64_t n_body) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(n_body >= 0 && (n_body == 0 || jla::gemm_tail_width((int)tile) > 0), "gemm n_body: tail-balanced tiles only");
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  check(mode >= 0 && mode <= 2, "gemm mode");
  const int64_t m = x.size(0);
  check_linear_out(out, m, n, mode);
  jla::bf16_t* mir = mode == 1 ? mirror_ptr(mirror, out.numel()) : nullptr;
  // packed copy of the bf16 output (decode M <= 64; the residual's mirror / the SwiGLU activation): written by the
  // split-K reduce epilogue, so only on that path
  jla::QKVArgs pqa{};
  if (pack_out.has_value()) {
    check(m <= SKINNY_MAX_M && (mode == 1 || mode == 2) && (mode != 1 || mir), "gemm pack_out: decode M, residual "
          "(with its mirror) or SwiGLU");
    check(ksplit > 1 || is_g5(tile), "gemm pack_out: the split-K reduce-kernel path only");
    pqa.pack = packed_ptr(pack_out, m, mode == 2 ? n / 2 : n, "pack_out");
  }
  const bool slabs = check_gemm_ws(ws, k, ksplit, m, n, rms_eps >= 0, tile);
  size_t rfl = 0;
  float* rws = rms_ws_ptr(rms_ws, m, &rfl);
  gemm_rc(jla::gemm(cbf(x), w.data_ptr(), out.data_ptr(), m, n, k, mode, accumulate,
                    out.scalar_type() == torch::kFloat32, mir, pqa.pack ? &pqa : nullptr,
                    slabs ? ptr<float>(*ws) : nullptr, slabs ? ws->numel() : 0, ksplit, stream(), (float)rms_eps,
                    (int)tile, rws, rfl, (int)n_body),
          "gemm");
}

// Tiled split-K qkv projection with the RoPE + KV-cache write in the reduce epilogue (x: bf16; rms_eps >= 0
// applies the fused RMSNorm statistic, otherwise x must already be scaled).
void gemm_qkv(Tensor x, Tensor w, int64_t n, int64_t k, Tensor table, Tensor positions, Tensor kc, Tensor vc,
              Tensor slot, int64_t seq_len, int64_t h, int64_t hkv, int64_t dh, Tensor q, int64_t ksplit,
              c10::optional<Tensor> ws, double rms_eps, int64_t tile, c10::optional<Tensor> rms_ws) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  const int64_t m = x.size(0);
  jla::QKVArgs qa = qkv_args(m, n, table, positions, kc, vc, slot, seq_len, h, hkv, dh, q);
  // without a K split (gemm5 apart): the GEMM's own RoPE / KV-write epilogue; else the reduce kernel's
  const bool slabs = check_gemm_ws(ws, k, ksplit, m, n, rms_eps >= 0, tile);
  size_t rfl = 0;
  float* rws = rms_ws_ptr(rms_ws, m, &rfl);
  gemm_rc(jla::gemm(cbf(x), w.data_ptr(), nullptr, m, n, k, MODE_QKV, 0, 0, nullptr, &qa,
                    slabs ? ptr<float>(*ws) : nullptr, slabs ? ws->numel() : 0, ksplit, stream(), (float)rms_eps,
                    (int)tile, rws, rfl),
          "gemm_qkv");
}

void rope_kv_write(Tensor qkv, Tensor table, Tensor positions, Tensor kc, Tensor vc, Tensor slot, int64_t seq_len,
                   int64_t h, int64_t hkv, int64_t dh, Tensor q) {
  for (auto* t : {&qkv, &table, &positions, &kc, &vc, &slot, &q}) check_gpu(*t, "rope_kv_write arg");
  check(qkv.scalar_type() == torch::kBFloat16 && kc.scalar_type() == torch::kBFloat16 &&
            vc.scalar_type() == torch::kBFloat16 && q.scalar_type() == torch::kBFloat16,
        "rope_kv_write bf16 tensors");
  check(table.scalar_type() == torch::kFloat32 && table.dim() == 3 && table.size(1) == dh / 2 && table.size(2) == 2,
        "rope table must be fp32 [L, Dh/2, 2]");
  check(positions.scalar_type() == torch::kInt32 && slot.scalar_type() == torch::kInt32, "int32 positions/slot");
  const int64_t m = qkv.size(0);
  check(qkv.dim() == 2 && qkv.size(1) == (h + 2 * hkv) * dh, "qkv shape");
  check(positions.numel() == m && m % seq_len == 0, "positions shape");
  const int64_t b = m / seq_len;
  check(kc.dim() == 4 && kc.size(0) == b && kc.size(1) == hkv && kc.size(3) == dh && vc.sizes() == kc.sizes(),
        "cache shape [B, Hkv, T, Dh]");
  check(q.numel() == m * h * dh, "q out shape");
  rc(jla::rope_kv_write(cbf(qkv), ptr<float>(table), table.size(0), ptr<int32_t>(positions), bf(kc), bf(vc),
                        ptr<int32_t>(slot), m, seq_len, h, hkv, dh, kc.size(2), bf(q), stream()),
     "rope_kv_write");
}

void check_attn(const Tensor& q, const Tensor& kc, const Tensor& vc, const Tensor& slot, const Tensor& kv_start,
                const c10::optional<Tensor>& key_mask, const Tensor& out) {
  for (auto* t : {&q, &kc, &vc, &slot, &kv_start, &out}) check_gpu(*t, "attention arg");
  check(q.scalar_type() == torch::kBFloat16 && kc.scalar_type() == torch::kBFloat16 &&
            vc.scalar_type() == torch::kBFloat16 && out.scalar_type() == torch::kBFloat16,
        "attention bf16 tensors");
  check(q.dim() == 4 && kc.dim() == 4 && kc.sizes() == vc.sizes(), "attention shapes");
  check(kc.size(0) == q.size(0) && kc.size(3) == q.size(3), "cache/q shape mismatch");
  check(q.size(2) % kc.size(1) == 0, "H must be a multiple of Hkv");
  check(slot.scalar_type() == torch::kInt32 && kv_start.scalar_type() == torch::kInt32 &&
            kv_start.numel() == q.size(0),
        "slot/kv_start");
  check(out.numel() == q.numel(), "attention out shape");
  if (key_mask.has_value()) {
    check_gpu(*key_mask, "key_mask");
    check(key_mask->scalar_type() == torch::kUInt8 && key_mask->dim() == 2 && key_mask->size(0) == q.size(0),
          "key_mask must be uint8 [B, L]");
  }
}

void attn_decode(Tensor q, Tensor kc, Tensor vc, Tensor slot, Tensor kv_start, c10::optional<Tensor> key_mask,
                 Tensor out, Tensor ws, Tensor tickets, int64_t t_cap, int64_t nsplit, c10::optional<Tensor> out_pack) {
  check_attn(q, kc, vc, slot, kv_start, key_mask, out);
  check(q.size(1) == 1, "attn_decode: one query per row");
  const int64_t b = q.size(0), h = q.size(2), dh = q.size(3), hkv = kc.size(1), T = kc.size(2);
  check(t_cap <= T, "t_cap exceeds the cache length");
  check_gpu(ws, "ws");
  check_gpu(tickets, "tickets");
  // the one resolver (kernels/attn_plan.h) says whether the shape is served and what the launch needs
  const jla::AttnPlanResult r = jla::attn_decode_plan(jla::attn_knobs(), b, h, hkv, dh, t_cap, key_mask.has_value());
  TORCH_CHECK(r.rc == 0, "jax_llama_amd._C: attn_decode: no plan (", r.why, "; see attn_plan.h)");
  TORCH_CHECK(nsplit == r.plan.nsplit, "jax_llama_amd._C: attn_decode: nsplit ", nsplit, " is not the plan's ",
              r.plan.nsplit, " (attn_decode_plan_check)");
  check(!out_pack.has_value() || r.plan.packs,
        "attn_decode: this launch does not write the packed copy (attn_decode_plan_check's packs)");
  check(ws.scalar_type() == torch::kFloat32 && (size_t)ws.numel() >= r.plan.ws_floats, "workspace too small");
  check(tickets.scalar_type() == torch::kInt32 && tickets.numel() >= r.plan.tickets, "tickets too small");
  const uint8_t* km = key_mask.has_value() ? ptr<uint8_t>(*key_mask) : nullptr;
  const int ml = key_mask.has_value() ? key_mask->size(1) : 0;
  rc(jla::attn_decode(cbf(q), cbf(kc), cbf(vc), ptr<int32_t>(slot), ptr<int32_t>(kv_start), km, ml, bf(out),
                      ptr<float>(ws), ptr<int32_t>(tickets), b, h, hkv, dh, T, t_cap, nsplit, stream(),
                      packed_ptr(out_pack, b, h * dh, "out_pack")),
     "attn_decode");
}

void attn_prefill(Tensor q, Tensor kc, Tensor vc, Tensor slot, Tensor kv_start, c10::optional<Tensor> key_mask,
                  Tensor out) {
  check_attn(q, kc, vc, slot, kv_start, key_mask, out);
  const uint8_t* km = key_mask.has_value() ? ptr<uint8_t>(*key_mask) : nullptr;
  const int ml = key_mask.has_value() ? key_mask->size(1) : 0;
  rc(jla::attn_prefill(cbf(q), cbf(kc), cbf(vc), ptr<int32_t>(slot), ptr<int32_t>(kv_start), km, ml, bf(out),
                       q.size(0), q.size(1), q.size(2), kc.size(1), q.size(3), kc.size(2), stream()),
     "attn_prefill");
}

// ---- the FP8 (e4m3) KV cache (kernels/kv8.hip): q bytes uint8 [B, Hkv, T, 128], scales fp32 [B, Hkv, T]
static void check_kv8(const Tensor& kq, const Tensor& ks, const Tensor& vq, const Tensor& vs, int64_t b, int64_t hkv,
                      const char* who) {
  for (auto* t : {&kq, &ks, &vq, &vs}) check_gpu(*t, who);
  check(kq.scalar_type() == torch::kUInt8 && vq.scalar_type() == torch::kUInt8 && kq.dim() == 4 && kq.size(0) == b &&
            kq.size(1) == hkv && kq.size(2) > 0 && kq.size(3) == jla::ATTN_DH && vq.sizes() == kq.sizes(),
        "fp8 KV cache: q bytes must be uint8 [B, Hkv, T, 128]");
  for (auto* t : {&ks, &vs})
    check(t->scalar_type() == torch::kFloat32 && t->dim() == 3 && t->size(0) == b && t->size(1) == hkv &&
              t->size(2) == kq.size(2),
          "fp8 KV cache: scales must be fp32 [B, Hkv, T]");
}

void rope_kv_write_q8(Tensor qkv, Tensor table, Tensor positions, Tensor kq, Tensor ks, Tensor vq, Tensor vs,
                      Tensor slot, int64_t seq_len, int64_t h, int64_t hkv, int64_t dh, Tensor q) {
  for (auto* t : {&qkv, &table, &positions, &slot, &q}) check_gpu(*t, "rope_kv_write_q8 arg");
  check(qkv.scalar_type() == torch::kBFloat16 && q.scalar_type() == torch::kBFloat16, "rope_kv_write_q8 bf16 tensors");
  check(dh == jla::ATTN_DH, "rope_kv_write_q8: Dh == 128");
  check(table.scalar_type() == torch::kFloat32 && table.dim() == 3 && table.size(0) > 0 && table.size(1) == dh / 2 &&
            table.size(2) == 2,
        "rope table must be fp32 [L, Dh/2, 2]");
  check(positions.scalar_type() == torch::kInt32 && slot.scalar_type() == torch::kInt32 && slot.numel() >= 1,
        "int32 positions/slot");
  const int64_t m = qkv.size(0);
  check(h > 0 && hkv > 0 && qkv.dim() == 2 && qkv.size(1) == (h + 2 * hkv) * dh, "qkv shape");
  check(seq_len > 0 && positions.numel() == m && m % seq_len == 0, "positions shape");
  check_kv8(kq, ks, vq, vs, m / seq_len, hkv, "rope_kv_write_q8 cache");
  check(q.numel() == m * h * dh, "q out shape");
  rc(jla::rope_kv_write_q8(cbf(qkv), ptr<float>(table), table.size(0), ptr<int32_t>(positions), ptr<uint8_t>(kq),
                           ptr<float>(ks), ptr<uint8_t>(vq), ptr<float>(vs), ptr<int32_t>(slot), m, seq_len, h, hkv, dh,
                           kq.size(2), bf(q), stream()),
     "rope_kv_write_q8");
}

// slots [0, n) of K and V as bf16 kout / vout [B, Hkv, n_out, 128], n <= n_out (rows past n are left as they are)
void kv8_dequant(Tensor kq, Tensor ks, Tensor vq, Tensor vs, int64_t n, Tensor kout, Tensor vout) {
  check(kq.dim() == 4, "kv8_dequant: q bytes must be uint8 [B, Hkv, T, 128]");
  const int64_t b = kq.size(0), hkv = kq.size(1);
  check_kv8(kq, ks, vq, vs, b, hkv, "kv8_dequant cache");
  check_gpu(kout, "kout");
  check_gpu(vout, "vout");
  check(kout.scalar_type() == torch::kBFloat16 && vout.scalar_type() == torch::kBFloat16 && kout.dim() == 4 &&
            kout.size(0) == b && kout.size(1) == hkv && kout.size(3) == jla::ATTN_DH && vout.sizes() == kout.sizes(),
        "kv8_dequant: outputs must be bf16 [B, Hkv, n_out, 128]");
  check(n >= 0 && n <= kq.size(2) && n <= kout.size(2), "kv8_dequant: n within the cache and the outputs");
  check(b * hkv <= INT32_MAX && kq.size(2) <= INT32_MAX, "kv8_dequant: sizes");
  rc(jla::kv8_dequant(ptr<uint8_t>(kq), ptr<float>(ks), ptr<uint8_t>(vq), ptr<float>(vs), bf(kout), bf(vout), b * hkv,
                      kq.size(2), n, kout.size(2), stream()),
     "kv8_dequant");
}

void attn_decode_q8(Tensor q, Tensor kq, Tensor ks, Tensor vq, Tensor vs, Tensor slot, Tensor kv_start,
                    c10::optional<Tensor> key_mask, Tensor out, int64_t t_cap, c10::optional<Tensor> ws,
                    c10::optional<Tensor> tickets) {
  for (auto* t : {&q, &slot, &kv_start, &out}) check_gpu(*t, "attn_decode_q8 arg");
  check(q.scalar_type() == torch::kBFloat16 && out.scalar_type() == torch::kBFloat16 && q.dim() == 4 && q.size(1) == 1,
        "attn_decode_q8: q bf16 [B, 1, H, Dh]");
  const int64_t b = q.size(0), h = q.size(2), dh = q.size(3);
  check(kq.dim() == 4, "attn_decode_q8: q bytes must be uint8 [B, Hkv, T, 128]");
  const int64_t hkv = kq.size(1), T = kq.size(2);
  check_kv8(kq, ks, vq, vs, b, hkv, "attn_decode_q8 cache");
  check(slot.scalar_type() == torch::kInt32 && slot.numel() >= 1 && kv_start.scalar_type() == torch::kInt32 &&
            kv_start.numel() == b,
        "slot/kv_start");
  check(out.numel() == q.numel(), "attention out shape");
  check(t_cap >= 0 && t_cap <= T, "t_cap exceeds the cache length");
  check(b <= 65535, "attn_decode_q8: at most 65535 rows");
  if (key_mask.has_value()) {
    check_gpu(*key_mask, "key_mask");
    check(key_mask->scalar_type() == torch::kUInt8 && key_mask->dim() == 2 && key_mask->size(0) == b,
          "key_mask must be uint8 [B, L]");
  }
  const jla::AttnQ8PlanResult r =
      jla::attn_decode_q8_plan(jla::attn_knobs(), b, h, hkv, dh, t_cap, key_mask.has_value());
  TORCH_CHECK(r.rc == 0, "jax_llama_amd._C: attn_decode_q8: no plan (", r.why, "; see attn_plan.h)");
  // a plan with key splits needs its workspace and tickets (attn_decode_q8_split_check); an unsplit one takes none
  float* wsp = nullptr;
  int32_t* tkp = nullptr;
  if (r.plan.nsplit > 1) {
    TORCH_CHECK(ws.has_value() && tickets.has_value(), "jax_llama_amd._C: attn_decode_q8: the plan splits the keys (nsplit ",
                r.plan.nsplit, "): ws and tickets are required (attn_decode_q8_split_check)");
    check_gpu(*ws, "ws");
    check_gpu(*tickets, "tickets");
    TORCH_CHECK(ws->scalar_type() == torch::kFloat32 && ws->device() == q.device() &&
                    (size_t)ws->numel() >= r.plan.ws_floats,
                "jax_llama_amd._C: attn_decode_q8: ws must be fp32 on q's device with at least B * H * nsplit * (128 + 4) = ",
                r.plan.ws_floats, " floats (attn_decode_q8_split_check)");
    TORCH_CHECK(tickets->scalar_type() == torch::kInt32 && tickets->device() == q.device() &&
                    tickets->numel() >= r.plan.tickets,
                "jax_llama_amd._C: attn_decode_q8: tickets must be int32 on q's device, one per (row, kv head) pair = ",
                r.plan.tickets, " (attn_decode_q8_split_check)");
    wsp = ptr<float>(*ws);
    tkp = ptr<int32_t>(*tickets);
  }
  const uint8_t* km = key_mask.has_value() ? ptr<uint8_t>(*key_mask) : nullptr;
  const int ml = key_mask.has_value() ? key_mask->size(1) : 0;
  rc(jla::attn_decode_q8(cbf(q), ptr<uint8_t>(kq), ptr<float>(ks), ptr<uint8_t>(vq), ptr<float>(vs),
                         ptr<int32_t>(slot), ptr<int32_t>(kv_start), km, ml, bf(out), b, h, hkv, dh, T, t_cap,
                         stream(), wsp, r.plan.ws_floats, tkp, r.plan.tickets),
     "attn_decode_q8");
}

void argmax(Tensor logits, Tensor idx, Tensor val) {
  check_gpu(logits, "logits");
  check_gpu(idx, "idx");
  check_gpu(val, "val");
  check(logits.scalar_type() == torch::kFloat32 && logits.dim() == 2, "logits must be fp32 [B, V]");
  check(idx.scalar_type() == torch::kInt32 && val.scalar_type() == torch::kFloat32 &&
            idx.numel() == logits.size(0) && val.numel() == logits.size(0),
        "argmax outputs");
  rc(jla::argmax(ptr<float>(logits), logits.size(0), logits.size(1), ptr<int32_t>(idx), ptr<float>(val), stream()),
     "argmax");
}

// Greedy lm_head: tiled GEMM (fused RMS when rms_eps >= 0) with the argmax in its epilogue; the fp32
// logits are never written. ws: fp32 >= gemm_argmax_workspace(m, n) floats.
void gemm_argmax(Tensor x, Tensor w, int64_t n, int64_t k, Tensor ws, double rms_eps, Tensor idx, Tensor val,
                 c10::optional<Tensor> rms_ws) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  const int64_t m = x.size(0);
  check_gpu(ws, "ws");
  check(ws.scalar_type() == torch::kFloat32 && (size_t)ws.numel() >= jla::gemm_argmax_workspace_floats(m, n),
        "gemm_argmax ws too small");
  check_gpu(idx, "idx");
  check_gpu(val, "val");
  check(idx.scalar_type() == torch::kInt32 && val.scalar_type() == torch::kFloat32 && idx.numel() == m &&
            val.numel() == m,
        "gemm_argmax outputs");
  size_t rfl = 0;
  float* rws = rms_ws_ptr(rms_ws, m, &rfl);
  rc(jla::gemm_argmax(cbf(x), w.data_ptr(), ptr<float>(ws), ws.numel(), m, n, k, (float)rms_eps, ptr<int32_t>(idx),
                      ptr<float>(val), stream(), rws, rfl),
     "gemm_argmax");
}

static void check_logprob_io(const Tensor& targets, const Tensor& tgt, const Tensor& mx, const Tensor& se, int64_t m,
                             int64_t col_offset) {
  for (auto* t : {&targets, &tgt, &mx, &se}) check_gpu(*t, "logprob arg");
  check(targets.scalar_type() == torch::kInt32 && targets.numel() == m, "targets must be int32 [M]");
  for (auto* t : {&tgt, &mx, &se})
    check(t->scalar_type() == torch::kFloat32 && t->numel() == m, "logprob outputs must be fp32 [M]");
  check(col_offset >= 0 && col_offset <= INT32_MAX, "col_offset");
}

// Scoring lm_head: tiled GEMM (fused RMS when rms_eps >= 0) with the log-sum-exp in its epilogue; the fp32 logits are
// never written. Per row of this weight shard: tgt = the logit at column targets - col_offset (0 outside [0, n)), mx =
// the row maximum, se = sum exp(logit - mx). ws: fp32 >= gemm_logprob_workspace(m, n) floats.
void gemm_logprob(Tensor x, Tensor w, int64_t n, int64_t k, Tensor ws, double rms_eps, Tensor targets,
                  int64_t col_offset, Tensor tgt, Tensor mx, Tensor se, c10::optional<Tensor> rms_ws) {
  check_gpu(x, "x");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  const int64_t m = x.size(0);
  check_gpu(ws, "ws");
  check(ws.scalar_type() == torch::kFloat32 && (size_t)ws.numel() >= jla::gemm_logprob_workspace_floats(m, n),
        "gemm_logprob ws too small");
  check_logprob_io(targets, tgt, mx, se, m, col_offset);
  size_t rfl = 0;
  float* rws = rms_ws_ptr(rms_ws, m, &rfl);
  gemm_rc(jla::gemm_logprob(cbf(x), w.data_ptr(), ptr<float>(ws), ws.numel(), m, n, k, (float)rms_eps,
                            ptr<int32_t>(targets), (int)col_offset, ptr<float>(tgt), ptr<float>(mx), ptr<float>(se),
                            stream(), rws, rfl),
          "gemm_logprob");
}

// the same triple from stored fp32 logits [B, V]
void logprob_rows(Tensor logits, Tensor targets, int64_t col_offset, Tensor tgt, Tensor mx, Tensor se) {
  check_gpu(logits, "logits");
  check(logits.scalar_type() == torch::kFloat32 && logits.dim() == 2 && logits.size(1) > 0,
        "logits must be fp32 [B, V]");
  check(logits.size(1) <= INT32_MAX, "logprob_rows: V too large");
  check_logprob_io(targets, tgt, mx, se, logits.size(0), col_offset);
  rc(jla::logprob_rows(ptr<float>(logits), logits.size(0), logits.size(1), ptr<int32_t>(targets), (int)col_offset,
                       ptr<float>(tgt), ptr<float>(mx), ptr<float>(se), stream()),
     "logprob_rows");
}

// stage 1 of the sampler: per-16384-chunk (jla::topk_chunks) top-K candidates (global indices = local + idx_offset)
void topk_chunk(Tensor logits, int64_t k, int64_t idx_offset, Tensor cv, Tensor ci) {
  for (auto* t : {&logits, &cv, &ci}) check_gpu(*t, "topk_chunk arg");
  check(logits.scalar_type() == torch::kFloat32 && logits.dim() == 2, "logits must be fp32 [B, V]");
  const int64_t b = logits.size(0), v = logits.size(1);
  check(k >= 1 && k <= 64 && k <= v, "topk_chunk: 1 <= k <= min(64, V)");
  const int64_t c = (int64_t)jla::topk_chunks(v) * k;
  check(cv.scalar_type() == torch::kFloat32 && ci.scalar_type() == torch::kInt32 && cv.numel() == b * c &&
            ci.numel() == b * c,
        "topk_chunk: candidates must be [B, chunks*k] fp32/int32");
  rc(jla::topk_chunk(ptr<float>(logits), b, v, k, idx_offset, ptr<float>(cv), ptr<int32_t>(ci), stream()),
     "topk_chunk");
}

// stage 2: merge [B, C] candidates -> sorted top-K (mode 0) or one sampled token per row (mode 1)
void topk_merge(Tensor cv, Tensor ci, int64_t k, int64_t mode, c10::optional<Tensor> out_v,
                c10::optional<Tensor> out_i, c10::optional<Tensor> nxt, double temperature, double top_p,
                int64_t seed, c10::optional<Tensor> step) {
  check_gpu(cv, "cv");
  check_gpu(ci, "ci");
  check(cv.dim() == 2 && cv.sizes() == ci.sizes() && cv.scalar_type() == torch::kFloat32 &&
            ci.scalar_type() == torch::kInt32,
        "topk_merge: candidates [B, C] fp32/int32");
  const int64_t b = cv.size(0), c = cv.size(1);
  check(k >= 1 && k <= 64 && k <= c && c <= 4096, "topk_merge: 1 <= k <= 64, k <= C <= 4096");
  float* ov = nullptr;
  int32_t* oi = nullptr;
  int32_t* nx = nullptr;
  const int32_t* st = nullptr;
  if (mode == 0) {
    check(out_v.has_value() && out_i.has_value(), "topk_merge mode 0 needs out_v/out_i");
    check_gpu(*out_v, "out_v");
    check_gpu(*out_i, "out_i");
    check(out_v->scalar_type() == torch::kFloat32 && out_i->scalar_type() == torch::kInt32 &&
              out_v->numel() == b * k && out_i->numel() == b * k,
          "topk_merge outputs [B, k]");
    ov = ptr<float>(*out_v);
    oi = ptr<int32_t>(*out_i);
  } else {
    check(mode == 1 && nxt.has_value() && step.has_value(), "topk_merge mode 1 needs nxt and step");
    check_gpu(*nxt, "nxt");
    check_gpu(*step, "step");
    check(nxt->scalar_type() == torch::kInt32 && nxt->numel() == b && step->scalar_type() == torch::kInt32,
          "topk_merge nxt [B] / step [1] int32");
    check(temperature > 0, "topk_merge: temperature > 0");
    nx = ptr<int32_t>(*nxt);
    st = ptr<int32_t>(*step);
  }
  rc(jla::topk_merge(ptr<float>(cv), ptr<int32_t>(ci), b, c, k, mode, ov, oi, nx, (float)temperature, (float)top_p,
                     (uint64_t)seed, st, stream()),
     "topk_merge");
}

void decode_update(Tensor nxt, Tensor finished, Tensor sequences, Tensor cur_len, Tensor tokens, Tensor positions,
                   Tensor slot, int64_t pad, int64_t eos) {
  for (auto* t : {&nxt, &finished, &sequences, &cur_len, &tokens, &positions, &slot}) {
    check_gpu(*t, "decode_update arg");
    check(t->scalar_type() == torch::kInt32, "decode_update: int32 tensors");
  }
  const int64_t b = nxt.numel();
  check(finished.numel() == b && tokens.numel() == b && positions.numel() == b && sequences.dim() == 2 &&
            sequences.size(0) == b,
        "decode_update shapes");
  rc(jla::decode_update(ptr<int32_t>(nxt), ptr<int32_t>(finished), ptr<int32_t>(sequences), ptr<int32_t>(cur_len),
                        ptr<int32_t>(tokens), ptr<int32_t>(positions), ptr<int32_t>(slot), b, sequences.size(1), pad,
                        eos, stream()),
     "decode_update");
}

// ---- logits processors (logits_proc.hip) ----
void process_logits(Tensor logits, Tensor sequences, Tensor cur_len, Tensor hist_start, int64_t col_offset,
                    int64_t vocab, double p, double inv_p, int64_t n, Tensor suppress, Tensor stop, Tensor min_len) {
  for (auto* t : {&logits, &sequences, &cur_len, &hist_start, &suppress, &stop, &min_len})
    check_gpu(*t, "process_logits arg");
  check(logits.scalar_type() == torch::kFloat32 && logits.dim() == 2, "process_logits: fp32 logits [B, V]");
  for (auto* t : {&sequences, &cur_len, &hist_start, &suppress, &stop, &min_len})
    check(t->scalar_type() == torch::kInt32, "process_logits: int32 tensors");
  const int64_t b = logits.size(0), v = logits.size(1);
  TORCH_CHECK_VALUE(v <= jla::process_logits_max_v(), "jax_llama_amd._C: process_logits: at most ",
                    jla::process_logits_max_v(), " logits per row (the LDS bitmap), got ", v);
  check(v >= 1 && col_offset >= 0 && vocab >= col_offset + v && vocab < (int64_t(1) << 31),
        "process_logits: 0 <= col_offset, col_offset + V <= vocab < 2^31");
  check(sequences.dim() == 2 && sequences.size(0) == b && sequences.size(1) >= 1 &&
            sequences.size(1) < (int64_t(1) << 30) && hist_start.numel() == b && cur_len.numel() == 1,
        "process_logits: sequences [B, L], hist_start [B], cur_len [1]");
  check(suppress.numel() == 64 && stop.numel() == 8 && min_len.numel() == 1,
        "process_logits: suppress [64], stop [8], min_len [1]");
  check(p > 0 && (float)p > 0.f && n >= 0 && n < (int64_t(1) << 30), "process_logits: p > 0, n >= 0");
  rc(jla::process_logits(ptr<float>(logits), b, v, ptr<int32_t>(sequences), sequences.size(1), ptr<int32_t>(cur_len),
                         ptr<int32_t>(hist_start), col_offset, vocab, (float)p, (float)inv_p, n,
                         ptr<int32_t>(suppress), ptr<int32_t>(stop), ptr<int32_t>(min_len), stream()),
     "process_logits");
}

void decode_update_set(Tensor nxt, Tensor finished, Tensor sequences, Tensor cur_len, Tensor tokens, Tensor positions,
                       Tensor slot, int64_t pad, Tensor stop) {
  for (auto* t : {&nxt, &finished, &sequences, &cur_len, &tokens, &positions, &slot, &stop}) {
    check_gpu(*t, "decode_update_set arg");
    check(t->scalar_type() == torch::kInt32, "decode_update_set: int32 tensors");
  }
  const int64_t b = nxt.numel();
  check(finished.numel() == b && tokens.numel() == b && positions.numel() == b && sequences.dim() == 2 &&
            sequences.size(0) == b && cur_len.numel() == 1 && slot.numel() == 1 && stop.numel() == 8,
        "decode_update_set shapes (stop: int32 [8])");
  rc(jla::decode_update_set(ptr<int32_t>(nxt), ptr<int32_t>(finished), ptr<int32_t>(sequences),
                            ptr<int32_t>(cur_len), ptr<int32_t>(tokens), ptr<int32_t>(positions), ptr<int32_t>(slot),
                            b, sequences.size(1), pad, ptr<int32_t>(stop), stream()),
     "decode_update_set");
}

// ---- beam search (beam.hip) ----
void check_beam_state(const Tensor& running_score, const Tensor& score, const Tensor& is_finished, const Tensor& inv_pen,
                      const Tensor& cur_len, const Tensor& alive, int64_t& b, int64_t& k, int64_t L, int64_t S) {
  for (auto* t : {&running_score, &score, &is_finished, &inv_pen, &cur_len, &alive}) check_gpu(*t, "beam state");
  check(running_score.scalar_type() == torch::kFloat32 && score.scalar_type() == torch::kFloat32 &&
            inv_pen.scalar_type() == torch::kFloat32 && is_finished.scalar_type() == torch::kInt32 &&
            cur_len.scalar_type() == torch::kInt32 && alive.scalar_type() == torch::kInt32,
        "beam state dtypes");
  check(running_score.dim() == 2, "beam: running_score [B, K]");
  b = running_score.size(0);
  k = running_score.size(1);
  check(b >= 1 && k >= 2 && k <= 8, "beam: B >= 1, 2 <= K <= 8");
  check(score.numel() == b * k && is_finished.numel() == b * k && cur_len.numel() == 1 && alive.numel() == 1,
        "beam state shapes");
  check(S >= 1 && S <= L && L < (1 << 30) && inv_pen.numel() == L + 1, "beam: 1 <= S <= L, inv_pen [L + 1]");
}

void beam_alive(Tensor running_score, Tensor score, Tensor is_finished, Tensor inv_pen, Tensor cur_len, Tensor alive,
                int64_t L, int64_t S, int64_t early, bool never_full) {
  int64_t b, k;
  check_beam_state(running_score, score, is_finished, inv_pen, cur_len, alive, b, k, L, S);
  check(early >= 0 && early <= 2, "beam: early_stopping code 0 / 1 / 2");
  rc(jla::beam_alive(ptr<float>(running_score), ptr<float>(score), ptr<int32_t>(is_finished), ptr<float>(inv_pen),
                     ptr<int32_t>(cur_len), ptr<int32_t>(alive), b, k, L, S, early, never_full ? 1 : 0, stream()),
     "beam_alive");
}

void beam_step(Tensor cand_v, Tensor cand_i, Tensor lse, Tensor running_seq, Tensor seq, Tensor running_score,
               Tensor score, Tensor is_finished, Tensor inv_pen, Tensor cur_len, Tensor slot, Tensor tokens,
               Tensor positions, Tensor alive, Tensor beam_idx, int64_t S, int64_t eos, int64_t early) {
  check(running_seq.dim() == 3, "beam_step: running_seq [B, K, L]");
  const int64_t L = running_seq.size(2);
  int64_t b, k;
  check_beam_state(running_score, score, is_finished, inv_pen, cur_len, alive, b, k, L, S);
  for (auto* t : {&cand_v, &cand_i, &lse, &running_seq, &seq, &slot, &tokens, &positions, &beam_idx})
    check_gpu(*t, "beam_step arg");
  check(cand_v.scalar_type() == torch::kFloat32 && lse.scalar_type() == torch::kFloat32, "beam_step: fp32 candidates");
  for (auto* t : {&cand_i, &running_seq, &seq, &slot, &tokens, &positions, &beam_idx})
    check(t->scalar_type() == torch::kInt32, "beam_step: int32 tensors");
  check(running_seq.size(0) == b && running_seq.size(1) == k && seq.sizes() == running_seq.sizes(),
        "beam_step: running_seq / seq [B, K, L]");
  check(cand_v.numel() == b * k * 2 * k && cand_i.numel() == b * k * 2 * k && lse.numel() == b * k,
        "beam_step: candidates [B*K, 2K], lse [B*K]");
  check(tokens.numel() == b * k && positions.numel() == b * k && beam_idx.numel() == b * k && slot.numel() == 1,
        "beam_step: tokens / positions / beam_idx [B*K], slot [1]");
  check(early >= 0 && early <= 2, "beam: early_stopping code 0 / 1 / 2");
  rc(jla::beam_step(ptr<float>(cand_v), ptr<int32_t>(cand_i), ptr<float>(lse), ptr<int32_t>(running_seq),
                    ptr<int32_t>(seq), ptr<float>(running_score), ptr<float>(score), ptr<int32_t>(is_finished),
                    ptr<float>(inv_pen), ptr<int32_t>(cur_len), ptr<int32_t>(slot), ptr<int32_t>(tokens),
                    ptr<int32_t>(positions), ptr<int32_t>(alive), ptr<int32_t>(beam_idx), b, k, L, S, eos, early,
                    stream()),
     "beam_step");
}

// t: one cache tensor [layers, B*K, heads, T] or [layers, B*K, heads, T, Dh], any 1-, 2- or 4-byte element type
void kv_beam_reorder(Tensor t, Tensor beam_idx, Tensor slot, int64_t k) {
  check_gpu(t, "kv_beam_reorder cache");
  check_gpu(beam_idx, "beam_idx");
  check_gpu(slot, "slot");
  check(beam_idx.scalar_type() == torch::kInt32 && slot.scalar_type() == torch::kInt32 && slot.numel() == 1,
        "kv_beam_reorder: int32 beam_idx, slot [1]");
  check(t.dim() == 4 || t.dim() == 5, "kv_beam_reorder: cache [layers, rows, heads, T(, Dh)]");
  check(k >= 2 && k <= 8 && t.size(1) % k == 0 && beam_idx.numel() == t.size(1), "kv_beam_reorder: rows = B * K");
  const int64_t rb = (t.dim() == 5 ? t.size(4) : 1) * t.element_size();
  check(rb % 4 == 0 && rb < (1 << 20) && t.size(3) < (1 << 30), "kv_beam_reorder: bytes per slot a multiple of 4");
  const int r = jla::kv_beam_reorder(t.data_ptr(), ptr<int32_t>(beam_idx), ptr<int32_t>(slot), t.size(0),
                                     t.size(1) / k, k, t.size(2), t.size(3), rb, stream());
  check(r != -2, "kv_beam_reorder: layers * groups and heads must each be <= 65535");
  rc(r, "kv_beam_reorder");
}

// ---- custom all-reduce (allreduce.hip) -------------------------------------------------------
py::tuple car_alloc(int64_t max_bytes, int64_t world) {
  void* buf = nullptr;
  void* sig = nullptr;
  hipIpcMemHandle_t hb, hs;
  rc(jla::car_alloc(max_bytes, world, &buf, &sig, &hb, &hs), "car_alloc");
  return py::make_tuple((int64_t)(uintptr_t)buf, (int64_t)(uintptr_t)sig,
                        py::bytes(reinterpret_cast<const char*>(&hb), sizeof(hb)),
                        py::bytes(reinterpret_cast<const char*>(&hs), sizeof(hs)));
}

int64_t car_init(int64_t rank, int64_t world, int64_t max_bytes, int64_t buf, int64_t sig, std::vector<std::string> hbufs,
                 std::vector<std::string> hsigs, double timeout_s) {
  check((int64_t)hbufs.size() == world && (int64_t)hsigs.size() == world, "car_init: one handle per rank");
  std::vector<hipIpcMemHandle_t> hb(world), hs(world);
  for (int64_t p = 0; p < world; ++p) {
    check(hbufs[p].size() == sizeof(hipIpcMemHandle_t) && hsigs[p].size() == sizeof(hipIpcMemHandle_t),
          "car_init: handle size");
    std::memcpy(&hb[p], hbufs[p].data(), sizeof(hipIpcMemHandle_t));
    std::memcpy(&hs[p], hsigs[p].data(), sizeof(hipIpcMemHandle_t));
  }
  void* state = nullptr;
  rc(jla::car_init(rank, world, max_bytes, reinterpret_cast<void*>(buf), reinterpret_cast<void*>(sig), hb.data(),
                   hs.data(), timeout_s, &state),
     "car_init");
  return (int64_t)(uintptr_t)state;
}

// out = sum over the TP group of in (same dtype, bf16/fp32)
void car_allreduce(int64_t state, Tensor in, Tensor out, bool two_shot) {
  check_gpu(in, "in");
  check_gpu(out, "out");
  check(in.scalar_type() == out.scalar_type() && in.numel() == out.numel(), "car_allreduce in/out");
  check(in.scalar_type() == torch::kBFloat16 || in.scalar_type() == torch::kFloat32, "car_allreduce dtype");
  const int64_t nbytes = in.numel() * in.element_size();
  check(nbytes % 16 == 0, "car_allreduce: bytes % 16");
  rc(jla::car_reduce(reinterpret_cast<void*>(state), 0, in.data_ptr(), out.data_ptr(), nullptr, nullptr, nbytes,
                     in.scalar_type() == torch::kBFloat16, two_shot, stream()),
     "car_allreduce");
}

// residual all-reduce of a row-parallel projection: h (fp32) += sum over ranks of partial; hb = bf16(h)
void car_allreduce_residual(int64_t state, Tensor partial, Tensor h, Tensor hb, bool two_shot,
                            c10::optional<Tensor> hb_pack) {
  check_gpu(partial, "partial");
  check_gpu(h, "h");
  check_gpu(hb, "hb");
  check(partial.scalar_type() == torch::kBFloat16 || partial.scalar_type() == torch::kFloat32, "partial dtype");
  check(h.scalar_type() == torch::kFloat32 && hb.scalar_type() == torch::kBFloat16, "h fp32 / hb bf16");
  check(h.numel() == partial.numel() && hb.numel() == partial.numel(), "residual shapes");
  const int64_t nbytes = partial.numel() * partial.element_size();
  check(nbytes % 16 == 0, "car_allreduce_residual: bytes % 16");
  const int64_t cols = h.size(-1);
  jla::bf16_t* hp = packed_ptr(hb_pack, h.numel() / cols, cols, "hb_pack");
  rc(jla::car_reduce(reinterpret_cast<void*>(state), 1, partial.data_ptr(), nullptr, ptr<float>(h), bf(hb), nbytes,
                     partial.scalar_type() == torch::kBFloat16, two_shot, stream(), hp, hp ? (int)cols : 0),
     "car_allreduce_residual");
}

// fused row-parallel decode projection (gemv.hip MODE_TPRESID): h (fp32) += sum over the TP group of x @ W^T, the
// partials exchanged as tagged granules in the GEMV's own epilogue; hb = bf16(h) (+ its packed copy). `state` is a
// custom all-reduce instance reserved for this path (its per-workgroup counters must not be shared)
void linear_tp_residual(int64_t state, Tensor x, Tensor w, int64_t n, int64_t k, Tensor h, Tensor hb, int64_t variant,
                        c10::optional<Tensor> x_packed, c10::optional<Tensor> hb_pack, c10::optional<Tensor> ws,
                        c10::optional<Tensor> tickets) {
  check_gpu(x, "x");
  check_gpu(h, "h");
  check_gpu(hb, "hb");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  const int64_t m = x.size(0);
  check(m >= 1 && m <= SKINNY_MAX_M, "linear_tp_residual: 1 <= M <= 64");
  check(h.scalar_type() == torch::kFloat32 && h.numel() == m * n && hb.scalar_type() == torch::kBFloat16 &&
            hb.numel() == m * n, "h fp32 / hb bf16 [M, N]");
  void* st = reinterpret_cast<void*>(state);
  // one TPRES_REGION per workgroup (at most 4096 workgroups: the counters), inside one slot
  const int64_t groups = n / 16;  // upper bound (1 tile per workgroup)
  check(groups <= jla::CAR_WG_COUNTERS && groups * jla::TPRES_REGION <= jla::car_max_bytes(st),
        "linear_tp_residual: too many workgroups for the buffer");
  jla::QKVArgs qa{};
  qa.res_bf16 = bf(hb);
  qa.pack = packed_ptr(hb_pack, m, n, "hb_pack");
  qa.tp = jla::car_device(st);
  // split-K variants take the shared decode workspace: only the last arriver of a column group exchanges
  run_skinny(x, w, n, k, h.data_ptr(), MODE_TPRESID, -1.0, true, true, &qa, variant, ws ? *ws : Tensor(),
             tickets ? *tickets : Tensor(), packed_ptr(x_packed, m, k, "x_packed"));
}

// Row-parallel tiled projection (decode batches past the GEMV's rows) with the TP all-reduce and residual add in its
// split-K reduce (gemm.hip gemm_reduce_tp_kernel): h (fp32) += sum over the group of x @ W^T, hb = bf16(h). A split plan
// (ksplit > 1, or a gemm5 tile) and the shared gemm workspace; one exchange region per 4096 output elements.
void gemm_tp_residual(int64_t state, Tensor x, Tensor w, int64_t n, int64_t k, Tensor h, Tensor hb, int64_t ksplit,
                      Tensor ws, int64_t tile) {
  check_gpu(x, "x");
  check_gpu(h, "h");
  check_gpu(hb, "hb");
  check_packed(w, n, k);
  check(x.dim() == 2 && x.size(1) == k && x.scalar_type() == torch::kBFloat16, "x must be bf16 [M, K]");
  const int64_t m = x.size(0);
  check(h.scalar_type() == torch::kFloat32 && h.numel() == m * n && hb.scalar_type() == torch::kBFloat16 &&
            hb.numel() == m * n, "h fp32 / hb bf16 [M, N]");
  void* st = reinterpret_cast<void*>(state);
  const int64_t groups = jla::gemm_tp_groups((int)m, (int)n);
  check(groups <= jla::CAR_WG_COUNTERS && groups * jla::TPRES_REGION <= jla::car_max_bytes(st),
        "gemm_tp_residual: the output does not fit the fused exchange buffer");
  check_gemm_ws(ws, k, ksplit, m, n, false, tile);  // (no split, gemm5 apart: no legal plan -- the exchange lives in the reduce)
  jla::QKVArgs qa{};
  qa.tp = jla::car_device(st);
  gemm_rc(jla::gemm(cbf(x), w.data_ptr(), h.data_ptr(), m, n, k, MODE_TPRESID, 1, 1, bf(hb), &qa, ptr<float>(ws),
                    ws.numel(), ksplit, stream(), -1.f, (int)tile, nullptr, 0),
          "gemm_tp_residual");
}

// (value fp32, index int32) all-gathers of the vocab-parallel sampler. mode 0: out_i[n] = index of the first max over
// ranks (out_v optional); mode 1: out_v/out_i [n / k, world * k]
void car_pairs(int64_t state, int64_t mode, Tensor vals, Tensor idx, int64_t idx_offset, int64_t k,
               c10::optional<Tensor> out_v, Tensor out_i) {
  check_gpu(vals, "vals");
  check_gpu(idx, "idx");
  check_gpu(out_i, "out_i");
  check(vals.scalar_type() == torch::kFloat32 && idx.scalar_type() == torch::kInt32 &&
            out_i.scalar_type() == torch::kInt32 && vals.numel() == idx.numel(),
        "car_pairs dtypes");
  const int64_t n = vals.numel();
  auto* st = reinterpret_cast<void*>(state);
  float* ov = nullptr;
  if (out_v.has_value()) {
    check_gpu(*out_v, "out_v");
    check(out_v->scalar_type() == torch::kFloat32 && out_v->numel() == out_i.numel(), "out_v");
    ov = ptr<float>(*out_v);
  }
  if (mode == 0) {
    check(out_i.numel() == n, "car_pairs argmax out shape");
  } else {
    check(mode == 1 && ov && k > 0 && n % k == 0 && out_i.numel() == n * jla::car_world(st), "car_pairs top-k shapes");
  }
  rc(jla::car_pairs(st, (int)mode, ptr<float>(vals), ptr<int32_t>(idx), (int)idx_offset, n, (int)k, ov,
                    ptr<int32_t>(out_i), stream()),
     "car_pairs");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {  // _C, or _C_dbg for the bounds-checked build
  m.doc() = "jax_llama_amd gfx950 (MI355X) HIP kernels";
  m.attr("SKINNY_MAX_M") = SKINNY_MAX_M;
  m.attr("ARCH") = "gfx950";
  m.def("embedding", &embedding, py::arg("ids"), py::arg("table"), py::arg("out"),
        py::arg("mirror") = py::none());
  m.def("rms_scale", &rms_scale);
  m.def("rmsnorm", &rmsnorm);
  m.def("residual_add", &residual_add);
  m.def("gemm_f32", &gemm_f32);
  m.def("prefetch", &prefetch, py::arg("t"), py::arg("grid") = 128);
  m.def("linear_skinny", &linear_skinny, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("out"),
        py::arg("mode"), py::arg("rms_eps"), py::arg("accumulate"), py::arg("variant"), py::arg("ws"),
        py::arg("tickets"), py::arg("mirror") = py::none(), py::arg("x_packed") = py::none(),
        py::arg("pack_out") = py::none());
  m.def("gemm", &gemm, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("out"), py::arg("mode"),
        py::arg("accumulate"), py::arg("mirror") = py::none(), py::arg("ksplit") = 1, py::arg("ws") = py::none(),
        py::arg("rms_eps") = -1.0, py::arg("tile") = 0, py::arg("pack_out") = py::none(),
        py::arg("rms_ws") = py::none(), py::arg("n_body") = 0);
  // (body, tail) n-tile counts of the tail-balanced gemm4 plan (tiles 18 / 19: width 192 / 256); (0, 0): not offered.
  // cus = 0: the current device's CU count
  m.def("gemm_tail_split", [](int64_t tiles_m, int64_t n, int64_t width, int64_t cus) {
    const int nb = jla::gemm_tail_split((int)tiles_m, (int)n, (int)width, cus > 0 ? (int)cus : jla::gemm_num_cus());
    return std::make_pair((int64_t)nb, nb > 0 ? (n - nb * width + 127) / 128 : (int64_t)0);
  }, py::arg("tiles_m"), py::arg("n"), py::arg("width"), py::arg("cus") = 0);
  // 0: a legal plan (kernels/gemm_plan.h, the CU count from the current device); else the code gemm() would fail with
  m.def("gemm_plan_check", [](int64_t m, int64_t n, int64_t k, int64_t mode, bool rms, int64_t ksplit, int64_t tile,
                              bool has_rms_ws, int64_t n_body) {
    return jla::gemm_plan_check((int)m, (int)n, (int)k, (int)mode, rms, (int)ksplit, (int)tile, has_rms_ws, (int)n_body);
  }, py::arg("m"), py::arg("n"), py::arg("k"), py::arg("mode"), py::arg("rms"), py::arg("ksplit"), py::arg("tile"),
     py::arg("has_rms_ws"), py::arg("n_body") = 0);
  // (rc, mt, nt, nw, deep, xp, ksplit) of a decode-GEMV call (kernels/gemv_plan.h): rc 0 and the resolved kernel form
  // (mt 0: nothing to launch), or the code linear_skinny() would fail with
  m.def("gemv_plan_check", [](int64_t m, int64_t n, int64_t k, int64_t mode, bool x_f32, bool x_packed,
                              int64_t variant) {
    const jla::GemvPlanResult r = jla::gemv_plan((int)m, (int)n, (int)k, (int)mode, x_f32, x_packed, (int)variant);
    const jla::GemvPlan& p = r.plan;
    return py::make_tuple(r.rc, p.mt, p.nt, p.nw, p.deep, p.xp, p.ksplit);
  }, py::arg("m"), py::arg("n"), py::arg("k"), py::arg("mode"), py::arg("x_f32"), py::arg("x_packed"),
     py::arg("variant"));
  // (rc, mt, nt, nw) of an FP8-weight decode-GEMV call (kernels/gemv_plan.h gemv_w8_plan); rc != 0: the dequant path
  m.def("gemv_w8_plan_check", [](int64_t m, int64_t n, int64_t k, int64_t mode, bool x_f32) {
    const jla::GemvPlanResult r = jla::gemv_w8_plan((int)m, (int)n, (int)k, (int)mode, x_f32);
    return py::make_tuple(r.rc, r.plan.mt, r.plan.nt, r.plan.nw);
  }, py::arg("m"), py::arg("n"), py::arg("k"), py::arg("mode"), py::arg("x_f32"));
  m.def("dequant_fp8", &dequant_fp8, py::arg("w8"), py::arg("scale"), py::arg("n"), py::arg("k"), py::arg("out"));
  m.def("linear_skinny_w8", &linear_skinny_w8, py::arg("x"), py::arg("w8"), py::arg("scale"), py::arg("n"),
        py::arg("k"), py::arg("out"), py::arg("mode"), py::arg("rms_eps"), py::arg("accumulate"),
        py::arg("mirror") = py::none(), py::arg("pack_out") = py::none());
  m.def("linear_qkv_w8", &linear_qkv_w8, py::arg("x"), py::arg("w8"), py::arg("scale"), py::arg("n"), py::arg("k"),
        py::arg("rms_eps"), py::arg("table"), py::arg("positions"), py::arg("kc"), py::arg("vc"), py::arg("slot"),
        py::arg("seq_len"), py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("q"));
  // (rc, mt, nt, nw) of an MXFP4-weight decode-GEMV call (kernels/gemv_plan.h gemv_w4_plan); rc != 0: the dequant path
  m.def("gemv_w4_plan_check", [](int64_t m, int64_t n, int64_t k, int64_t mode, bool x_f32) {
    const jla::GemvPlanResult r = jla::gemv_w4_plan((int)m, (int)n, (int)k, (int)mode, x_f32);
    return py::make_tuple(r.rc, r.plan.mt, r.plan.nt, r.plan.nw);
  }, py::arg("m"), py::arg("n"), py::arg("k"), py::arg("mode"), py::arg("x_f32"));
  m.def("dequant_fp4", &dequant_fp4, py::arg("w4"), py::arg("s4"), py::arg("n"), py::arg("k"), py::arg("out"));
  m.def("linear_skinny_w4", &linear_skinny_w4, py::arg("x"), py::arg("w4"), py::arg("s4"), py::arg("n"),
        py::arg("k"), py::arg("out"), py::arg("mode"), py::arg("rms_eps"), py::arg("accumulate"),
        py::arg("mirror") = py::none(), py::arg("pack_out") = py::none());
  m.def("linear_qkv_w4", &linear_qkv_w4, py::arg("x"), py::arg("w4"), py::arg("s4"), py::arg("n"), py::arg("k"),
        py::arg("rms_eps"), py::arg("table"), py::arg("positions"), py::arg("kc"), py::arg("vc"), py::arg("slot"),
        py::arg("seq_len"), py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("q"));
  m.def("gemv_variant_table", []() {  // {id: (packed x, split-K)}
    py::dict t;
    for (const jla::GemvVariant& v : jla::GEMV_VARIANTS) t[py::int_(v.id)] = py::make_tuple(v.xp, v.split);
    return t;
  });
  m.attr("GEMV_SPLIT_MAX_GROUPS") = jla::GEMV_SPLIT_MAX_GROUPS;
  m.def("gemm_qkv_direct_ok", [](int64_t m, int64_t tile, int64_t k) {
    return jla::gemm_qkv_direct_ok((int)m, (int)tile, (int)k) != 0;
  });
  m.def("gemm_set_g4_default", [](int64_t on) { jla::gemm_set_g4_default((int)on); });
  m.def("gemm_set_g4_group", [](int64_t gm) { jla::gemm_set_g4_group((int)gm); });
  m.def("gemm_qkv", &gemm_qkv, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("table"),
        py::arg("positions"), py::arg("kc"), py::arg("vc"), py::arg("slot"), py::arg("seq_len"), py::arg("h"),
        py::arg("hkv"), py::arg("dh"), py::arg("q"), py::arg("ksplit"), py::arg("ws"), py::arg("rms_eps") = -1.0,
        py::arg("tile") = 0, py::arg("rms_ws") = py::none());
  m.def("gemm_argmax", &gemm_argmax, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("ws"),
        py::arg("rms_eps"), py::arg("idx"), py::arg("val"), py::arg("rms_ws") = py::none());
  m.def("gemm_argmax_workspace", [](int64_t m, int64_t n) { return (int64_t)jla::gemm_argmax_workspace_floats(m, n); });
  m.def("gemm_logprob", &gemm_logprob, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("ws"),
        py::arg("rms_eps"), py::arg("targets"), py::arg("col_offset"), py::arg("tgt"), py::arg("mx"), py::arg("se"),
        py::arg("rms_ws") = py::none());
  m.def("gemm_logprob_workspace",
        [](int64_t m, int64_t n) { return (int64_t)jla::gemm_logprob_workspace_floats(m, n); });
  m.def("logprob_rows", &logprob_rows);
  m.def("gemm_ksplit", [](int64_t m, int64_t n, int64_t k) { return jla::gemm_ksplit(m, n, k); });
  m.def("rope_kv_write", &rope_kv_write);
  m.def("attn_set_impl", [](int64_t impl, int64_t waves_target) { jla::attn_set_impl(impl, waves_target); },
        py::arg("impl"), py::arg("waves_target") = 0);
  m.def("attn_reset_knobs", []() { jla::attn_reset_knobs(); }, "every attn_set_* knob back to its default");
  // (rc, why, kernel, nsplit, packs, ws_floats, tickets, rep, kpg, ring, fold, wpp, split_len) of the decode-attention
  // launch for this shape under the current knobs (kernels/attn_plan.h)
  m.def("attn_decode_plan_check", [](int64_t b, int64_t h, int64_t hkv, int64_t dh, int64_t t_cap, bool masked) {
    const jla::AttnPlanResult r =
        jla::attn_decode_plan(jla::attn_knobs(), (int)b, (int)h, (int)hkv, (int)dh, (int)t_cap, masked);
    const jla::AttnPlan& p = r.plan;
    return py::make_tuple(r.rc, r.why, r.rc ? "" : jla::attn_kernel_name(p.kernel), p.nsplit, p.packs,
                          (int64_t)p.ws_floats, p.tickets, p.rep, p.kpg, p.ring, p.fold, p.wpp, p.split_len);
  }, py::arg("b"), py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("t_cap"), py::arg("masked"));
  // the two older queries, now of the same plan (no key mask; packs does not depend on t_cap)
  m.def("attn_decode_splits", [](int64_t b, int64_t hkv, int64_t t, int64_t rep) {
    return jla::attn_decode_plan(jla::attn_knobs(), (int)b, (int)(hkv * rep), (int)hkv, jla::ATTN_DH, (int)t, false)
        .plan.nsplit;
  });
  m.def("attn_decode_packs", [](int64_t b, int64_t hkv, int64_t rep) {
    return (int)jla::attn_decode_plan(jla::attn_knobs(), (int)b, (int)(hkv * rep), (int)hkv, jla::ATTN_DH, 1, false)
        .plan.packs;
  });
  m.def("linear_qkv", &linear_qkv, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"), py::arg("rms_eps"),
        py::arg("table"), py::arg("positions"), py::arg("kc"), py::arg("vc"), py::arg("slot"), py::arg("seq_len"),
        py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("q"), py::arg("variant"), py::arg("ws"), py::arg("tickets"),
        py::arg("x_packed") = py::none());
  m.def("linear_qkv_attn", &linear_qkv_attn, py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"),
        py::arg("rms_eps"), py::arg("table"), py::arg("positions"), py::arg("kc"), py::arg("vc"), py::arg("slot"),
        py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("q"), py::arg("kv_start"), py::arg("out"),
        py::arg("out_pack"), py::arg("ws"), py::arg("tickets"), py::arg("sync"), py::arg("t_cap"), py::arg("splits"),
        py::arg("x_packed") = py::none(), py::arg("spl") = 1, py::arg("sk_ws") = py::none(),
        py::arg("sk_tk") = py::none(), py::arg("o_w") = py::none(), py::arg("o_n") = 0, py::arg("o_k") = 0,
        py::arg("o_h") = py::none(), py::arg("o_hb") = py::none(), py::arg("o_hb_pack") = py::none(),
        py::arg("tp_state") = 0);
  m.def("qkv_attn_splits", [](int64_t m, int64_t b, int64_t hkv, int64_t rep, int64_t t_cap, int64_t n, int64_t cus,
                              int64_t spl, int64_t o_groups) {
    return jla::qkv_attn_splits((int)m, (int)b, (int)hkv, (int)rep, (int)t_cap, (int)n, (int)cus, (int)spl,
                                (int)o_groups);
  }, py::arg("m"), py::arg("b"), py::arg("hkv"), py::arg("rep"), py::arg("t_cap"), py::arg("n"), py::arg("cus"),
     py::arg("spl") = 1, py::arg("o_groups") = 0);
  m.def("qkv_attn_o_groups", [](int64_t m, int64_t rep, int64_t n, int64_t k) {
    return jla::qkv_attn_o_groups((int)m, (int)rep, (int)n, (int)k);
  });
  m.def("qkv_attn_sync_ints", []() { return (int64_t)jla::qkv_attn_sync_ints(); });
  m.def("qkv_attn_set_o_nt", [](int64_t nt) { jla::qkv_attn_set_o_nt((int)nt); });
  m.def("qkv_attn_set_diag", [](int64_t d) { jla::qkv_attn_set_diag((int)d); });
  m.def("qkv_attn_set_stamps", [](c10::optional<Tensor> t) {  // int64 [>= grid * 8]; None: off (keep t alive)
    if (t.has_value()) {
      check_gpu(*t, "stamps");
      check(t->scalar_type() == torch::kInt64, "stamps int64");
    }
    jla::qkv_attn_set_stamps(t.has_value() ? reinterpret_cast<unsigned long long*>(t->data_ptr()) : nullptr);
  });
  m.def("qkv_attn_occupancy", [](int64_t m, int64_t rep, int64_t spl, int64_t o_groups) {
    return jla::qkv_attn_occupancy((int)m, (int)rep, (int)spl, (int)o_groups);
  }, py::arg("m"), py::arg("rep"), py::arg("spl") = 1, py::arg("o_groups") = 0);
  m.def("skinny_workspace", &skinny_workspace);
  m.def("linear_skinny_argmax", &linear_skinny_argmax);
  m.def("gemm_tp_residual", &gemm_tp_residual, py::arg("state"), py::arg("x"), py::arg("w"), py::arg("n"), py::arg("k"),
        py::arg("h"), py::arg("hb"), py::arg("ksplit"), py::arg("ws"), py::arg("tile"));
  m.def("gemm_tp_groups", [](int64_t m, int64_t n) { return (int64_t)jla::gemm_tp_groups((int)m, (int)n); });
  m.def("linear_tp_residual", &linear_tp_residual, py::arg("state"), py::arg("x"), py::arg("w"), py::arg("n"),
        py::arg("k"), py::arg("h"), py::arg("hb"), py::arg("variant"), py::arg("x_packed") = py::none(),
        py::arg("hb_pack") = py::none(), py::arg("ws") = py::none(), py::arg("tickets") = py::none());
  m.def("bounds_error", [](bool reset) {
    const int r = reset ? 1 : 0;
    return (int64_t)(jla::jla_bounds_norm_embed(r) | jla::jla_bounds_rope_kv(r) | jla::jla_bounds_sample(r) |
                     jla::jla_bounds_gemm(r) | jla::jla_bounds_gemv(r) | jla::jla_bounds_kv8(r) |
                     jla::jla_bounds_attn_decode(r) | jla::jla_bounds_attn_prefill(r) | jla::jla_bounds_beam(r) |
                     jla::jla_bounds_logits_proc(r));
  }, "OR of the bounds-checked debug build's error words (JLA_BOUNDS_* bits); always 0 in a release build",
        py::arg("reset") = false);
#ifdef JLA_DEBUG_BOUNDS
  m.attr("DEBUG_BOUNDS") = true;
#else
  m.attr("DEBUG_BOUNDS") = false;
#endif
  m.def("attn_set_diag", [](int64_t d) { jla::attn_set_diag((int)d); });
  // CU placement (placement.hip): streams restricted to a CU set (returned as the raw hipStream_t, wrapped by
  // torch.cuda.ExternalStream) and a census kernel recording each workgroup's HW_ID / XCC_ID
  m.def("cu_mask_stream", [](std::vector<int64_t> words) {
    std::vector<uint32_t> mk(words.begin(), words.end());
    hipStream_t s = nullptr;
    rc(jla::cu_mask_stream_create(mk.data(), (int)mk.size(), &s), "cu_mask_stream");
    return reinterpret_cast<int64_t>(s);
  });
  m.def("cu_mask_of", [](int64_t s, int64_t words) {
    std::vector<uint32_t> mk((size_t)words, 0u);
    rc(jla::cu_mask_stream_get(reinterpret_cast<hipStream_t>(s), mk.data(), (int)words), "cu_mask_of");
    return std::vector<int64_t>(mk.begin(), mk.end());
  });
  m.def("graph_kernel_nodes", [](int64_t g) {
    const int n = jla::graph_kernel_nodes(reinterpret_cast<hipGraph_t>(g));
    check(n >= 0, "graph_kernel_nodes: hipGraphGetNodes failed");
    return n;
  });
  m.def("stream_destroy", [](int64_t s) { rc(jla::stream_destroy(reinterpret_cast<hipStream_t>(s)), "stream_destroy"); });
  m.def("cu_census", [](Tensor out) {
    check_gpu(out, "out");
    check(out.scalar_type() == torch::kInt32 && out.numel() % 2 == 0, "cu_census: int32 [2 * blocks]");
    rc(jla::cu_census(reinterpret_cast<uint32_t*>(out.data_ptr()), (int)(out.numel() / 2), stream()), "cu_census");
  });
  m.def("attn_set_v3_kpg", [](int64_t m) { jla::attn_set_v3_kpg((int)m); });
  m.def("attn_set_v3_max_pairs", [](int64_t n) { jla::attn_set_v3_max_pairs((int)n); });
  m.def("attn_set_v5_max_pairs", [](int64_t n) { jla::attn_set_v5_max_pairs((int)n); });
  m.def("attn_set_v5_fold", [](int64_t n) { jla::attn_set_v5_fold((int)n); });
  m.def("clock_probe", [](int64_t iters, int64_t grid, Tensor out) {
    check(out.is_cuda() && out.scalar_type() == torch::kInt64 && out.numel() >= 3, "clock_probe: int64[3] on the GPU");
    rc(jla::clock_probe((int)iters, (int)grid, reinterpret_cast<unsigned long long*>(out.data_ptr()), stream()),
       "clock_probe");
  });
  m.def("gemm5_set_diag", [](int64_t d) { jla::gemm5_set_diag((int)d); });
  m.def("gemm5_ksplit", [](int64_t k, int64_t ks) { return jla::gemm5_ksplit((int)k, (int)ks); });
  m.def("attn_set_v6", [](int64_t mode) { jla::attn_set_v6((int)mode); });
  m.def("attn_set_v6_wpp", [](int64_t wpp) { jla::attn_set_v6_wpp((int)wpp); });
  m.def("attn_set_v6_diag", [](int64_t d) { jla::attn_set_v6_diag((int)d); });
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("slot"),
        py::arg("kv_start"), py::arg("key_mask").none(true), py::arg("out"), py::arg("ws"), py::arg("tickets"), py::arg("t_cap"),
        py::arg("nsplit"), py::arg("out_pack") = py::none());
  m.def("attn_prefill", &attn_prefill, py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("slot"),
        py::arg("kv_start"), py::arg("key_mask").none(true), py::arg("out"));
  m.def("attn_prefill_set_impl", [](int64_t impl) { jla::attn_prefill_set_impl((int)impl); });
  // the FP8 (e4m3) KV cache (kernels/kv8.hip)
  m.def("rope_kv_write_q8", &rope_kv_write_q8, py::arg("qkv"), py::arg("table"), py::arg("positions"), py::arg("kq"),
        py::arg("ks"), py::arg("vq"), py::arg("vs"), py::arg("slot"), py::arg("seq_len"), py::arg("h"), py::arg("hkv"),
        py::arg("dh"), py::arg("q"));
  m.def("kv8_dequant", &kv8_dequant, py::arg("kq"), py::arg("ks"), py::arg("vq"), py::arg("vs"), py::arg("n"),
        py::arg("kout"), py::arg("vout"));
  m.def("attn_decode_q8", &attn_decode_q8, py::arg("q"), py::arg("kq"), py::arg("ks"), py::arg("vq"), py::arg("vs"),
        py::arg("slot"), py::arg("kv_start"), py::arg("key_mask").none(true), py::arg("out"), py::arg("t_cap"),
        py::arg("ws") = py::none(), py::arg("tickets") = py::none());
  // (rc, why, waves, kpg, rep) of the fp8-cache decode-attention launch under the current knobs (kernels/attn_plan.h)
  m.def("attn_decode_q8_plan_check", [](int64_t b, int64_t h, int64_t hkv, int64_t dh, int64_t t_cap, bool masked) {
    const jla::AttnQ8PlanResult r =
        jla::attn_decode_q8_plan(jla::attn_knobs(), (int)b, (int)h, (int)hkv, (int)dh, (int)t_cap, masked);
    return py::make_tuple(r.rc, r.why, r.plan.waves, r.plan.kpg, r.plan.rep);
  }, py::arg("b"), py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("t_cap"), py::arg("masked"));
  m.def("attn_set_q8_waves", [](int64_t w) { jla::attn_set_q8_waves((int)w); },
        "waves per pair of the fp8-cache decode attention pinned to 1 / 8 (tests, A/B); 0: by shape");
  // (rc, why, nsplit, ws_floats, tickets) of the same plan: the key splits and what a split launch must be given
  m.def("attn_decode_q8_split_check", [](int64_t b, int64_t h, int64_t hkv, int64_t dh, int64_t t_cap, bool masked) {
    const jla::AttnQ8PlanResult r =
        jla::attn_decode_q8_plan(jla::attn_knobs(), (int)b, (int)h, (int)hkv, (int)dh, (int)t_cap, masked);
    return py::make_tuple(r.rc, r.why, r.plan.nsplit, (int64_t)r.plan.ws_floats, r.plan.tickets);
  }, py::arg("b"), py::arg("h"), py::arg("hkv"), py::arg("dh"), py::arg("t_cap"), py::arg("masked"));
  m.def("attn_set_q8_splits", [](int64_t n) { jla::attn_set_q8_splits((int)n); },
        "key splits per pair of the fp8-cache decode attention: 0 by shape, 1 never, n > 1 pinned (tests, A/B)");
  // (n_act, [(key_begin, key_end) per split]) of the valid keys [lo, hi) at kpg key rows per lane group: the geometry
  // function the 8-wave kernel calls (kernels/attn_plan.h attn_q8_split_range), on the host
  m.def("attn_q8_split_ranges", [](int64_t lo, int64_t hi, int64_t kpg, int64_t nsplit) {
    check(kpg >= 1 && kpg <= 8 && nsplit >= 1 && lo <= INT32_MAX && hi <= INT32_MAX && lo >= INT32_MIN &&
              hi >= INT32_MIN && nsplit <= INT32_MAX,
          "attn_q8_split_ranges: kpg in 1..8, nsplit >= 1, int32 keys");
    std::vector<std::pair<int, int>> ranges;
    int n_act = 0;
    for (int s = 0; s < (int)nsplit; ++s) {
      const jla::AttnQ8SplitRange r = jla::attn_q8_split_range((int)lo, (int)hi, 32 * (int)kpg, (int)nsplit, s);
      n_act = r.n_act;
      ranges.emplace_back(r.key_begin, r.key_end);
    }
    return py::make_tuple(n_act, ranges);
  }, py::arg("lo"), py::arg("hi"), py::arg("kpg"), py::arg("nsplit"));
  m.def("argmax", &argmax);
  m.def("topk_chunks", [](int64_t v) { return jla::topk_chunks(v); });
  m.def("car_alloc", &car_alloc);
  m.def("car_init", &car_init);
  m.def("car_allreduce", &car_allreduce, py::arg("state"), py::arg("inp"), py::arg("out"), py::arg("two_shot") = false);
  m.def("car_allreduce_residual", &car_allreduce_residual, py::arg("state"), py::arg("partial"), py::arg("h"),
        py::arg("hb"), py::arg("two_shot") = false, py::arg("hb_pack") = py::none());
  m.def("car_pairs", &car_pairs, py::arg("state"), py::arg("mode"), py::arg("vals"), py::arg("idx"),
        py::arg("idx_offset"), py::arg("k"), py::arg("out_v").none(true), py::arg("out_i"));
  m.def("car_set_gran_max", [](int64_t n) { jla::car_set_gran_max(n); });
  m.def("car_set_grid", [](int64_t st, int64_t grid) {
    rc(jla::car_set_grid(reinterpret_cast<void*>(st), (int)grid), "car_set_grid");
  });
  m.def("car_error", [](int64_t st) { return jla::car_error(reinterpret_cast<void*>(st)); });
  m.def("car_destroy", [](int64_t st) { jla::car_destroy(reinterpret_cast<void*>(st)); });
  m.def("car_free", [](int64_t buf, int64_t sig) {
    jla::car_free(reinterpret_cast<void*>(buf), reinterpret_cast<void*>(sig));
  }, "free car_alloc's buffers (a failed rendezvous)");
  m.def("topk_chunk", &topk_chunk);
  m.def("topk_merge", &topk_merge, py::arg("cv"), py::arg("ci"), py::arg("k"), py::arg("mode"),
        py::arg("out_v") = py::none(), py::arg("out_i") = py::none(), py::arg("nxt") = py::none(),
        py::arg("temperature") = 1.0, py::arg("top_p") = 1.0, py::arg("seed") = 0, py::arg("step") = py::none());
  m.def("decode_update", &decode_update);
  m.def("process_logits", &process_logits);
  m.def("decode_update_set", &decode_update_set);
  m.def("process_logits_max_v", []() { return (int64_t)jla::process_logits_max_v(); });
  m.def("beam_alive", &beam_alive);
  m.def("beam_step", &beam_step);
  m.def("kv_beam_reorder", &kv_beam_reorder);
}
