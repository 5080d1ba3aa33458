// LoRA (csrc/lora.hip): the fused low-rank adapter kernels.
#include "bind_common.h"

namespace dllm {
namespace {

// A bf16 GPU matrix whose rows are 16-B aligned vectors of a multiple of 8 columns (unit inner stride, row stride a
// multiple of 8): a contiguous tensor or a column slice of one.
template <class T>
Rows<T> lora_wide(const Tensor& t, const Tensor& first, const char* fn, const char* n) {
  const auto r = rows<T>(t, first, at::kBFloat16, kRows16, fn, ": ", n);
  TORCH_CHECK(t.size(1) % 8 == 0, fn, ": ", n,
              " needs a column count and a row stride that are multiples of 8, got ", t.size(1), " / ", t.stride(0));
  TORCH_CHECK(t.size(0) < INT_MAX && t.size(1) < INT_MAX, fn, ": ", n, " too large");
  return r;
}

// A contiguous, 16-B aligned bf16 GPU matrix with the rank on one side (1 .. 64)
const void* lora_small(const Tensor& t, const Tensor& first, int64_t r, const char* fn, const char* n) {
  const void* p = flat_ptr<const void>(t, first, at::kBFloat16, at_least(0, 16), fn, ": ", n);
  TORCH_CHECK(t.dim() == 2, fn, ": ", n, " must be a contiguous matrix");
  TORCH_CHECK(r >= 1 && r <= 64, fn, ": the rank must be 1 .. 64, got ", r);
  return p;
}

// t[N, r] = bf16(alpha * (keep . x) A^T): x [N, K] (rows may be strided: a column slice), A [r, K]
Tensor lora_down(const Tensor& x, const Tensor& A, double alpha, double p, int64_t seed, int64_t row0) {
  const auto xr = lora_wide<const void>(x, x, "lora_down", "x");
  const void* Ap = lora_small(A, x, A.dim() == 2 ? A.size(0) : 0, "lora_down", "A");
  TORCH_CHECK(A.size(1) == x.size(1), "lora_down: A must be [r, K] with x's K, got ", A.sizes(), " for x ", x.sizes());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "lora_down: p must be in [0, 1)");
  const int N = x.size(0), K = x.size(1), r = A.size(0);
  auto t = at::empty({N, r}, x.options());
  check_rc(dllm_lora_down(xr.ptr, xr.ld, Ap, t.data_ptr(), N, K, r, (float)alpha, (float)p, (uint32_t)seed,
                          (uint32_t)row0, stream()),
           "lora_down");
  return t;
}

// y[:, c0:c0+n] += alpha * (keep .) (t M): t [N, r]; M [n, r], or [r, n] with kmajor; y [N, ld] in place
void lora_up(const Tensor& t, const Tensor& M, bool kmajor, double alpha, Tensor& y, int64_t c0, int64_t n, double p,
             int64_t seed, int64_t row0) {
  const auto yr = lora_wide<void>(y, y, "lora_up", "y");
  const void* tp = lora_small(t, y, t.dim() == 2 ? t.size(1) : 0, "lora_up", "t");
  const int64_t r = t.size(1);
  const void* Mp = lora_small(M, y, r, "lora_up", "M");
  TORCH_CHECK(t.size(0) == y.size(0), "lora_up: t and y need the same rows");
  TORCH_CHECK(n > 0 && n % 8 == 0 && c0 >= 0 && c0 % 8 == 0 && c0 + n <= y.size(1),
              "lora_up: the slice [c0, c0 + n) must lie inside y's columns with c0 and n multiples of 8, got c0 ", c0,
              " n ", n, " of ", y.size(1));
  TORCH_CHECK(kmajor ? (M.size(0) == r && M.size(1) == n) : (M.size(0) == n && M.size(1) == r),
              "lora_up: M must be ", kmajor ? "[r, n]" : "[n, r]", ", got ", M.sizes());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "lora_up: p must be in [0, 1)");
  check_rc(dllm_lora_up(tp, (int)r, Mp, kmajor ? 1 : 0, yr.ptr, yr.ld, (int)c0, (int)n, (int)y.size(0), (float)alpha,
                        (float)p, (uint32_t)seed, (uint32_t)row0, stream()),
           "lora_up");
}

std::vector<int64_t> lora_wgrad_splits(int64_t N) {
  const int64_t per = dllm_lora_wgrad_split_rows(N);  // tokens per split
  return {N > 0 ? (N + per - 1) / per : 0, per};
}

// G (+)= alpha * (keep . W)^T S over tokens: W [N, wc] (rows may be strided), S [N, r]; G [wc, r] (wide_major) or
// [r, wc], fp32 or bf16, contiguous.  Fixed token splits summed in order: bitwise reproducible.
void lora_wgrad(const Tensor& W, const Tensor& S, double alpha, Tensor& G, bool wide_major, bool beta, double p,
                int64_t seed, int64_t row0) {
  const auto Wr = lora_wide<const void>(W, W, "lora_wgrad", "W");
  const void* Sp = lora_small(S, W, S.dim() == 2 ? S.size(1) : 0, "lora_wgrad", "S");
  TORCH_CHECK(S.size(0) == W.size(0), "lora_wgrad: W and S need the same rows");
  const int64_t N = W.size(0), wc = W.size(1), r = S.size(1);
  TORCH_CHECK(G.dim() == 2, "lora_wgrad: G must be a contiguous fp32 / bf16 GPU matrix");
  void* Gp = flat_ptr<void>(G, W, {at::kFloat, at::kBFloat16}, at_least(0), "lora_wgrad: G");
  TORCH_CHECK(wide_major ? (G.size(0) == wc && G.size(1) == r) : (G.size(0) == r && G.size(1) == wc),
              "lora_wgrad: G must be ", wide_major ? "[wc, r]" : "[r, wc]", ", got ", G.sizes());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "lora_wgrad: p must be in [0, 1)");
  if (N == 0) return;
  const auto sp = lora_wgrad_splits(N);
  auto part = at::empty({sp[0], wc * r}, W.options().dtype(at::kFloat));
  check_rc(dllm_lora_wgrad(Wr.ptr, Wr.ld, (int)wc, Sp, (int)r, part.data_ptr<float>(), (int)N, (int)sp[1],
                           wide_major ? 1 : 0, Gp, G.scalar_type() == at::kBFloat16 ? 1 : 0, (float)alpha,
                           beta ? 1 : 0, (float)p, (uint32_t)seed, (uint32_t)row0, stream()),
           "lora_wgrad");
}

}  // namespace

void bind_lora(pybind11::module& m) {
  m.def("lora_down", &lora_down, "t = bf16(alpha * (keep . x) A^T) (csrc/lora.hip)", py::arg("x"), py::arg("A"),
        py::arg("alpha") = 1.0, py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("row0") = 0);
  m.def("lora_up", &lora_up, "y[:, c0:c0+n] += alpha * (keep .) (t M), in place", py::arg("t"), py::arg("M"),
        py::arg("kmajor"), py::arg("alpha"), py::arg("y"), py::arg("c0"), py::arg("n"), py::arg("p") = 0.0,
        py::arg("seed") = 0, py::arg("row0") = 0);
  m.def("lora_wgrad", &lora_wgrad, "G (+)= alpha * (keep . W)^T S over tokens, fixed splits summed in order",
        py::arg("W"), py::arg("S"), py::arg("alpha"), py::arg("G"), py::arg("wide_major"), py::arg("beta") = true,
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("row0") = 0);
  m.def("lora_wgrad_splits", &lora_wgrad_splits, "(splits, tokens per split) of lora_wgrad for N tokens");
  m.attr("lora_wgrad_rows") = dllm_lora_wgrad_rows();
  m.attr("lora_wgrad_max_splits") = dllm_lora_wgrad_max_splits();
}

}  // namespace dllm
