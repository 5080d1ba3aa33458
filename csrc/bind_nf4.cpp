// NF4 frozen base weights (csrc/nf4.hip): quantiser, dequantiser and the GEMMs on the 4-bit codes.
#include "bind_common.h"

namespace dllm {
namespace {

// the quantised weight of an op: codes uint8 [N, K/2] and absmax fp32 [N, K/64], contiguous, N and K multiples of 64
struct Nf4 {
  const uint8_t* codes;
  const float* absmax;
  int64_t N, K;
};

Nf4 nf4_weight(const Tensor& codes, const Tensor& absmax, const Tensor& first, const char* fn) {
  TORCH_CHECK(codes.dim() == 2 && absmax.dim() == 2, fn, ": codes and absmax must be matrices");
  const int64_t N = codes.size(0), K = codes.size(1) * 2;
  TORCH_CHECK(N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, fn, ": the weight's N and K must be multiples of 64, got [",
              N, ", ", K, "]");
  TORCH_CHECK(N < INT_MAX && K < INT_MAX, fn, ": weight too large");
  Nf4 w;
  w.codes = flat_ptr<const uint8_t>(codes, first, at::kByte, exactly(N * K / 2, 16), fn, ": codes");
  w.absmax = flat_ptr<const float>(absmax, first, at::kFloat, exactly(N * K / 64, 4), fn, ": absmax");
  TORCH_CHECK(absmax.size(0) == N, fn, ": absmax must be [N, K / 64], got ", absmax.sizes());
  w.N = N;
  w.K = K;
  return w;
}

std::vector<Tensor> nf4_quantize(const Tensor& w) {
  TORCH_CHECK(w.dim() == 2, "nf4_quantize: w must be a matrix");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N > 0 && N % 64 == 0 && K > 0 && K % 64 == 0, "nf4_quantize: w's N and K must be multiples of 64, got ",
              w.sizes());
  const void* wp = flat_ptr<const void>(w, w, {at::kBFloat16, at::kFloat}, exactly(N * K, 16), "nf4_quantize: w");
  auto codes = at::empty({N, K / 2}, w.options().dtype(at::kByte));
  auto absmax = at::empty({N, K / 64}, w.options().dtype(at::kFloat));
  check_rc(dllm_nf4_quantize(wp, is_bf16(w) ? 1 : 0, codes.data_ptr<uint8_t>(), absmax.data_ptr<float>(), N, K,
                             stream()),
           "nf4_quantize");
  return {codes, absmax};
}

Tensor nf4_dequant(const Tensor& codes, const Tensor& absmax) {
  const Nf4 w = nf4_weight(codes, absmax, codes, "nf4_dequant");
  auto out = at::empty({w.N, w.K}, codes.options().dtype(at::kBFloat16));
  check_rc(dllm_nf4_dequant(w.codes, w.absmax, out.data_ptr(), w.N, w.K, stream()), "nf4_dequant");
  return out;
}

// NT (nn = false): x [M, K] -> [M, N] = x . deq(W)^T (+ bias [N]); NN: x [M, N] -> [M, K] = x . deq(W).  x: bf16 rows
// with unit inner stride, a row stride % 8 == 0, 16-B aligned (a contiguous matrix or a column slice of one).
Tensor gemm_nf4(const Tensor& x, const Tensor& codes, const Tensor& absmax, const optional<Tensor>& bias, bool nn) {
  const Nf4 w = nf4_weight(codes, absmax, x, "gemm_nf4");
  const int64_t red = nn ? w.N : w.K, outc = nn ? w.K : w.N;
  const auto xr = rows<const void>(x, x, at::kBFloat16, kRows16.shape(-1, red).dense(), "gemm_nf4: x");
  TORCH_CHECK(x.size(0) < INT_MAX, "gemm_nf4: x too large");
  TORCH_CHECK(!(nn && has(bias)), "gemm_nf4: the NN form takes no bias");
  const void* bp = flat_ptr<const void>(bias, x, at::kBFloat16, exactly(w.N, 8), "gemm_nf4: bias");
  auto out = at::empty({x.size(0), outc}, x.options());
  check_rc(dllm_gemm_nf4(xr.ptr, xr.ld, w.codes, w.absmax, bp, out.data_ptr(), outc, (int)x.size(0), (int)w.N,
                         (int)w.K, nn ? 1 : 0, stream()),
           "gemm_nf4");
  return out;
}

}  // namespace

void bind_nf4(pybind11::module& m) {
  m.def("nf4_quantize", &nf4_quantize, "(codes uint8 [N, K/2], absmax fp32 [N, K/64]) of a bf16 / fp32 [N, K] weight");
  m.def("nf4_dequant", &nf4_dequant, "bf16 [N, K] = bf16(NF4[code] * absmax)", py::arg("codes"), py::arg("absmax"));
  m.def("gemm_nf4", &gemm_nf4, "x . deq(W)^T (+ bias) (nn = False) or x . deq(W) (nn = True) on the 4-bit codes",
        py::arg("x"), py::arg("codes"), py::arg("absmax"), py::arg("bias") = py::none(), py::arg("nn") = false);
  m.attr("nf4_decode_rows") = dllm_nf4_decode_rows();
}

}  // namespace dllm
