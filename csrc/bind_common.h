// Shared by the binding files (csrc/bind.cpp and csrc/bind_<family>.cpp): the launcher declarations, the stream and
// return-code helpers, the tensor checkers and the GEMM parameter-block fill helpers.
//
// Host-side validation lives in the bindings: every shape / dtype / stride / alignment a kernel assumes is checked
// BEFORE launch (a kernel that faults can reset every GPU on the node).  A caller-supplied tensor's pointer reaches a
// launcher only through a checker below (flat_ptr / rows; attention's 4-D views: bind_attn.cpp check_bshd), and every
// checker includes residency: a GPU tensor on the device of the op's first operand.  Tensors a binding allocates
// itself from a checked tensor's options are exempt.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <string>
#include <type_traits>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include "launchers.h"
#include "route.h"

namespace dllm {

using at::Tensor;
using c10::optional;

// one per family file; csrc/bind.cpp calls them all
void bind_rowwise(pybind11::module& m);  // norm, activation, dropout, colsum, embedding backward
void bind_loss(pybind11::module& m);     // cross entropy, distillation
void bind_optim(pybind11::module& m);    // sq_norm, AdamW, Adafactor
void bind_attn(pybind11::module& m);
void bind_gemm(pybind11::module& m);     // wgrad, fused, w4, GEGLU, LM-head CE
void bind_generate(pybind11::module& m); // beam, sample, kv_reorder
void bind_lora(pybind11::module& m);
void bind_reducer(pybind11::module& m);  // csrc/reducer.cpp

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "dllm kernel launch failed (", what, "): rc=", rc,
              rc > 0 ? std::string(" ") + hipGetErrorString((hipError_t)rc) : std::string(""));
}

inline bool has(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

inline bool is_bf16(const Tensor& t) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat, "unsupported dtype ",
              t.scalar_type());
  return t.scalar_type() == at::kBFloat16;
}

// ------------------------------------------------------------------------------------------- checkers
// Both return "" for a tensor the kernels can take, else the failed property as the rest of a sentence that starts
// with the operand's name ("must be ...").  `first` is the op's first operand (itself, for that operand).
using Dtypes = c10::ArrayRef<at::ScalarType>;

inline const char* dtype_name(at::ScalarType t) {
  switch (t) {
    case at::kBFloat16: return "bf16";
    case at::kFloat: return "fp32";
    case at::kLong: return "int64";
    case at::kInt: return "int32";
    case at::kByte: return "uint8";
    default: return c10::toString(t);
  }
}

inline std::string residency_fault(const Tensor& t, const Tensor& first) {
  if (!t.is_cuda()) return "must be a GPU tensor";
  if (t.device() != first.device()) return "must be on the device of the op's first operand";
  return "";
}

inline std::string dtype_fault(const Tensor& t, Dtypes dt) {  // {}: any (the op judges it, e.g. is_bf16 at the launch)
  if (dt.empty() || std::find(dt.begin(), dt.end(), t.scalar_type()) != dt.end()) return "";
  std::string s = "must be ";
  for (size_t i = 0; i < dt.size(); ++i) s += std::string(i ? " or " : "") + dtype_name(dt[i]);
  return s + ", got " + dtype_name(t.scalar_type());
}

inline std::string align_fault(const Tensor& t, int bytes) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0) return "";
  return "must be " + std::to_string(bytes) + "-byte aligned";
}

// Vectors, scalars and dense tensors a kernel walks as one flat array.
struct Flat {
  int64_t n;        // element count
  bool at_least;    // n is a lower bound
  bool contiguous;
  int align;        // base alignment in bytes
};
inline Flat exactly(int64_t n, int align = 1) { return {n, false, true, align}; }
inline Flat at_least(int64_t n, int align = 1) { return {n, true, true, align}; }
inline Flat scalar() { return {1, true, false, 1}; }  // a device scalar: only element 0 is read

inline std::string flat_fault(const Tensor& t, const Tensor& first, Dtypes dt, Flat f) {
  std::string why = residency_fault(t, first);
  if (why.empty()) why = dtype_fault(t, dt);
  if (!why.empty()) return why;
  if (f.at_least ? t.numel() < f.n : t.numel() != f.n)
    return std::string("must have ") + (f.at_least ? "at least " : "") + std::to_string(f.n) + " elements, got " +
           std::to_string(t.numel());
  if (f.contiguous && !t.is_contiguous()) return "must be contiguous";
  return align_fault(t, f.align);
}

template <class T, class... What>
T* flat_ptr(const Tensor& t, const Tensor& first, Dtypes dt, Flat f, const What&... what) {
  const std::string why = flat_fault(t, first, dt, f);
  TORCH_CHECK(why.empty(), what..., " ", why);
  return static_cast<T*>(t.data_ptr());
}

// the same for an optional operand: nullptr when it is not given
template <class T, class... What>
T* flat_ptr(const optional<Tensor>& t, const Tensor& first, Dtypes dt, Flat f, const What&... what) {
  return has(t) ? flat_ptr<T>(*t, first, dt, f, what...) : nullptr;
}

// Row-major 2-D operands: unit inner stride, a row stride that is a multiple of `ld_mult` elements, a base aligned to
// `align` bytes.  The named constants are the kernels' row accesses; shape() / dense() / range() add what one op needs
// on top.
struct Mat {
  int ld_mult, align;
  int64_t nrows = -1, ncols = -1;  // -1: any
  bool ld_ge_cols = false;         // row stride >= column count (rows do not overlap)
  int64_t range_rows = 0;          // > 0: range_rows rows span < 2^31 bytes (32-bit buffer-descriptor offsets)
  Mat shape(int64_t r, int64_t c) const { Mat m = *this; m.nrows = r; m.ncols = c; return m; }
  Mat dense() const { Mat m = *this; m.ld_ge_cols = true; return m; }
  Mat range(int64_t r) const { Mat m = *this; m.range_rows = r; return m; }
};
constexpr Mat kRows16{8, 16};  // bf16 rows read as 16-B vectors
constexpr Mat kRows8{4, 8};    // bf16 rows read as 8-B vectors
constexpr Mat kRows4{2, 4};    // bf16 rows read as 4-B pairs

inline std::string mat_fault(const Tensor& t, const Tensor& first, Dtypes dt, const Mat& m) {
  std::string why = residency_fault(t, first);
  if (why.empty()) why = dtype_fault(t, dt);
  if (!why.empty()) return why;
  if (t.dim() != 2 || t.stride(1) != 1) return "must be 2-D with unit inner stride";
  if ((m.nrows >= 0 && t.size(0) != m.nrows) || (m.ncols >= 0 && t.size(1) != m.ncols))
    return "must be [" + (m.nrows >= 0 ? std::to_string(m.nrows) : std::string("*")) + ", " +
           (m.ncols >= 0 ? std::to_string(m.ncols) : std::string("*")) + "], got [" + std::to_string(t.size(0)) + ", " +
           std::to_string(t.size(1)) + "]";
  if (t.stride(0) % m.ld_mult != 0)
    return "needs a row stride in multiples of " + std::to_string(m.ld_mult) + " elements, got " +
           std::to_string(t.stride(0));
  if (m.ld_ge_cols && t.stride(0) < t.size(1)) return "needs a row stride >= its column count";
  if (m.range_rows > 0 && m.range_rows * t.stride(0) * (int64_t)t.element_size() >= (1LL << 31))
    return "rows too long: " + std::to_string(m.range_rows) + " of them must span < 2^31 bytes";
  return align_fault(t, m.align);
}

// a checked matrix as the kernels take it: base pointer and row stride (elements)
template <class T>
struct Rows {
  T* ptr;
  long ld;
};

template <class T, class... What>
Rows<T> rows(const Tensor& t, const Tensor& first, Dtypes dt, const Mat& m, const What&... what) {
  const std::string why = mat_fault(t, first, dt, m);
  TORCH_CHECK(why.empty(), what..., " ", why);
  return {static_cast<T*>(t.data_ptr()), (long)t.stride(0)};
}

// the non-throwing form, for the *_supported predicates: false, or the checked matrix in `out`
template <class T>
bool try_rows(const Tensor& t, const Tensor& first, Dtypes dt, const Mat& m, Rows<T>& out) {
  if (!mat_fault(t, first, dt, m).empty()) return false;
  out = {static_cast<T*>(t.data_ptr()), (long)t.stride(0)};
  return true;
}

// ------------------------------------------------------------------------------------------- GEMM parameter blocks
// the dropout fields of GemmFusedParams / GemmW4Params; thr: the 16-bit keep threshold of csrc/common.h drop_threshold
template <class P>
void set_dropout(P& p, double prob, int64_t seed) {
  p.p = (float)prob;
  p.scale = prob > 0.0 ? (float)(1.0 / (1.0 - prob)) : 1.f;
  p.seed = (uint32_t)seed;
  const double t = prob * 65536.0;
  p.thr = t >= 65535.0 ? 0xFFFFu : (uint32_t)t;
}

// operands, leading dimensions, sizes and 256 x 256 tile counts (ragged edges round up) of the same two blocks
template <class P>
void set_gemm(P& p, Rows<const uint16_t> a, Rows<const uint16_t> b, Rows<uint16_t> c, int64_t M, int64_t N, int64_t K) {
  p.A = a.ptr; p.B = b.ptr; p.C = c.ptr;
  p.lda = a.ld; p.ldb = b.ld; p.ldc = c.ld;
  p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.tm = (int)((M + 255) / 256);
  p.tn = (int)((N + 255) / 256);
}

}  // namespace dllm
