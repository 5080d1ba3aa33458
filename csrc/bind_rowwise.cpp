// Row-wise kernels: norms (csrc/norm.hip), activations and dropout (csrc/act.hip), column sums (csrc/colsum.hip,
// csrc/norm.hip), the embedding backward (csrc/embed.hip) and the rotary position embedding (csrc/rope.hip).
#include "bind_common.h"

namespace dllm {
namespace {

// a dense [N, d] activation of either dtype: the op's first operand.  The dtype is judged by is_bf16 at the launch.
const void* dense_rows(const Tensor& x, const char* name, const char* shape_msg) {
  const void* p = flat_ptr<const void>(x, x, {}, at_least(0), name);
  TORCH_CHECK(x.dim() == 2, shape_msg);
  return p;
}

// ------------------------------------------------------------------------------------------- norms
std::vector<Tensor> norm_fwd(const Tensor& x, const optional<Tensor>& resid, const Tensor& w,
                             const optional<Tensor>& b, double eps, double p, int64_t seed, int64_t kind,
                             bool want_s, double w_offset) {
  const void* xp = dense_rows(x, "x", "x must be contiguous [N, d]");
  const int N = x.size(0), d = x.size(1);
  TORCH_CHECK(d % 4 == 0 && d <= 2048, "norm: d must be a multiple of 4 and <= 2048, got ", d);
  const void* wp = flat_ptr<const void>(w, x, x.scalar_type(), exactly(d), "norm weight");
  if (has(resid)) TORCH_CHECK(resid->sizes() == x.sizes(), "resid mismatch");
  const void* rp = flat_ptr<const void>(resid, x, x.scalar_type(), exactly(x.numel()), "norm: resid");
  const void* bp = flat_ptr<const void>(b, x, x.scalar_type(), exactly(d), "norm bias");
  const bool need_s = want_s && (has(resid) || p > 0.0);
  auto out = at::empty_like(x);
  Tensor s = need_s ? at::empty_like(x) : Tensor();
  auto f32 = x.options().dtype(at::kFloat);
  auto rstd = at::empty({N}, f32);
  auto mean = kind == 1 ? at::empty({N}, f32) : Tensor();
  if (N > 0)
    check_rc(dllm_norm_fwd(xp, rp, wp, bp, out.data_ptr(), need_s ? s.data_ptr() : nullptr,
                           kind == 1 ? mean.data_ptr<float>() : nullptr, rstd.data_ptr<float>(), N, d, (float)eps,
                           (float)p, (uint32_t)seed, (int)kind, is_bf16(x), (float)w_offset, stream()),
             "norm_fwd");
  return {out, s, mean, rstd};
}

std::vector<Tensor> norm_bwd(const optional<Tensor>& dout_o, const optional<Tensor>& ds, const Tensor& s,
                             const Tensor& w, const optional<Tensor>& b, const optional<Tensor>& mean,
                             const Tensor& rstd, double p, int64_t seed, int64_t kind, bool want_stream,
                             const optional<Tensor>& dw_acc, const optional<Tensor>& db_acc, bool want_colsum,
                             bool partials_only, double w_offset) {
  const void* sp = dense_rows(s, "s", "s must be contiguous [N, d]");
  const int N = s.size(0), d = s.size(1);
  Tensor dout = has(dout_o) ? dout_o->contiguous() : at::zeros_like(s);
  TORCH_CHECK(dout.sizes() == s.sizes(), "dout mismatch");
  const void* dout_p = flat_ptr<const void>(dout, s, s.scalar_type(), exactly(s.numel()), "norm_bwd: dout");
  Tensor dse;
  const void* dse_p = nullptr;
  if (has(ds)) {
    dse = ds->contiguous();
    TORCH_CHECK(dse.sizes() == s.sizes(), "ds mismatch");
    dse_p = flat_ptr<const void>(dse, s, s.scalar_type(), exactly(s.numel()), "norm_bwd: ds");
  }
  TORCH_CHECK(d % 4 == 0 && d <= 2048, "norm: d must be a multiple of 4 and <= 2048, got ", d);
  const void* wp = flat_ptr<const void>(w, s, s.scalar_type(), exactly(d), "norm weight");
  const float* rstd_p = flat_ptr<const float>(rstd, s, at::kFloat, exactly(N), "norm_bwd: rstd");
  const float* mean_p = nullptr;
  if (kind == 1) {
    TORCH_CHECK(has(mean), "mean required for LayerNorm (fp32 [N])");
    mean_p = flat_ptr<const float>(*mean, s, at::kFloat, exactly(N), "norm_bwd: mean");
  }
  auto dx = at::empty_like(s);
  Tensor dstream = want_stream ? at::empty_like(s) : Tensor();
  const int G = dllm_norm_bwd_grid(N > 0 ? N : 1);
  auto f32 = s.options().dtype(at::kFloat);
  auto dw_part = at::empty({G, d}, f32);
  const bool has_b = has(b);  // the bias itself is not read: its gradient is wanted
  // dw_acc / db_acc: accumulate the parameter gradients in place (d elements, contiguous; the flat gradient buffer:
  // param dtype or fp32, FlatParams grad_dtype)
  // partials_only: no reduction at all — dw / db come back as the fp32 per-block partials [G, d] (deferred windows)
  const bool acc = !partials_only && has(dw_acc);
  void *dw_acc_p = nullptr, *db_acc_p = nullptr;
  if (acc) {
    dw_acc_p = flat_ptr<void>(*dw_acc, s, {s.scalar_type(), at::kFloat}, exactly(d), "norm_bwd: dw_acc");
    if (has_b) {
      TORCH_CHECK(has(db_acc), "db_acc mismatch");
      db_acc_p = flat_ptr<void>(*db_acc, s, dw_acc->scalar_type(), exactly(d), "norm_bwd: db_acc");
    }
  }
  Tensor dw = (acc || partials_only) ? Tensor() : at::zeros({d}, f32);
  Tensor db_part = has_b ? at::empty({G, d}, f32) : Tensor();
  Tensor db = (has_b && !acc && !partials_only) ? at::zeros({d}, f32) : Tensor();
  // column sums of dx (the upstream linear layer's bias gradient) stay per-block partials [G, d]: the consuming bias
  // gradient reduces them (ops/gemm.py, one kernel)
  Tensor dxs_part = want_colsum ? at::empty({G, d}, f32) : Tensor();
  if (N > 0)
    check_rc(dllm_norm_bwd(dout_p, dse_p, sp, wp, mean_p, rstd_p, dx.data_ptr(),
                           want_stream ? dstream.data_ptr() : nullptr, dw_part.data_ptr<float>(),
                           has_b ? db_part.data_ptr<float>() : nullptr, dw.defined() ? dw.data_ptr<float>() : nullptr,
                           db.defined() ? db.data_ptr<float>() : nullptr, dw_acc_p, db_acc_p,
                           want_colsum ? dxs_part.data_ptr<float>() : nullptr, /*dxs=*/nullptr, N, d, (float)p,
                           (uint32_t)seed, (int)kind, is_bf16(s), acc && dw_acc->scalar_type() == at::kFloat,
                           (float)w_offset, stream()),
             "norm_bwd");
  if (partials_only) return {dx, dstream, dw_part, db_part, dxs_part};
  return {dx, dstream, dw, db, dxs_part};
}

// ------------------------------------------------------------------------------------------- activations
Tensor act_fwd(const Tensor& x, int64_t act, bool gated, double p, int64_t seed) {
  const void* xp = dense_rows(x, "act: x", "act: x must be contiguous [N, F]");
  const long N = x.size(0);
  const int F = gated ? x.size(1) / 2 : x.size(1);
  TORCH_CHECK(F % 4 == 0 && (!gated || x.size(1) == 2 * F), "act: F must be a multiple of 4");
  auto y = at::empty({N, F}, x.options());
  if (N > 0) check_rc(dllm_act_fwd(xp, y.data_ptr(), N, F, (int)act, gated, (float)p, (uint32_t)seed, is_bf16(x),
                                   stream()), "act_fwd");
  return y;
}

Tensor act_bwd(const Tensor& dy_, const Tensor& x, int64_t act, bool gated, double p, int64_t seed) {
  const void* xp = dense_rows(x, "act_bwd: x", "act_bwd: x must be contiguous [N, F or 2F]");
  Tensor dy = dy_.contiguous();
  const long N = x.size(0);
  const int F = gated ? x.size(1) / 2 : x.size(1);
  TORCH_CHECK(dy.dim() == 2 && dy.size(0) == N && dy.size(1) == F, "act_bwd: dy shape mismatch");
  const void* dyp = flat_ptr<const void>(dy, x, x.scalar_type(), exactly(N * F), "act_bwd: dy");
  auto dx = at::empty_like(x);
  if (N > 0) check_rc(dllm_act_bwd(dyp, xp, dx.data_ptr(), N, F, (int)act, gated, (float)p, (uint32_t)seed, is_bf16(x),
                                   stream()), "act_bwd");
  return dx;
}

Tensor dropout_fwd(const Tensor& x, double p, int64_t seed) {
  const void* xp = flat_ptr<const void>(x, x, {}, at_least(0), "dropout: x");
  TORCH_CHECK(x.numel() % 4 == 0, "dropout: contiguous, numel % 4 == 0");
  auto y = at::empty_like(x);
  if (x.numel() > 0)
    check_rc(dllm_dropout(xp, y.data_ptr(), x.numel(), (float)p, (uint32_t)seed, is_bf16(x), stream()), "dropout");
  return y;
}

// ------------------------------------------------------------------------------------------- column sums
// out += part.sum(0): fp32 partial column sums [G, d] into a bias gradient (fp32 / bf16 [d])
void colsum_partials_acc(const Tensor& part, Tensor& out) {
  TORCH_CHECK(part.dim() == 2, "colsum_partials_acc: part fp32 [G, d] contiguous, out fp32/bf16 [d] contiguous");
  const float* pp = flat_ptr<const float>(part, part, at::kFloat, at_least(0), "colsum_partials_acc: part");
  void* op = flat_ptr<void>(out, part, {at::kFloat, at::kBFloat16}, exactly(part.size(1)), "colsum_partials_acc: out");
  TORCH_CHECK(part.size(0) < INT_MAX && part.size(1) < INT_MAX, "colsum_partials_acc: too large");
  check_rc(dllm_colsum_partials_acc(pp, op, out.scalar_type() == at::kBFloat16 ? 1 : 0, (int)part.size(0),
                                    (int)part.size(1), stream()),
           "colsum_partials_acc");
}

// out (+)= column sums of x ([T, N] bf16, unit inner stride): bias gradients accumulated in place
void colsum_acc(const Tensor& x, Tensor& out) {
  const auto xr = rows<const void>(x, x, at::kBFloat16, kRows4, "colsum_acc: x");
  const int64_t T = x.size(0), N = x.size(1);
  TORCH_CHECK(N % 2 == 0 && N < (1LL << 31), "colsum_acc: N must be even");
  void* op = flat_ptr<void>(out, x, {at::kBFloat16, at::kFloat}, exactly(N), "colsum_acc: out");
  if (T == 0) return;
  const int R = (int)std::min<int64_t>(T, dllm_colsum_rows());
  auto part = at::empty({(int64_t)R * N}, x.options().dtype(at::kFloat));
  check_rc(dllm_colsum_acc(xr.ptr, xr.ld, T, (int)N, part.data_ptr<float>(), op, out.scalar_type() == at::kBFloat16,
                           stream()),
           "colsum_acc");
}

// out[ids[t]] += dy[t] for every token (sorted ids + their positions), deterministic (csrc/embed.hip)
void embed_bwd(const Tensor& ids_sorted, const Tensor& perm, const Tensor& dy, Tensor& out, int64_t padding_idx) {
  const auto dyr = rows<const void>(dy, dy, at::kBFloat16, kRows16, "embed_bwd: dy");
  const int64_t T = dy.size(0), d = dy.size(1);
  TORCH_CHECK(ids_sorted.dim() == 1 && perm.dim() == 1, "embed_bwd: ids / perm must be contiguous int64 [T]");
  const int64_t* ids_p = flat_ptr<const int64_t>(ids_sorted, dy, at::kLong, exactly(T), "embed_bwd: ids");
  const int64_t* perm_p = flat_ptr<const int64_t>(perm, dy, at::kLong, exactly(T), "embed_bwd: perm");
  TORCH_CHECK(d % 8 == 0 && d <= 2048, "embed_bwd: d must be a multiple of 8 and <= 2048");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == d, "embed_bwd: out must be a contiguous bf16/fp32 [V, d] GPU tensor");
  void* op = flat_ptr<void>(out, dy, {at::kBFloat16, at::kFloat}, at_least(0), "embed_bwd: out");
  if (T == 0) return;
  auto ws = at::empty({(T + 63) / 64 * d}, dy.options().dtype(at::kFloat));
  check_rc(dllm_embed_bwd(ids_p, perm_p, dyr.ptr, dyr.ld, T, (int)d, ws.data_ptr<float>(), op, out.size(0),
                          padding_idx, out.scalar_type() == at::kFloat, stream()),
           "embed_bwd");
}

// ------------------------------------------------------------------------------------------- rotary embedding
// x [B, S, n, H, D] (a strided view, head dim contiguous) rotated in place by the positions' cos / sin rows
// (csrc/rope.hip); sign -1: the backward.  Returns x.
Tensor rope_fwd(Tensor x, const Tensor& pos, const Tensor& cos, const Tensor& sin, double sign) {
  const std::string where = residency_fault(x, x);
  TORCH_CHECK(where.empty(), "rope: x ", where);
  const bool bf = is_bf16(x);
  const int64_t E = bf ? 8 : 4;
  TORCH_CHECK(x.dim() == 5, "rope: x must be [B, S, n, H, D], got ", x.sizes());
  const int64_t B = x.size(0), S = x.size(1), n = x.size(2), H = x.size(3), D = x.size(4);
  TORCH_CHECK(D % (2 * E) == 0, "rope: head dim must be a multiple of ", 2 * E, " (16-B chunks per half), got ", D);
  TORCH_CHECK(x.stride(4) == 1, "rope: head dim must be contiguous");
  for (int i = 0; i < 4; ++i)
    TORCH_CHECK(x.stride(i) % E == 0, "rope: strides must be multiples of ", E, " elements (16-B vector loads)");
  const std::string al = align_fault(x, 16);
  TORCH_CHECK(al.empty(), "rope: x ", al);
  TORCH_CHECK(sign == 1.0 || sign == -1.0, "rope: sign must be 1 or -1");
  TORCH_CHECK((pos.dim() == 1 && pos.size(0) == S) || (pos.dim() == 2 && pos.size(0) == B && pos.size(1) == S),
              "rope: pos must be int32 [S] or [B, S] = [", B, ", ", S, "], got ", pos.sizes());
  const int* pos_p = flat_ptr<const int>(pos, x, at::kInt, exactly(pos.dim() == 1 ? S : B * S), "rope: pos");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == D / 2 && cos.size(0) > 0 && cos.size(0) < INT_MAX &&
                  sin.sizes() == cos.sizes(),
              "rope: cos / sin must be fp32 [max_pos, D / 2]");
  const float* cp = flat_ptr<const float>(cos, x, at::kFloat, exactly(cos.numel(), 16), "rope: cos");
  const float* sp = flat_ptr<const float>(sin, x, at::kFloat, exactly(sin.numel(), 16), "rope: sin");
  TORCH_CHECK(B * S * n * H * (D / 2 / E) < ((int64_t)1 << 38) && B < INT_MAX && S < INT_MAX && H < INT_MAX &&
                  n < INT_MAX, "rope: too large");
  if (x.numel() == 0) return x;
  check_rc(dllm_rope(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), x.stride(3), (int)n, (int)B, (int)S, (int)H,
                     (int)D, pos_p, pos.dim() == 1 ? 0 : S, cp, sp, (int)cos.size(0), (float)sign, bf, stream()),
           "rope_fwd");
  return x;
}

}  // namespace

void bind_rowwise(pybind11::module& m) {
  m.def("rope_fwd", &rope_fwd, py::arg("x"), py::arg("pos"), py::arg("cos"), py::arg("sin"), py::arg("sign") = 1.0,
        "rotary position embedding of the slots of x [B, S, n, H, D], in place (sign -1: the backward)");
  m.def("norm_fwd", &norm_fwd, py::arg("x"), py::arg("resid"), py::arg("w"), py::arg("b"), py::arg("eps"),
        py::arg("p"), py::arg("seed"), py::arg("kind"), py::arg("want_s"), py::arg("w_offset") = 0.0);
  m.def("norm_bwd", &norm_bwd, py::arg("dout"), py::arg("ds"), py::arg("s"), py::arg("w"), py::arg("b"),
        py::arg("mean"), py::arg("rstd"), py::arg("p"), py::arg("seed"), py::arg("kind"), py::arg("want_stream"),
        py::arg("dw_acc") = py::none(), py::arg("db_acc") = py::none(), py::arg("want_colsum") = false,
        py::arg("partials_only") = false, py::arg("w_offset") = 0.0);
  m.def("act_fwd", &act_fwd);
  m.def("act_bwd", &act_bwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("colsum_partials_acc", &colsum_partials_acc, "out += part.sum(0) for fp32 partial column sums [G, d]");
  m.def("colsum_acc", &colsum_acc, "out += x.sum(0) for a token-major bf16 x (bias gradients)");
  m.def("embed_bwd", &embed_bwd);
}

}  // namespace dllm
