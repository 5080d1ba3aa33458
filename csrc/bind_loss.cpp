// Loss kernels: cross entropy (csrc/ce.hip) and the distillation loss (csrc/kd.hip), whole-vocabulary and
// vocabulary-chunked forms.
#include "bind_common.h"

namespace dllm {
namespace {

const at::ScalarType kLogitDtypes[] = {at::kBFloat16, at::kFloat};

// fp32 [V] bias (or none) on the logits' device; `keep` holds the converted copy alive
const float* f32_bias(const optional<Tensor>& bias, const Tensor& logits, int64_t V, Tensor& keep, const char* name) {
  if (!has(bias)) return nullptr;
  keep = bias->to(at::kFloat).contiguous();
  return flat_ptr<const float>(keep, logits, at::kFloat, exactly(V), name);
}

// ------------------------------------------------------------------------------------------- cross entropy
// dense [N, V] logits of either dtype (judged by is_bf16 at the launch): the op's first operand
void* ce_logits(const Tensor& logits) {
  void* p = flat_ptr<void>(logits, logits, {}, at_least(0), "ce: logits");
  TORCH_CHECK(logits.dim() == 2, "ce: logits must be contiguous [N, V]");
  return p;
}

std::vector<Tensor> ce_fwd(const Tensor& logits, const Tensor& labels, const optional<Tensor>& bias, double eps,
                           int64_t ignore) {
  const void* lp = ce_logits(logits);
  const long N = logits.size(0);
  const int V = logits.size(1);
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, logits, at::kLong, exactly(N), "ce: labels");
  Tensor bf;
  const float* bp = f32_bias(bias, logits, V, bf, "ce: bias");
  auto f32 = logits.options().dtype(at::kFloat);
  auto loss = at::empty({N}, f32), lse = at::empty({N}, f32);
  if (N > 0)
    check_rc(dllm_ce_fwd(lp, labels_p, bp, loss.data_ptr<float>(), lse.data_ptr<float>(), N, V, (float)eps, ignore,
                         is_bf16(logits), stream()),
             "ce_fwd");
  return {loss, lse};
}

Tensor ce_bwd(const Tensor& scale, Tensor logits, const Tensor& labels, const Tensor& lse,
              const optional<Tensor>& bias, double eps, int64_t ignore, bool inplace) {
  void* lp = ce_logits(logits);
  const float* scale_p = flat_ptr<const float>(scale, logits, at::kFloat, scalar(), "ce: scale");
  const long N = logits.size(0);
  const int V = logits.size(1);
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, logits, at::kLong, exactly(N), "ce: labels");
  const float* lse_p = flat_ptr<const float>(lse, logits, at::kFloat, exactly(N), "ce: lse");
  Tensor bf;
  const float* bp = f32_bias(bias, logits, V, bf, "ce: bias");
  Tensor out = inplace ? logits : at::empty_like(logits);
  if (N > 0)
    check_rc(dllm_ce_bwd(scale_p, lp, labels_p, lse_p, bp, inplace ? lp : out.data_ptr(), N, V, (float)eps, ignore,
                         is_bf16(logits), stream()),
             "ce_bwd");
  return out;
}

// vocab-chunked LM head + CE (ops/lm_head.py): logits chunk [N, Vc] bf16 (row stride ld) holding vocab ids c0..c0+Vc-1
Rows<void> chunk_logits(const Tensor& logits, const char* what) {
  const auto r = rows<void>(logits, logits, at::kBFloat16, kRows8, what);
  TORCH_CHECK(logits.size(1) % 4 == 0, what, " needs a column count that is a multiple of 4");
  return r;
}

void ce_chunk_fwd(const Tensor& logits, const Tensor& labels, const optional<Tensor>& bias, Tensor& state, Tensor& loss,
                  Tensor& lse, int64_t c0, int64_t V, double eps, int64_t ignore, bool first, bool last, int64_t skip) {
  const auto lg = chunk_logits(logits, "ce_chunk: logits");
  const int64_t N = logits.size(0), Vc = logits.size(1);
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, logits, at::kLong, exactly(N), "ce_chunk: labels");
  float* state_p = flat_ptr<float>(state, logits, at::kFloat, exactly(4 * N), "ce_chunk: state");
  const Flat rowwise{N, false, false, 1};  // any layout of N elements, as before
  float* loss_p = flat_ptr<float>(loss, logits, at::kFloat, rowwise, "ce_chunk: loss");
  float* lse_p = flat_ptr<float>(lse, logits, at::kFloat, rowwise, "ce_chunk: lse");
  TORCH_CHECK(c0 >= 0 && c0 + Vc <= V, "ce_chunk: chunk outside the vocabulary");
  const float* bp = flat_ptr<const float>(bias, logits, at::kFloat, exactly(V), "ce_chunk: bias");
  if (N == 0) return;
  check_rc(dllm_ce_chunk_fwd(lg.ptr, lg.ld, labels_p, bp, state_p, loss_p, lse_p, N, (int)Vc, (int)c0, (int)V,
                             (float)eps, ignore, first, last, (int)skip, stream()),
           "ce_chunk_fwd");
}

void ce_chunk_bwd(const Tensor& scale, Tensor& logits, const Tensor& labels, const Tensor& lse,
                  const optional<Tensor>& bias, int64_t c0, int64_t V, double eps, int64_t ignore, int64_t skip) {
  const auto lg = chunk_logits(logits, "ce_chunk_bwd: logits");
  const int64_t N = logits.size(0), Vc = logits.size(1);
  const float* scale_p = flat_ptr<const float>(scale, logits, at::kFloat, scalar(), "ce_chunk_bwd: scale");
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, logits, at::kLong, exactly(N), "ce_chunk_bwd: labels");
  const float* lse_p = flat_ptr<const float>(lse, logits, at::kFloat, exactly(N), "ce_chunk_bwd: lse");
  TORCH_CHECK(c0 >= 0 && c0 + Vc <= V, "ce_chunk_bwd: chunk outside the vocabulary");
  TORCH_CHECK(skip >= 0 && skip < Vc, "ce_chunk_bwd: skip outside [0, Vc)");
  const float* bp = flat_ptr<const float>(bias, logits, at::kFloat, exactly(V), "ce_chunk_bwd: bias");
  if (N == 0) return;
  check_rc(dllm_ce_chunk_bwd(scale_p, lg.ptr, lg.ld, labels_p, lse_p, bp, N, (int)Vc, (int)c0, (int)V, (float)eps,
                             ignore, (int)skip, stream()),
           "ce_chunk_bwd");
}

// ------------------------------------------------------------------------------------------- distillation loss
// csrc/kd.hip: label-smoothed CE + temperature-scaled KL to a teacher's logits, one pass over both [N, V] tensors.
struct KdPair {
  void* student;
  const void* teacher;
  const int64_t* labels;
};
KdPair kd_pair(const Tensor& student, const Tensor& teacher, const Tensor& labels, double T) {
  KdPair r;
  r.student = flat_ptr<void>(student, student, kLogitDtypes, at_least(0), "kd: student");
  TORCH_CHECK(student.dim() == 2, "kd: student must be contiguous [N, V]");
  TORCH_CHECK(teacher.dim() == 2 && teacher.size(0) == student.size(0) && teacher.size(1) == student.size(1),
              "kd: teacher must have the student's shape [N, V]");
  r.teacher = flat_ptr<const void>(teacher, student, student.scalar_type(), exactly(student.numel()), "kd: teacher");
  TORCH_CHECK(student.size(1) > 0 && student.size(1) <= INT_MAX, "kd: student V out of range");
  r.labels = flat_ptr<const int64_t>(labels, student, at::kLong, exactly(student.size(0)), "kd: labels");
  TORCH_CHECK(T > 0.0, "kd: temperature must be > 0");
  return r;
}

std::vector<Tensor> kd_fwd(const Tensor& student, const Tensor& teacher, const Tensor& labels,
                           const optional<Tensor>& bias_s, const optional<Tensor>& bias_t, double eps, int64_t ignore,
                           double T) {
  const KdPair in = kd_pair(student, teacher, labels, T);
  const long N = student.size(0);
  const int V = student.size(1);
  Tensor bs, bt;
  const float* bs_p = f32_bias(bias_s, student, V, bs, "kd: bias_s");
  const float* bt_p = f32_bias(bias_t, student, V, bt, "kd: bias_t");
  auto f32 = student.options().dtype(at::kFloat);
  auto ce = at::empty({N}, f32), kl = at::empty({N}, f32), stats = at::empty({N, 3}, f32);
  if (N > 0)
    check_rc(dllm_kd_fwd(in.student, in.teacher, in.labels, bs_p, bt_p, ce.data_ptr<float>(), kl.data_ptr<float>(),
                         stats.data_ptr<float>(), N, V, (float)eps, ignore, (float)T, is_bf16(student), stream()),
             "kd_fwd");
  return {ce, kl, stats};
}

Tensor kd_bwd(const Tensor& w_ce, const Tensor& w_kl, Tensor student, const Tensor& teacher, const Tensor& labels,
              const Tensor& stats, const optional<Tensor>& bias_s, const optional<Tensor>& bias_t, double eps,
              int64_t ignore, double T, bool inplace) {
  const KdPair in = kd_pair(student, teacher, labels, T);
  const long N = student.size(0);
  const int V = student.size(1);
  const float* w_ce_p = flat_ptr<const float>(w_ce, student, at::kFloat, scalar(), "kd: w_ce");
  const float* w_kl_p = flat_ptr<const float>(w_kl, student, at::kFloat, scalar(), "kd: w_kl");
  const float* stats_p = flat_ptr<const float>(stats, student, at::kFloat, exactly(3 * N), "kd: stats");
  Tensor bs, bt;
  const float* bs_p = f32_bias(bias_s, student, V, bs, "kd: bias_s");
  const float* bt_p = f32_bias(bias_t, student, V, bt, "kd: bias_t");
  Tensor out = inplace ? student : at::empty_like(student);
  if (N > 0)
    check_rc(dllm_kd_bwd(w_ce_p, w_kl_p, in.student, in.teacher, in.labels, stats_p, bs_p, bt_p,
                         inplace ? in.student : out.data_ptr(), N, V, (float)eps, ignore, (float)T, is_bf16(student),
                         stream()),
             "kd_bwd");
  return out;
}

// the [N, Vc] bf16 chunk pair of the vocabulary-chunked form: same conventions as ce_chunk_*
struct KdChunks {
  Rows<void> student;
  Rows<const void> teacher;
  const int64_t* labels;
  float* stats;
  const float *bias_s, *bias_t;
};
KdChunks kd_chunks(const Tensor& student, const Tensor& teacher, const Tensor& labels, const Tensor& stats,
                   const optional<Tensor>& bias_s, const optional<Tensor>& bias_t, int64_t c0, int64_t V, double T,
                   int64_t skip) {
  KdChunks r;
  r.student = chunk_logits(student, "kd_chunk: student");
  const int64_t N = student.size(0), Vc = student.size(1);
  r.teacher = rows<const void>(teacher, student, at::kBFloat16, kRows8.shape(N, Vc), "kd_chunk: teacher");
  r.labels = flat_ptr<const int64_t>(labels, student, at::kLong, exactly(N), "kd_chunk: labels");
  r.stats = flat_ptr<float>(stats, student, at::kFloat, exactly(3 * N), "kd_chunk: stats");
  TORCH_CHECK(V > 0 && V <= INT_MAX && c0 >= 0 && c0 + Vc <= V, "kd_chunk: chunk outside the vocabulary");
  TORCH_CHECK(skip >= 0 && skip < std::max<int64_t>(Vc, 1), "kd_chunk: skip out of range");
  TORCH_CHECK(T > 0.0, "kd_chunk: temperature must be > 0");
  r.bias_s = flat_ptr<const float>(bias_s, student, at::kFloat, exactly(V), "kd_chunk: bias_s");
  r.bias_t = flat_ptr<const float>(bias_t, student, at::kFloat, exactly(V), "kd_chunk: bias_t");
  return r;
}

void kd_chunk_fwd(const Tensor& student, const Tensor& teacher, const Tensor& labels, const optional<Tensor>& bias_s,
                  const optional<Tensor>& bias_t, Tensor& state, Tensor& ce, Tensor& kl, Tensor& stats, int64_t c0,
                  int64_t V, double eps, int64_t ignore, double T, bool first, bool last, int64_t skip) {
  const KdChunks in = kd_chunks(student, teacher, labels, stats, bias_s, bias_t, c0, V, T, skip);
  const int64_t N = student.size(0), Vc = student.size(1);
  float* state_p = flat_ptr<float>(state, student, at::kFloat, exactly(8 * N), "kd_chunk: state");
  float* ce_p = flat_ptr<float>(ce, student, at::kFloat, exactly(N), "kd_chunk: ce");
  float* kl_p = flat_ptr<float>(kl, student, at::kFloat, exactly(N), "kd_chunk: kl");
  if (N == 0) return;
  check_rc(dllm_kd_chunk_fwd(in.student.ptr, in.student.ld, in.teacher.ptr, in.teacher.ld, in.labels, in.bias_s,
                             in.bias_t, state_p, ce_p, kl_p, in.stats, N, (int)Vc, (int)c0, (int)V, (float)eps, ignore,
                             (float)T, first, last, (int)skip, stream()),
           "kd_chunk_fwd");
}

void kd_chunk_bwd(const Tensor& w_ce, const Tensor& w_kl, Tensor& student, const Tensor& teacher, const Tensor& labels,
                  const Tensor& stats, const optional<Tensor>& bias_s, const optional<Tensor>& bias_t, int64_t c0,
                  int64_t V, double eps, int64_t ignore, double T, int64_t skip) {
  const KdChunks in = kd_chunks(student, teacher, labels, stats, bias_s, bias_t, c0, V, T, skip);
  const int64_t N = student.size(0), Vc = student.size(1);
  const float* w_ce_p = flat_ptr<const float>(w_ce, student, at::kFloat, scalar(), "kd_chunk: w_ce");
  const float* w_kl_p = flat_ptr<const float>(w_kl, student, at::kFloat, scalar(), "kd_chunk: w_kl");
  if (N == 0) return;
  check_rc(dllm_kd_chunk_bwd(w_ce_p, w_kl_p, in.student.ptr, in.student.ld, in.teacher.ptr, in.teacher.ld, in.labels,
                             in.stats, in.bias_s, in.bias_t, N, (int)Vc, (int)c0, (int)V, (float)eps, ignore, (float)T,
                             (int)skip, stream()),
           "kd_chunk_bwd");
}

}  // namespace

void bind_loss(pybind11::module& m) {
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_chunk_fwd", &ce_chunk_fwd);
  m.def("ce_chunk_bwd", &ce_chunk_bwd);
  m.def("kd_fwd", &kd_fwd, "distillation loss forward (CE + KL to the teacher): (ce_rows, kl_rows, stats [N, 3])");
  m.def("kd_bwd", &kd_bwd, "student-logits gradient of the distillation loss, optionally in place");
  m.def("kd_chunk_fwd", &kd_chunk_fwd);
  m.def("kd_chunk_bwd", &kd_chunk_bwd);
}

}  // namespace dllm
