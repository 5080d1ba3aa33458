// Loss kernels: cross entropy (csrc/ce.hip), the distillation loss (csrc/kd.hip) and the preference loss
// (csrc/pref.hip), whole-vocabulary and vocabulary-chunked forms.
#include "bind_common.h"

#include <cmath>

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

// softcap (all four): c > 0 caps the logits to c tanh(x / c) inside the kernels' pass; 0: none
std::vector<Tensor> ce_fwd(const Tensor& logits, const Tensor& labels, const optional<Tensor>& bias, double eps,
                           int64_t ignore, double softcap) {
  TORCH_CHECK(softcap >= 0.0 && std::isfinite(softcap), "ce: softcap must be finite and >= 0, got ", softcap);
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
                         is_bf16(logits), (float)softcap, stream()),
             "ce_fwd");
  return {loss, lse};
}

Tensor ce_bwd(const Tensor& scale, Tensor logits, const Tensor& labels, const Tensor& lse,
              const optional<Tensor>& bias, double eps, int64_t ignore, bool inplace, double softcap) {
  TORCH_CHECK(softcap >= 0.0 && std::isfinite(softcap), "ce: softcap must be finite and >= 0, got ", softcap);
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
                         is_bf16(logits), (float)softcap, stream()),
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
                  Tensor& lse, int64_t c0, int64_t V, double eps, int64_t ignore, bool first, bool last, int64_t skip,
                  double softcap) {
  TORCH_CHECK(softcap >= 0.0 && std::isfinite(softcap), "ce_chunk: softcap must be finite and >= 0, got ", softcap);
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
                             (float)eps, ignore, first, last, (int)skip, (float)softcap, stream()),
           "ce_chunk_fwd");
}

void ce_chunk_bwd(const Tensor& scale, Tensor& logits, const Tensor& labels, const Tensor& lse,
                  const optional<Tensor>& bias, int64_t c0, int64_t V, double eps, int64_t ignore, int64_t skip,
                  double softcap) {
  TORCH_CHECK(softcap >= 0.0 && std::isfinite(softcap), "ce_chunk_bwd: softcap must be finite and >= 0, got ", softcap);
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
                             ignore, (int)skip, (float)softcap, stream()),
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

// ------------------------------------------------------------------------------------------- preference loss
// csrc/pref.hip: per-row log-probabilities of a policy's and a frozen reference's logits in one pass, the pairwise
// loss over the 2P interleaved sequences, and the gradient over the policy logits.
struct PrefIn {
  void* policy;
  const void* ref;  // nullptr: the policy alone
  const int64_t* labels;
};
PrefIn pref_in(const Tensor& policy, const optional<Tensor>& ref, const Tensor& labels) {
  PrefIn r;
  r.policy = flat_ptr<void>(policy, policy, kLogitDtypes, at_least(0), "pref: policy");
  TORCH_CHECK(policy.dim() == 2, "pref: policy must be contiguous [N, V]");
  TORCH_CHECK(policy.size(1) > 0 && policy.size(1) <= INT_MAX, "pref: policy V out of range");
  r.ref = nullptr;
  if (has(ref)) {
    TORCH_CHECK(ref->dim() == 2 && ref->size(0) == policy.size(0) && ref->size(1) == policy.size(1),
                "pref: reference must have the policy's shape [N, V]");
    r.ref = flat_ptr<const void>(*ref, policy, policy.scalar_type(), exactly(policy.numel()), "pref: reference");
  }
  r.labels = flat_ptr<const int64_t>(labels, policy, at::kLong, exactly(policy.size(0)), "pref: labels");
  return r;
}

std::vector<Tensor> pref_fwd(const Tensor& policy, const optional<Tensor>& ref, const Tensor& labels,
                             const optional<Tensor>& bias_p, const optional<Tensor>& bias_r, int64_t ignore) {
  const PrefIn in = pref_in(policy, ref, labels);
  const long N = policy.size(0);
  const int V = policy.size(1);
  Tensor bp, br;
  const float* bp_p = f32_bias(bias_p, policy, V, bp, "pref: bias");
  const float* br_p = f32_bias(bias_r, policy, V, br, "pref: ref_bias");
  TORCH_CHECK(in.ref != nullptr || br_p == nullptr, "pref: ref_bias without a reference");
  auto f32 = policy.options().dtype(at::kFloat);
  auto lp_pi = at::empty({N}, f32), lp_ref = at::empty({N}, f32), lse = at::empty({N}, f32);
  if (N > 0)
    check_rc(dllm_pref_fwd(in.policy, in.ref, in.labels, bp_p, br_p, lp_pi.data_ptr<float>(),
                           lp_ref.data_ptr<float>(), lse.data_ptr<float>(), N, V, ignore, is_bf16(policy), stream()),
             "pref_fwd");
  return {lp_pi, lp_ref, lse};
}

// (out [7] = {loss, rewards/chosen, rewards/rejected, rewards/margins, rewards/accuracies, logps/chosen,
// logps/rejected}, pair_out [P, 8] = {loss, h, reward_c, reward_r, L_c, L_r, n_c, n_r}, coef [N]).  G: the upstream
// scalar (none: 1); inv_pairs: 1 / P_step.  kind: 0 sigmoid, 1 hinge, 2 ipo.
std::vector<Tensor> pref_pairs(const Tensor& lp_pi, const Tensor& lp_ref, const Tensor& labels,
                               const optional<Tensor>& G, const Tensor& inv_pairs, int64_t T, int64_t V,
                               int64_t ignore, double beta, int64_t kind, double eps, double sft_alpha) {
  const int64_t N = lp_pi.numel();
  TORCH_CHECK(T > 0 && T <= INT_MAX && N > 0 && N % (2 * T) == 0, "pref_pairs: N = ", N,
              " rows are not 2 P T interleaved (chosen, rejected) sequences of T = ", T);
  TORCH_CHECK(V > 0 && V <= INT_MAX, "pref_pairs: V out of range");
  TORCH_CHECK(beta > 0.0, "pref_pairs: beta must be > 0");
  TORCH_CHECK(eps >= 0.0 && eps < 0.5, "pref_pairs: label smoothing must lie in [0, 0.5)");
  TORCH_CHECK(kind >= 0 && kind <= 2, "pref_pairs: kind must be 0 (sigmoid), 1 (hinge) or 2 (ipo)");
  const int64_t P = N / (2 * T);
  const float* lp_p = flat_ptr<const float>(lp_pi, lp_pi, at::kFloat, exactly(N), "pref_pairs: lp_pi");
  const float* lr_p = flat_ptr<const float>(lp_ref, lp_pi, at::kFloat, exactly(N), "pref_pairs: lp_ref");
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, lp_pi, at::kLong, exactly(N), "pref_pairs: labels");
  const float* g_p = has(G) ? flat_ptr<const float>(*G, lp_pi, at::kFloat, scalar(), "pref_pairs: G") : nullptr;
  const float* ip_p = flat_ptr<const float>(inv_pairs, lp_pi, at::kFloat, scalar(), "pref_pairs: inv_pairs");
  auto f32 = lp_pi.options().dtype(at::kFloat);
  auto seq = at::empty({2 * P, 3}, f32), pair_out = at::empty({P, dllm_pref_pair_cols()}, f32);
  auto out = at::empty({dllm_pref_out_cols()}, f32), coef = at::empty({N}, f32);
  check_rc(dllm_pref_pairs(lp_p, lr_p, labels_p, g_p, ip_p, seq.data_ptr<float>(), pair_out.data_ptr<float>(),
                           out.data_ptr<float>(), coef.data_ptr<float>(), P, (int)T, (int)V, ignore, beta, (int)kind,
                           eps, sft_alpha, stream()),
           "pref_pairs");
  return {out, pair_out, coef};
}

Tensor pref_bwd(const Tensor& coef, Tensor policy, const Tensor& labels, const Tensor& lse,
                const optional<Tensor>& bias_p, bool inplace) {
  const PrefIn in = pref_in(policy, {}, labels);
  const long N = policy.size(0);
  const int V = policy.size(1);
  const float* coef_p = flat_ptr<const float>(coef, policy, at::kFloat, exactly(N), "pref: coef");
  const float* lse_p = flat_ptr<const float>(lse, policy, at::kFloat, exactly(N), "pref: lse");
  Tensor bp;
  const float* bp_p = f32_bias(bias_p, policy, V, bp, "pref: bias");
  Tensor out = inplace ? policy : at::empty_like(policy);
  if (N > 0)
    check_rc(dllm_pref_bwd(coef_p, in.policy, in.labels, lse_p, bp_p, inplace ? in.policy : out.data_ptr(), N, V,
                           is_bf16(policy), stream()),
             "pref_bwd");
  return out;
}

// the [N, Vc] bf16 chunks of the vocabulary-chunked form: same conventions as ce_chunk_* / kd_chunk_*
void pref_chunk_fwd(const Tensor& policy, const Tensor& ref, const Tensor& labels, const optional<Tensor>& bias_p,
                    const optional<Tensor>& bias_r, Tensor& state, Tensor& lp_pi, Tensor& lp_ref, Tensor& lse,
                    int64_t c0, int64_t V, int64_t ignore, bool first, bool last, int64_t skip) {
  const auto pl = chunk_logits(policy, "pref_chunk: policy");
  const int64_t N = policy.size(0), Vc = policy.size(1);
  const auto rf = rows<const void>(ref, policy, at::kBFloat16, kRows8.shape(N, Vc), "pref_chunk: reference");
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, policy, at::kLong, exactly(N), "pref_chunk: labels");
  TORCH_CHECK(V > 0 && V <= INT_MAX && c0 >= 0 && c0 + Vc <= V, "pref_chunk: chunk outside the vocabulary");
  TORCH_CHECK(skip >= 0 && skip < std::max<int64_t>(Vc, 1), "pref_chunk: skip out of range");
  const float* bp_p = flat_ptr<const float>(bias_p, policy, at::kFloat, exactly(V), "pref_chunk: bias");
  const float* br_p = flat_ptr<const float>(bias_r, policy, at::kFloat, exactly(V), "pref_chunk: ref_bias");
  float* state_p = flat_ptr<float>(state, policy, at::kFloat, exactly(6 * N), "pref_chunk: state");
  float* lp_p = flat_ptr<float>(lp_pi, policy, at::kFloat, exactly(N), "pref_chunk: lp_pi");
  float* lr_p = flat_ptr<float>(lp_ref, policy, at::kFloat, exactly(N), "pref_chunk: lp_ref");
  float* lse_p = flat_ptr<float>(lse, policy, at::kFloat, exactly(N), "pref_chunk: lse");
  if (N == 0) return;
  check_rc(dllm_pref_chunk_fwd(pl.ptr, pl.ld, rf.ptr, rf.ld, labels_p, bp_p, br_p, state_p, lp_p, lr_p, lse_p, N,
                               (int)Vc, (int)c0, (int)V, ignore, first, last, (int)skip, stream()),
           "pref_chunk_fwd");
}

void pref_chunk_bwd(const Tensor& coef, Tensor& policy, const Tensor& labels, const Tensor& lse,
                    const optional<Tensor>& bias_p, int64_t c0, int64_t V, int64_t skip) {
  const auto pl = chunk_logits(policy, "pref_chunk_bwd: policy");
  const int64_t N = policy.size(0), Vc = policy.size(1);
  const float* coef_p = flat_ptr<const float>(coef, policy, at::kFloat, exactly(N), "pref_chunk_bwd: coef");
  const int64_t* labels_p = flat_ptr<const int64_t>(labels, policy, at::kLong, exactly(N), "pref_chunk_bwd: labels");
  const float* lse_p = flat_ptr<const float>(lse, policy, at::kFloat, exactly(N), "pref_chunk_bwd: lse");
  TORCH_CHECK(V > 0 && V <= INT_MAX && c0 >= 0 && c0 + Vc <= V, "pref_chunk_bwd: chunk outside the vocabulary");
  TORCH_CHECK(skip >= 0 && skip < std::max<int64_t>(Vc, 1), "pref_chunk_bwd: skip out of range");
  const float* bp_p = flat_ptr<const float>(bias_p, policy, at::kFloat, exactly(V), "pref_chunk_bwd: bias");
  if (N == 0) return;
  check_rc(dllm_pref_chunk_bwd(coef_p, pl.ptr, pl.ld, labels_p, lse_p, bp_p, N, (int)Vc, (int)c0, (int)skip, stream()),
           "pref_chunk_bwd");
}

}  // namespace

void bind_loss(pybind11::module& m) {
  m.def("ce_fwd", &ce_fwd, py::arg("logits"), py::arg("labels"), py::arg("bias"), py::arg("eps"), py::arg("ignore"),
        py::arg("softcap") = 0.0);
  m.def("ce_bwd", &ce_bwd, py::arg("scale"), py::arg("logits"), py::arg("labels"), py::arg("lse"), py::arg("bias"),
        py::arg("eps"), py::arg("ignore"), py::arg("inplace"), py::arg("softcap") = 0.0);
  m.def("ce_chunk_fwd", &ce_chunk_fwd, py::arg("logits"), py::arg("labels"), py::arg("bias"), py::arg("state"),
        py::arg("loss"), py::arg("lse"), py::arg("c0"), py::arg("V"), py::arg("eps"), py::arg("ignore"),
        py::arg("first"), py::arg("last"), py::arg("skip"), py::arg("softcap") = 0.0);
  m.def("ce_chunk_bwd", &ce_chunk_bwd, py::arg("scale"), py::arg("logits"), py::arg("labels"), py::arg("lse"),
        py::arg("bias"), py::arg("c0"), py::arg("V"), py::arg("eps"), py::arg("ignore"), py::arg("skip"),
        py::arg("softcap") = 0.0);
  m.def("kd_fwd", &kd_fwd, "distillation loss forward (CE + KL to the teacher): (ce_rows, kl_rows, stats [N, 3])");
  m.def("kd_bwd", &kd_bwd, "student-logits gradient of the distillation loss, optionally in place");
  m.def("kd_chunk_fwd", &kd_chunk_fwd);
  m.def("kd_chunk_bwd", &kd_chunk_bwd);
  m.def("pref_fwd", &pref_fwd, "per-row log-probabilities of policy and reference logits: (lp_pi, lp_ref, lse_pi)");
  m.def("pref_pairs", &pref_pairs, "pairwise preference loss over 2P sequences: (out [7], pair_out [P, 8], coef [N])");
  m.def("pref_bwd", &pref_bwd, "policy-logits gradient of the preference loss, optionally in place");
  m.def("pref_chunk_fwd", &pref_chunk_fwd);
  m.def("pref_chunk_bwd", &pref_chunk_bwd);
}

}  // namespace dllm
