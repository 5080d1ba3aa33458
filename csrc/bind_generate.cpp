// Generation: beam search and the KV-cache reorder (csrc/beam.hip), sampling (csrc/sample.hip).
#include "bind_common.h"

namespace dllm {
namespace {

constexpr Mat kAnyRows{1, 1};  // unit inner stride, any row stride: the kernels read element by element

// logits [rows, V] (bf16 / fp32) and the generated prefixes seqs [rows, L >= cur] (int64) of one decoding step
struct StepInputs {
  Rows<const void> logits;
  Rows<const int64_t> seqs;
};
StepInputs step_inputs(const Tensor& logits, const Tensor& seqs, int64_t cur, const char* op) {
  StepInputs r;
  r.logits = rows<const void>(logits, logits, {at::kBFloat16, at::kFloat}, kAnyRows, op, ": logits");
  r.seqs = rows<const int64_t>(seqs, logits, at::kLong, kAnyRows.shape(logits.size(0), -1), op, ": seqs");
  TORCH_CHECK(cur <= seqs.size(1), op, ": seqs must be an int64 [rows, L >= cur] GPU tensor with unit inner stride");
  return r;
}

// One beam-search step (csrc/beam.hip): logits [B * nb, V] (bf16 / fp32, unit inner stride), beam scores [B * nb]
// fp32, generated prefix seqs [B * nb, L] int64 -> (rc, top scores [B, k_out] fp32, flat indices [B, k_out] int64).
// rc -4: arguments the kernel does not take (nothing was launched or written; the caller runs the composite).
std::tuple<int64_t, Tensor, Tensor> beam_topk(const Tensor& logits, const Tensor& beam_scores, const Tensor& seqs,
                                              int64_t cur, int64_t ngram, int64_t ban_tok, int64_t force_tok,
                                              int64_t nb, int64_t k_out) {
  const StepInputs in = step_inputs(logits, seqs, cur, "beam_topk");
  const float* scores_p = flat_ptr<const float>(beam_scores, logits, at::kFloat, exactly(logits.size(0)),
                                                "beam_topk: beam_scores");
  TORCH_CHECK(nb > 0 && logits.size(0) % nb == 0, "beam_topk: rows must be a multiple of nb");
  const int64_t B = logits.size(0) / nb, V = logits.size(1);
  TORCH_CHECK(force_tok < V && ban_tok < V, "beam_topk: token id out of range");
  TORCH_CHECK(k_out > 0, "beam_topk: k_out must be positive");
  auto top_s = at::empty({B, k_out}, beam_scores.options());
  auto top_i = at::empty({B, k_out}, seqs.options());
  if (B == 0) return {0, top_s, top_i};
  if (V >= (1LL << 31) || B >= (1LL << 31) || nb >= (1LL << 31) || k_out >= (1LL << 31)) return {-4, top_s, top_i};
  const int rc = dllm_beam_topk(in.logits.ptr, in.logits.ld, logits.scalar_type() == at::kBFloat16, scores_p,
                                in.seqs.ptr, in.seqs.ld, (int)cur, (int)ngram, (int)ban_tok, (int)force_tok, (int)B,
                                (int)nb, (int)V, (int)k_out, top_s.data_ptr<float>(), top_i.data_ptr<int64_t>(),
                                stream());
  if (rc != -4) check_rc(rc, "beam_topk");
  return {rc, top_s, top_i};
}

// One sampling step (csrc/sample.hip): (rc, token [rows] int64, thresholds [rows, 2] fp32).  rc -4: arguments the
// kernel does not take (the caller runs the composite); thresholds: the top-k one (-inf: off) and the final one — the
// kept set is x >= it and x > -inf on the processed scores (the tests compare it with the composite's).
std::tuple<int64_t, Tensor, Tensor> sample_step(const Tensor& logits, const Tensor& seqs, int64_t cur, int64_t ngram,
                                                int64_t ban_tok, int64_t force_tok, double penalty, double temperature,
                                                int64_t top_k, double top_p, int64_t seed, int64_t step) {
  const StepInputs in = step_inputs(logits, seqs, cur, "sample_step");
  TORCH_CHECK(cur >= 0, "sample_step: seqs must be an int64 [rows, L >= cur] GPU tensor with unit inner stride");
  const int64_t nrows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(force_tok < V && ban_tok < V, "sample_step: token id out of range");
  auto tok = at::empty({nrows}, seqs.options());
  auto thr = at::empty({nrows, 2}, logits.options().dtype(at::kFloat));
  if (nrows == 0) return {0, tok, thr};
  if (V >= (1LL << 30) || nrows >= (1LL << 30) || top_k >= (1LL << 31) || ngram >= (1LL << 30)) return {-4, tok, thr};
  const int64_t cap = dllm_sample_list_cap();
  auto list_v = at::empty({nrows, cap}, thr.options());
  auto list_i = at::empty({nrows, cap}, thr.options().dtype(at::kInt));
  const int rc = dllm_sample_step(in.logits.ptr, in.logits.ld, logits.scalar_type() == at::kBFloat16, in.seqs.ptr,
                                  in.seqs.ld, (int)cur, (int)ngram, (int)ban_tok, (int)force_tok, (int)nrows, (int)V,
                                  (float)penalty, (float)temperature, (int)top_k, (float)top_p, (uint32_t)seed,
                                  (uint32_t)step, tok.data_ptr<int64_t>(), thr.data_ptr<float>(),
                                  list_v.data_ptr<float>(), list_i.data_ptr<int>(), stream());
  if (rc != -4) check_rc(rc, "sample_step");
  return {rc, tok, thr};
}

// In-place beam reorder of a [layers * 2, rows, max_len, hd] bf16 cache's live prefix (csrc/beam.hip kv_reorder).
void kv_reorder(Tensor& cache, const Tensor& src, int64_t nb, int64_t n) {
  void* cache_p = flat_ptr<void>(cache, cache, at::kBFloat16, at_least(0), "kv_reorder: cache");
  TORCH_CHECK(cache.dim() == 4, "kv_reorder: cache must be a contiguous bf16 [layers*2, rows, max_len, hd] GPU tensor");
  const int64_t* src_p = flat_ptr<const int64_t>(src, cache, at::kLong, exactly(cache.size(1)), "kv_reorder: src");
  if (n <= 0) return;
  check_rc(dllm_kv_reorder(cache_p, src_p, (int)cache.size(0), (int)cache.size(1), (int)nb, (int)cache.size(2),
                           (int)cache.size(3), (int)n, stream()),
           "kv_reorder");
}

}  // namespace

void bind_generate(pybind11::module& m) {
  m.def("beam_topk", &beam_topk);
  m.def("beam_topk_max_vocab", []() { return (int64_t)dllm_beam_topk_max_vocab(); });
  m.def("kv_reorder", &kv_reorder);
  m.def("sample_step", &sample_step);
}

}  // namespace dllm
