// The C-ABI launchers of the kernel library: the ONE declaration of every extern "C" dllm_* entry point.
// Every csrc/*.hip sees it through common.h and every binding file through bind_common.h, so a definition or a call
// that disagrees with it ("conflicting types" / "no matching function") does not compile; the HIP sources are built
// with -Werror=missing-prototypes (tools/build_native.py), so a launcher that is not declared here does not either.
// C linkage carries no types: without this header a swapped pair of ints links cleanly and then reads out of range.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "attn_params.h"
#include "gemm_params.h"

// Every translation unit with dropout (common.h DLLM_SEED_STEP_TU(tu)).  The list declares dllm_set_seed_step_<tu>
// below and drives the binding's set_seed_step (csrc/bind.cpp): a new unit is added here and nowhere else.
#define DLLM_SEED_STEP_TUS(X) X(norm) X(act) X(attn) X(attn_f32) X(attn_hd) X(gemm_fused) X(gemm_w4) X(lora)

extern "C" {

#define DLLM_DECLARE_SEED_STEP(tu) int dllm_set_seed_step_##tu(const uint32_t* p);
DLLM_SEED_STEP_TUS(DLLM_DECLARE_SEED_STEP)
#undef DLLM_DECLARE_SEED_STEP

// ---- csrc/norm.hip
int dllm_norm_fwd(const void* x, const void* resid, const void* w, const void* b, void* out, void* s_out, float* mean,
                  float* rstd, int N, int d, float eps, float p, uint32_t seed, int kind, int is_bf16, float w_offset,
                  hipStream_t st);
int dllm_norm_bwd_grid(int N);
int dllm_norm_bwd(const void* dout, const void* ds_extra, const void* s, const void* w, const float* mean,
                  const float* rstd, void* dx, void* dstream, float* dw_part, float* db_part, float* dw, float* db,
                  void* dw_acc, void* db_acc, float* dxs_part, float* dxs, int N, int d, float p, uint32_t seed,
                  int kind, int is_bf16, int acc_f32, float w_offset, hipStream_t st);
int dllm_colsum_partials_acc(const float* part, void* out, int out_is_bf16, int G, int d, hipStream_t st);

// ---- csrc/act.hip
int dllm_act_fwd(const void* x, void* y, long N, int F, int act, int gated, float p, uint32_t seed, int is_bf16,
                 hipStream_t st);
int dllm_act_bwd(const void* dy, const void* x, void* dx, long N, int F, int act, int gated, float p, uint32_t seed,
                 int is_bf16, hipStream_t st);
int dllm_dropout(const void* x, void* y, long numel, float p, uint32_t seed, int is_bf16, hipStream_t st);

// ---- csrc/colsum.hip, csrc/embed.hip
int dllm_colsum_rows();
int dllm_colsum_acc(const void* x, long ld, long T, int N, float* part, void* out, int out_is_bf16, hipStream_t st);
int dllm_embed_bwd(const int64_t* ids, const int64_t* perm, const void* dy, long ld, long T, int d, float* ws,
                   void* out, long V, long padding_idx, int out_f32, hipStream_t st);

// ---- csrc/ce.hip
// cap: the soft cap c of x' = c tanh(x / c) (0: none), in all four
int dllm_ce_fwd(const void* logits, const int64_t* labels, const float* bias, float* loss, float* lse, long N, int V,
                float eps, long ignore, int is_bf16, float cap, hipStream_t st);
int dllm_ce_bwd(const float* scale, const void* logits, const int64_t* labels, const float* lse, const float* bias,
                void* dlogits, long N, int V, float eps, long ignore, int is_bf16, float cap, hipStream_t st);
int dllm_ce_chunk_fwd(const void* logits, long ld, const int64_t* labels, const float* bias, float* state, float* loss,
                      float* lse, long N, int Vc, int c0, int V, float eps, long ignore, int first, int last, int skip,
                      float cap, hipStream_t st);
int dllm_ce_chunk_bwd(const float* scale, void* logits, long ld, const int64_t* labels, const float* lse,
                      const float* bias, long N, int Vc, int c0, int V, float eps, long ignore, int skip, float cap,
                      hipStream_t st);
int dllm_ce_merge(const float* part, int np, long pstride, const float* xlab, const int64_t* labels, float* loss,
                  float* lse, long N, int V, float eps, long ignore, hipStream_t st);

// ---- csrc/kd.hip
int dllm_kd_fwd(const void* student, const void* teacher, const int64_t* labels, const float* bias_s,
                const float* bias_t, float* ce, float* kl, float* stats, long N, int V, float eps, long ignore, float T,
                int is_bf16, hipStream_t st);
int dllm_kd_bwd(const float* w_ce, const float* w_kl, const void* student, const void* teacher, const int64_t* labels,
                const float* stats, const float* bias_s, const float* bias_t, void* dlogits, long N, int V, float eps,
                long ignore, float T, int is_bf16, hipStream_t st);
int dllm_kd_chunk_fwd(const void* student, long ld_s, const void* teacher, long ld_t, const int64_t* labels,
                      const float* bias_s, const float* bias_t, float* state, float* ce, float* kl, float* stats, long N,
                      int Vc, int c0, int V, float eps, long ignore, float T, int first, int last, int skip,
                      hipStream_t st);
int dllm_kd_chunk_bwd(const float* w_ce, const float* w_kl, void* student, long ld_s, const void* teacher, long ld_t,
                      const int64_t* labels, const float* stats, const float* bias_s, const float* bias_t, long N,
                      int Vc, int c0, int V, float eps, long ignore, float T, int skip, hipStream_t st);

// ---- csrc/pref.hip
int dllm_pref_fwd(const void* policy, const void* ref, const int64_t* labels, const float* bias_p, const float* bias_r,
                  float* lp_pi, float* lp_ref, float* lse_pi, long N, int V, long ignore, int is_bf16, hipStream_t st);
int dllm_pref_pair_cols();
int dllm_pref_out_cols();
int dllm_pref_pairs(const float* lp_pi, const float* lp_ref, const int64_t* labels, const float* G,
                    const float* inv_pairs, float* seq_sum, float* pair_out, float* out, float* coef, long P, int T,
                    int V, long ignore, double beta, int kind, double eps, double sft_alpha, hipStream_t st);
int dllm_pref_bwd(const float* coef, const void* policy, const int64_t* labels, const float* lse_pi,
                  const float* bias_p, void* dlogits, long N, int V, int is_bf16, hipStream_t st);
int dllm_pref_chunk_fwd(const void* policy, long ld_p, const void* ref, long ld_r, const int64_t* labels,
                        const float* bias_p, const float* bias_r, float* state, float* lp_pi, float* lp_ref,
                        float* lse_pi, long N, int Vc, int c0, int V, long ignore, int first, int last, int skip,
                        hipStream_t st);
int dllm_pref_chunk_bwd(const float* coef, void* policy, long ld_p, const int64_t* labels, const float* lse_pi,
                        const float* bias_p, long N, int Vc, int c0, int skip, hipStream_t st);

// ---- csrc/adamw.hip, csrc/adafactor.hip
int dllm_sq_norm(const void* g, long n, float* part, float* out, int is_bf16, hipStream_t st);
int dllm_adamw(void* param, float* master, const void* grad, float* m, float* v, const uint8_t* wd_mask,
               const float* coef, long n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2,
               int is_bf16, int grad_f32, const float* hyper, hipStream_t st);
int dllm_adafactor_step(void* param, float* master, const float* grad, float* rv, float* cst, const long* tab, int U,
                        long n_tiles, float* scal, float* colpart, float* rowpart, float* tpart, const float* coef,
                        float rel, float b2t, float eps1, float eps2, float clip_thr, float wd, int scale_param,
                        int is_bf16, const float* hyper, hipStream_t st);

// ---- csrc/attn.hip, csrc/attn_f32.hip, csrc/attn_hd.hip
int dllm_attn_fwd(AttnParams* pp, hipStream_t st);
int dllm_attn_bwd(AttnParams* pp, hipStream_t st);
int dllm_attn_dropout_mask(AttnParams* pp, hipStream_t st);
int dllm_attn_f32_fwd(AttnF32Params* pp, hipStream_t st);
int dllm_attn_f32_bwd(AttnF32Params* pp, hipStream_t st);
int dllm_attn_hd_fwd(AttnHdParams* pp, hipStream_t st);
int dllm_attn_hd_bwd(AttnHdParams* pp, hipStream_t st);

// ---- csrc/rope.hip: rotate the `n` listed slots of x [B, S, *, H, D] in place (x_sn: the slot stride; strides in
// elements); pos [B, S] (pos_sb = S) or [S] (pos_sb = 0); cos / sin fp32 [max_pos, D / 2]; sign -1: the backward
int dllm_rope(void* x, long x_sb, long x_ss, long x_sn, long x_sh, int n, int B, int S, int H, int D, const int* pos,
              long pos_sb, const float* cos, const float* sin, int max_pos, float sign, int is_bf16, hipStream_t st);

// ---- csrc/gemm.hip, csrc/gemm_fused.hip, csrc/gemm_w4.hip (variant: GEMM_FUSED_V_*, epi: W4_EPI_*; gemm_params.h)
int dllm_wgrad_reduce(const GemmWgradParams* pp, hipStream_t st);
int dllm_gemm_fused(const GemmFusedParams* pp, int b_kmajor, int variant, hipStream_t st);
int dllm_gemm_w4(const GemmW4Params* pp, int b_kmajor, int persist, int epi, hipStream_t st);

// ---- csrc/beam.hip, csrc/sample.hip
int dllm_beam_topk(const void* logits, long ld, int is_bf16, const float* beam_scores, const int64_t* seqs, long lds,
                   int cur, int ngram, int ban_tok, int force_tok, int B, int nb, int V, int k_out, float* top_s,
                   int64_t* top_i, hipStream_t st);
int dllm_beam_topk_max_vocab();
int dllm_kv_reorder(void* cache, const int64_t* src, int lk, int rows, int nb, int max_len, int hd, int n,
                    hipStream_t st);
int dllm_sample_list_cap();
int dllm_sample_step(const void* logits, long ld, int is_bf16, const int64_t* seqs, long lds, int cur, int ngram,
                     int ban_tok, int force_tok, int rows, int V, float penalty, float temperature, int top_k,
                     float top_p, uint32_t seed, uint32_t step, int64_t* tok, float* thr, float* list_v, int* list_i,
                     hipStream_t st);

// ---- csrc/lora.hip
int dllm_lora_wgrad_rows();
int dllm_lora_wgrad_max_splits();
int dllm_lora_wgrad_split_rows(long N);
int dllm_lora_down(const void* x, long ldx, const void* A, void* t, int N, int K, int r, float alpha, float p,
                   uint32_t seed, uint32_t row0, hipStream_t st);
int dllm_lora_up(const void* t, int r, const void* M, int kmajor, void* y, long ld, int c0, int n, int N, float alpha,
                 float p, uint32_t seed, uint32_t row0, hipStream_t st);
int dllm_lora_wgrad(const void* Wd, long ldw, int wc, const void* S, int r, float* part, int N, int rows_per_split,
                    int wide_major, void* G, int g_bf16, float alpha, int beta, float p, uint32_t seed, uint32_t row0,
                    hipStream_t st);
}
