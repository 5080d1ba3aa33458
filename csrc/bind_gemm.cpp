// GEMMs: weight gradient and LM-head cross entropy on csrc/gemm_w4.hip (+ csrc/gemm.hip's split-K reduce), the
// fused-epilogue and gated-GELU GEMMs of csrc/gemm_fused.hip, the one-wave-per-SIMD projection GEMM of csrc/gemm_w4.hip.
// Operands are bf16 matrices with 16-B aligned rows (kRows16); what one kernel needs on top is said where it is used.
#include "bind_common.h"

namespace dllm {
namespace {

// The operands a *_supported predicate checked, as the kernels take them.  The predicates judge every tensor on its
// own (a GPU tensor); that the operands share a device is the op's own check ("device mismatch"), as before.
struct Operands {
  Rows<const uint16_t> a, b;
  Rows<void> c;  // the weight gradient's output
};
bool ok16(const Tensor& t, const Mat& m, Rows<const uint16_t>& out) {
  return try_rows(t, t, at::kBFloat16, m, out);
}
Rows<const uint16_t> in16(const Tensor& t, const Tensor& first, const Mat& m, const char* op, const char* name) {
  return rows<const uint16_t>(t, first, at::kBFloat16, m, op, ": ", name);
}
constexpr Rows<uint16_t> kNoC{nullptr, 0};

// ------------------------------------------------------------------------------------------- weight gradient
// c[M][N] (+)= a^T b with a = [K][M], b = [K][N] (token-major), bf16; returns the split count used.
bool wgrad_operands(const Tensor& a, const Tensor& b, const Tensor& c, Operands& o) {
  if (!ok16(a, kRows16, o.a) || !ok16(b, kRows16, o.b) ||
      !try_rows(c, c, {at::kBFloat16, at::kFloat}, kRows16, o.c))
    return false;
  const int64_t K = a.size(0), M = a.size(1), N = b.size(1);
  return b.size(0) == K && c.size(0) == M && c.size(1) == N && K % 64 == 0 && K > 0 && M % 8 == 0 && M >= 8 &&
         N % 256 == 0 &&
         K < (1LL << 31) && M * N < (1LL << 31);
}

bool gemm_wgrad_supported(const Tensor& a, const Tensor& b, const Tensor& c) {
  Operands o;
  return wgrad_operands(a, b, c, o);
}

// K split count of the weight-gradient GEMM.  One 128-KB-LDS workgroup per CU, all workgroups equally long, so the
// kernel runs ceil(T s / CUs) rounds of 1/s of a tile's K each: minimise that (the tail of the last round) plus the
// split-K reduce pass (s fp32 slabs of the output; relative cost ~ 1.7 T s / K at ~1.1 PF/s and ~5 TB/s), fewest
// splits on ties, at least 4 k-stages of 64 per split.  378 tiles (t5 LM head): 2 (3 full rounds instead of 1.48);
// 216 (t5 cross-attention K/V of 12 layers): 13 (11 rounds, 99 % full, instead of one at 84 %);
// 9 / 36 (768 x 768 / 768 x 3072 at 512K tokens): 28 / 7, one round; 27 (QKV): 28, three rounds.
int wgrad_splits(int T, int K) {
  static const int cus = [] {
    const int n = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    return n > 0 ? n : 256;
  }();
  const int smax = std::max(1, std::min(K / 256, 64));
  int best = 1;
  double bestc = 1e30;
  for (int s = 1; s <= smax; ++s) {
    const double rounds = (double)((T * s + cus - 1) / cus);
    const double c = rounds / s + (s > 1 ? 1.7 * T * s / K : 0.0);
    if (c < bestc * (1.0 - 1e-6)) {
      bestc = c;
      best = s;
    }
  }
  return best;
}

// the w4 kernel addresses a split's k-rows through one 32-bit buffer-descriptor range
bool wgrad_chunk_fits(const GemmW4Params& Q, int kchunk) {
  const long ld = std::max(Q.lda, Q.ldb), wd = std::max(Q.M, Q.N);
  return ((long)(kchunk - 1) * ld + wd) * 2 < 0xFFFFFFFFL;
}

// csrc/gemm_w4.hip weight-gradient mode (one wave per SIMD, both operands k-major) into c or, with more than one
// split, into fp32 slabs that csrc/gemm.hip's reduce pass sums into c
void wgrad_launch(GemmW4Params& Q, const Operands& o, const Tensor& c, const Tensor& a, bool beta, const char* what) {
  Q.grp = 8;
  Q.Cw = o.c.ptr;
  Q.c_f32 = c.scalar_type() == at::kFloat ? 1 : 0;
  Q.beta = beta ? 1 : 0;
  Tensor ws;
  if (Q.splits > 1) {
    ws = at::empty({(int64_t)Q.splits * Q.M * Q.N}, a.options().dtype(at::kFloat));
    Q.ws = ws.data_ptr<float>();
  }
  check_rc(dllm_gemm_w4(&Q, 1, 0, W4_EPI_WG, stream()), what);
  if (Q.splits > 1) {
    GemmWgradParams P{};
    P.ws = Q.ws;
    P.C = Q.Cw;
    P.ldc = Q.ldc;
    P.M = Q.M;
    P.N = Q.N;
    P.splits = Q.splits;
    P.beta = Q.beta;
    P.c_f32 = Q.c_f32;
    check_rc(dllm_wgrad_reduce(&P, stream()), "gemm_wgrad split-K reduce");
  }
}

constexpr int64_t kWgradW4 = 12;  // the only gemm_wgrad variant: csrc/gemm_w4.hip's weight-gradient mode

int64_t gemm_wgrad(const Tensor& a, const Tensor& b, Tensor& c, bool beta, int64_t variant, int64_t splits_req) {
  Operands o;
  TORCH_CHECK(wgrad_operands(a, b, c, o),
              "gemm_wgrad: need bf16 GPU [K,M] x [K,N] -> bf16/fp32 [M,N], unit inner stride, 16-B aligned rows, K % 64 == 0, "
              "M % 8 == 0, N a multiple of 256");
  TORCH_CHECK(a.device() == b.device() && a.device() == c.device(), "gemm_wgrad: device mismatch");
  TORCH_CHECK(variant < 0 || variant == kWgradW4, "gemm_wgrad: variant must be -1 (the w4 weight-gradient mode)");
  const int K = a.size(0), M = a.size(1), N = b.size(1);
  GemmW4Params Q{};
  set_gemm(Q, o.a, o.b, Rows<uint16_t>{nullptr, o.c.ld}, M, N, K);  // ragged last M tile (vocab-sized LM-head gradients)
  int splits = splits_req > 0 ? (int)splits_req : wgrad_splits(Q.tm * Q.tn, K);
  splits = std::max(1, std::min(splits, K / 256));
  int kchunk = ((K + splits - 1) / splits + 63) / 64 * 64;
  // more splits when a wide operand (e.g. the decoder's stacked cross-attention K/V gradient, 24576 columns) would
  // overflow the buffer-descriptor range
  while (kchunk > 64 && !wgrad_chunk_fits(Q, kchunk)) {
    ++splits;
    kchunk = ((K + splits - 1) / splits + 63) / 64 * 64;
  }
  TORCH_CHECK(wgrad_chunk_fits(Q, kchunk), "gemm_wgrad: operand rows too long for 64-row splits");
  Q.kchunk = kchunk;
  Q.splits = (K + kchunk - 1) / kchunk;
  wgrad_launch(Q, o, c, a, beta, "gemm_wgrad (w4)");
  return Q.splits;
}

// c[M][N] (+)= sum_i a_i^T b_i over the deferred micro-batches of a gradient-accumulation window (ops/gemm.py
// WgradDefer): equal-shaped token-major segments a_i = [rows][M], b_i = [rows][N] (up to W4_MAX_SEGS), read in place
// by the w4 weight-gradient mode — each segment cut into seg_chunks splits, split-K slabs as gemm_wgrad.  Returns the
// split count.
int64_t gemm_wgrad_segs(const std::vector<Tensor>& as, const std::vector<Tensor>& bs, Tensor& c, bool beta) {
  const int nseg = (int)as.size();
  TORCH_CHECK(nseg >= 1 && nseg <= W4_MAX_SEGS && (int)bs.size() == nseg, "gemm_wgrad_segs: 1..", W4_MAX_SEGS,
              " (a, b) segment pairs");
  GemmW4Params Q{};
  Operands o;
  for (int i = 0; i < nseg; ++i) {
    TORCH_CHECK(wgrad_operands(as[i], bs[i], c, o), "gemm_wgrad_segs: segment ", i, " unsupported");
    TORCH_CHECK(as[i].sizes() == as[0].sizes() && bs[i].sizes() == bs[0].sizes() &&
                    as[i].stride(0) == as[0].stride(0) && bs[i].stride(0) == bs[0].stride(0) &&
                    as[i].device() == c.device() && bs[i].device() == c.device(),
                "gemm_wgrad_segs: segments must share shapes, leading dimensions and device");
    Q.segA[i] = o.a.ptr;
    Q.segB[i] = o.b.ptr;
  }
  const int seg_rows = as[0].size(0), M = as[0].size(1), N = bs[0].size(1);
  set_gemm(Q, Rows<const uint16_t>{nullptr, o.a.ld}, Rows<const uint16_t>{nullptr, o.b.ld},
           Rows<uint16_t>{nullptr, o.c.ld}, M, N, (int64_t)seg_rows * nseg);
  // the split count gemm_wgrad would pick for the window's whole K, spread over the segments
  const int want = wgrad_splits(Q.tm * Q.tn, Q.K);
  int chunks = std::max(1, std::min((want + nseg / 2) / nseg, seg_rows / 64));
  int kchunk = ((seg_rows + chunks - 1) / chunks + 63) / 64 * 64;
  while (kchunk > 64 && !wgrad_chunk_fits(Q, kchunk)) kchunk -= 64;
  TORCH_CHECK(wgrad_chunk_fits(Q, kchunk), "gemm_wgrad_segs: leading dimension too large");
  chunks = (seg_rows + kchunk - 1) / kchunk;
  Q.nseg = nseg;
  Q.seg_rows = seg_rows;
  Q.seg_chunks = chunks;
  Q.kchunk = kchunk;
  Q.splits = nseg * chunks;
  wgrad_launch(Q, o, c, as[0], beta, "gemm_wgrad_segs (w4)");
  return Q.splits;
}

// ------------------------------------------------------------------------------------------- fused epilogues
// c[M][N] = epi(a[M][K] . b) with b = [N][K] (nn.Linear weight, b_kmajor = false) or [K][N] (b_kmajor = true).
// epi: GEMM_FUSED_EPI_* (csrc/gemm_params.h).  Forward activations apply dropout(p, seed) on the output element
// index m * N + n (ops/rng.py); the GELU forwards also write G = dropout'(act'(u)) to aux_out; the backward epilogues
// read aux (saved activation for d-relu, whose dropout backward they apply; G for d-gelu, which they multiply in).
int64_t gemm_fused_variant(int64_t K) {
  // ping-pong kernel (16x16x32 MFMA, BK = 64, two wave rows one barrier apart), persistent for store-only epilogues:
  // fastest on every T5 / BART shape measured (profiles/r1_gemm_*_bench*.jsonl, r1_gemm_experiments.md);
  // K % 64 != 0: BK = 32 x 4 stages
  return K % 64 == 0 ? GEMM_FUSED_V_PP_PERSIST : GEMM_FUSED_V_STAGED;
}

bool is_pp(int v) { return v == GEMM_FUSED_V_PP || v == GEMM_FUSED_V_PP_PERSIST; }

bool fused_operands(const Tensor& a, const Tensor& b, bool b_kmajor, Operands& o) {
  if (!ok16(a, kRows16, o.a) || !ok16(b, kRows16, o.b)) return false;
  const int64_t M = a.size(0), K = a.size(1);
  const int64_t N = b_kmajor ? b.size(1) : b.size(0);
  const int64_t Kb = b_kmajor ? b.size(0) : b.size(1);
  return Kb == K && M % 256 == 0 && N % 256 == 0 && K % 64 == 0 && K > 0 && M > 0 && M * N < (1LL << 32) &&
         K < (1LL << 31);
}

bool gemm_fused_supported(const Tensor& a, const Tensor& b, bool b_kmajor) {
  Operands o;
  return fused_operands(a, b, b_kmajor, o);
}

// the block of a checked (fused_operands) operand pair: everything but C and the epilogue's extras
GemmFusedParams fused_params(const Operands& o, const Tensor& a, const Tensor& b, bool b_kmajor, int epi) {
  GemmFusedParams P{};
  set_gemm(P, o.a, o.b, kNoC, a.size(0), b_kmajor ? b.size(1) : b.size(0), a.size(1));
  P.epi = epi;
  P.scale = 1.f;
  // tile-order group size of the ping-pong kernel (read per call so microbenchmarks can A/B it in one process)
  P.grp = std::max(0, dllm::route_int("gemm_grp", 4));  // 4: +1-3 % over row-major (profiles/r1_gemm_experiments.md)
  return P;
}

Tensor gemm_fused(const Tensor& a, const Tensor& b, bool b_kmajor, int64_t epi, const optional<Tensor>& bias,
                  const optional<Tensor>& aux, const optional<Tensor>& aux_out, double p, int64_t seed,
                  int64_t variant, const optional<Tensor>& mask, const optional<Tensor>& colsum) {
  Operands o;
  TORCH_CHECK(fused_operands(a, b, b_kmajor, o),
              "gemm_fused: need bf16 GPU a [M,K], b [N,K] (or [K,N] k-major), unit inner stride, 16-B aligned rows, "
              "M and N multiples of 256, K % 64 == 0, M*N < 2^32");
  TORCH_CHECK(a.device() == b.device(), "gemm_fused: device mismatch");
  TORCH_CHECK(epi >= GEMM_FUSED_EPI_NONE && epi <= GEMM_FUSED_EPI_DRELU_M, "gemm_fused: bad epilogue ", epi);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "gemm_fused: dropout p must be in [0, 1)");
  GemmFusedParams P = fused_params(o, a, b, b_kmajor, (int)epi);
  const int64_t M = P.M, N = P.N, K = P.K;
  auto out = at::empty({M, N}, a.options());
  P.C = reinterpret_cast<uint16_t*>(out.data_ptr());
  P.ldc = out.stride(0);
  if (has(bias)) {
    TORCH_CHECK(epi <= GEMM_FUSED_EPI_GELU || epi == GEMM_FUSED_EPI_GELU_TANH,
                "gemm_fused: bias only on forward epilogues");
    P.bias = flat_ptr<const uint16_t>(*bias, a, at::kBFloat16, exactly(N, 8), "gemm_fused: bias");
  }
  const bool needs_aux = epi == GEMM_FUSED_EPI_DRELU || epi == GEMM_FUSED_EPI_DGELU || epi == GEMM_FUSED_EPI_DGELU_TANH;
  const bool needs_aux_out = epi == GEMM_FUSED_EPI_GELU || epi == GEMM_FUSED_EPI_GELU_TANH;
  if (needs_aux) {
    TORCH_CHECK(has(aux), "gemm_fused: epilogue ", epi, " needs aux");
    const auto x = in16(*aux, a, kRows8.shape(M, N), "gemm_fused", "aux");
    P.aux = x.ptr;
    P.ldaux = x.ld;
  }
  if (needs_aux_out) {
    TORCH_CHECK(has(aux_out), "gemm_fused: epilogue ", epi, " needs aux_out");
    const auto x = rows<uint16_t>(*aux_out, a, at::kBFloat16, kRows8.shape(M, N), "gemm_fused: aux_out");
    P.aux_out = x.ptr;
    P.ldaux = x.ld;
  }
  set_dropout(P, p, seed);
  const int v = variant >= 0 ? (int)variant : (int)gemm_fused_variant(K);
  TORCH_CHECK(v == GEMM_FUSED_V_STAGED || is_pp(v), "gemm_fused: variant must be 1, 8 or 9, got ", v);
  // ReLU derivative bit mask (ping-pong kernel only): the ReLU forward writes it when given, DRELU_M reads it instead
  // of aux
  TORCH_CHECK(epi != GEMM_FUSED_EPI_DRELU_M || has(mask), "gemm_fused: epilogue 7 needs the ReLU mask");
  if (has(mask)) {
    TORCH_CHECK(epi == GEMM_FUSED_EPI_RELU || epi == GEMM_FUSED_EPI_DRELU_M,
                "gemm_fused: a mask goes with epilogue 1 (write) or 7 (read)");
    TORCH_CHECK(is_pp(v), "gemm_fused: the ReLU mask needs the ping-pong kernel (variant 8 / 9)");
    P.mask = reinterpret_cast<uint32_t*>(
        flat_ptr<int>(*mask, a, at::kInt, exactly(M * N / 32, 16), "gemm_fused: mask (M*N/32 words)"));
  }
  if (has(colsum)) {  // per-128-row column sums of the output (GELU backward: bias grad)
    TORCH_CHECK(epi == GEMM_FUSED_EPI_DGELU || epi == GEMM_FUSED_EPI_DGELU_TANH,
                "gemm_fused: colsum goes with the GELU backward epilogues (4 / 6)");
    TORCH_CHECK(is_pp(v), "gemm_fused: colsum needs the ping-pong kernel (variant 8 / 9)");
    TORCH_CHECK(colsum->dim() == 2 && colsum->size(0) == M / 128 && colsum->size(1) == N,
                "gemm_fused: colsum must be a contiguous fp32 [M / 128, N] GPU tensor");
    P.colsum = flat_ptr<float>(*colsum, a, at::kFloat, exactly(M / 128 * N), "gemm_fused: colsum");
  }
  check_rc(dllm_gemm_fused(&P, b_kmajor ? 1 : 0, v, stream()), "gemm_fused");
  return out;
}

// Gated-GELU FFN (FLAN-T5 / T5 v1.1 "gated-gelu", tanh GELU) on the ping-pong kernel (GEMM_FUSED_EPI_GEGLU / DGEGLU).
// forward: x [M, d] . [wi_0; wi_1]^T ([2F, d], the stacked wi weight) -> h = dropout(gelu(x wi_0^T) * (x wi_1^T)) [M, F]
//          plus G1 = s gelu'(gate) up and G2 = s gelu(gate) ([M, F] each, s = keep / (1 - p)) for the backward;
// backward: dH = dy [M, d] . wo [d, F] (k-major) -> [dH G1 | dH G2] = d(stacked wi output) [M, 2F].
// M % 256 == 0, F % 256 == 0, d % 64 == 0 (the fused FFN's shape rule, ops/ffn.py).
GemmFusedParams geglu_params(const Tensor& a, const Tensor& b, bool b_kmajor, int epi) {
  Operands o;
  TORCH_CHECK(fused_operands(a, b, b_kmajor, o), "gemm_geglu: unsupported operands (bf16 GPU, M / N % 256, K % 64)");
  TORCH_CHECK(a.device() == b.device(), "gemm_geglu: device mismatch");
  return fused_params(o, a, b, b_kmajor, epi);
}

std::vector<Tensor> gemm_geglu(const Tensor& x, const Tensor& wi, double p, int64_t seed) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "gemm_geglu: dropout p must be in [0, 1)");
  GemmFusedParams P = geglu_params(x, wi, false, GEMM_FUSED_EPI_GEGLU);
  const int64_t M = P.M, F = P.N / 2;
  TORCH_CHECK(F % 256 == 0, "gemm_geglu: d_ff must be a multiple of 256");
  auto h = at::empty({M, F}, x.options());
  auto g1 = at::empty({M, F}, x.options());
  auto g2 = at::empty({M, F}, x.options());
  P.C = reinterpret_cast<uint16_t*>(h.data_ptr());
  P.ldc = F;
  P.aux_out = reinterpret_cast<uint16_t*>(g1.data_ptr());
  P.aux_out2 = reinterpret_cast<uint16_t*>(g2.data_ptr());
  P.ldaux = F;
  set_dropout(P, p, seed);
  check_rc(dllm_gemm_fused(&P, 0, GEMM_FUSED_V_PP_PERSIST, stream()), "gemm_geglu");
  return {h, g1, g2};
}

Tensor gemm_dgeglu(const Tensor& dy, const Tensor& wo, const Tensor& g1, const Tensor& g2) {
  GemmFusedParams P = geglu_params(dy, wo, true, GEMM_FUSED_EPI_DGEGLU);
  const int64_t M = P.M, F = P.N;
  for (const Tensor* t : {&g1, &g2})
    TORCH_CHECK(t->dim() == 2 && t->size(0) == M && t->size(1) == F,
                "gemm_dgeglu: G1 / G2 must be contiguous bf16 [M, F] GPU tensors");
  auto du = at::empty({M, 2 * F}, dy.options());
  P.C = reinterpret_cast<uint16_t*>(du.data_ptr());
  P.ldc = 2 * F;
  P.aux = flat_ptr<const uint16_t>(g1, dy, at::kBFloat16, exactly(M * F), "gemm_dgeglu: G1");
  P.aux2 = flat_ptr<const uint16_t>(g2, dy, at::kBFloat16, exactly(M * F), "gemm_dgeglu: G2");
  P.ldaux = F;
  check_rc(dllm_gemm_fused(&P, 1, GEMM_FUSED_V_PP_PERSIST, stream()), "gemm_dgeglu");
  return du;
}

// ------------------------------------------------------------------------------------------- gemm_w4
// One-wave-per-SIMD projection GEMM (csrc/gemm_w4.hip): out (+)= a . b (+ bias), b = [N][K] (nn.Linear weight) or
// [K][N] (b_kmajor, the input-gradient GEMM).  Ragged M / N; K % 64 == 0; N % 8 == 0.  Its buffer-descriptor offsets
// are 32-bit with 0x80000000 as the out-of-range marker: rows do not overlap (dense) and every per-tile byte range
// (256 rows; K rows of a k-major b) is < 2^31.
const Mat kW4Tile = kRows16.dense().range(256);
const Mat kW4Out = kRows16.range(256);

Mat w4_b(bool b_kmajor, int64_t K) { return b_kmajor ? kRows16.dense().range(K) : kW4Tile; }

bool w4_operands(const Tensor& a, const Tensor& b, bool b_kmajor, Operands& o) {
  if (!ok16(a, kW4Tile, o.a)) return false;
  const int64_t M = a.size(0), K = a.size(1);
  if (!ok16(b, w4_b(b_kmajor, K), o.b)) return false;
  const int64_t N = b_kmajor ? b.size(1) : b.size(0);
  const int64_t Kb = b_kmajor ? b.size(0) : b.size(1);
  return Kb == K && K > 0 && K % 64 == 0 && M > 0 && N > 0 && N % 8 == 0 && (M + 255) / 256 * ((N + 255) / 256) < INT_MAX;
}

bool gemm_w4_supported(const Tensor& a, const Tensor& b, bool b_kmajor) {
  Operands o;
  return w4_operands(a, b, b_kmajor, o);
}

// epi 0: plain; 1: ReLU + dropout(p, seed) writing the keep-and-positive bit mask (NT); 7: input gradient through
// that mask (NN).  mask: int32 tensor of >= ceil(M/256) * ceil(N/256) * 2048 words (gemm_w4_mask_words).
Tensor gemm_w4(const Tensor& a, const Tensor& b, bool b_kmajor, const optional<Tensor>& bias, const optional<Tensor>& out,
               bool accumulate, int64_t grp, bool persist, int64_t epi, double p, int64_t seed,
               const optional<Tensor>& mask, bool mask_pp, const optional<Tensor>& aux,
               const optional<Tensor>& aux_out, const optional<Tensor>& colsum) {
  Operands o;
  TORCH_CHECK(w4_operands(a, b, b_kmajor, o),
              "gemm_w4: need bf16 GPU a [M,K], b [N,K] (or [K,N] k-major), unit inner stride, 16-B aligned rows, K % 64 == 0, "
              "N % 8 == 0");
  TORCH_CHECK(a.device() == b.device(), "gemm_w4: device mismatch");
  const int64_t M = a.size(0), K = a.size(1), N = b_kmajor ? b.size(1) : b.size(0);
  Tensor c;
  Rows<uint16_t> cr;
  if (has(out)) {
    c = *out;
    cr = rows<uint16_t>(c, a, at::kBFloat16, kW4Out.shape(M, N), "gemm_w4: out (bf16 [M, N], 16-B aligned rows)");
  } else {
    TORCH_CHECK(!accumulate, "gemm_w4: accumulate needs out");
    c = at::empty({M, N}, a.options());
    cr = {reinterpret_cast<uint16_t*>(c.data_ptr()), (long)c.stride(0)};
  }
  GemmW4Params P{};
  set_gemm(P, o.a, o.b, cr, M, N, K);
  P.bias = flat_ptr<const uint16_t>(bias, a, at::kBFloat16, exactly(N, 8), "gemm_w4: bias");
  P.grp = grp >= 0 ? (int)grp : 8;  // tile-group sweep: profiles/r3_gemm_w4_grp_sweep.txt
  P.accumulate = accumulate ? 1 : 0;
  auto dropout = [&] {
    TORCH_CHECK(M * N < (1LL << 32), "gemm_w4: dropout element index must fit 32 bits");
    TORCH_CHECK(p >= 0.0 && p < 1.0, "gemm_w4: dropout p in [0, 1)");
    set_dropout(P, p, seed);
  };
  if (epi == W4_EPI_GELU || epi == W4_EPI_DGELU) {
    // GELU FFN: bf16 [M, N] derivative out (forward) / in (backward), and the backward's fp32 [M / 128, N] dU column
    // partials
    const optional<Tensor>& x = epi == W4_EPI_GELU ? aux_out : aux;
    TORCH_CHECK(has(x), "gemm_w4: GELU epilogues need a bf16 [M, N] aux tensor with 16-B aligned rows");
    const auto xr = rows<uint16_t>(*x, a, at::kBFloat16, kW4Out.shape(M, N), "gemm_w4: GELU epilogues' aux");
    dropout();
    P.ldaux = xr.ld;
    if (epi == W4_EPI_GELU) {
      P.aux_out = xr.ptr;
    } else {
      P.aux = xr.ptr;
      TORCH_CHECK(has(colsum) && M % 128 == 0,
                  "gemm_w4: GELU backward needs an fp32 contiguous [M / 128, N] colsum tensor (M % 128 == 0)");
      P.colsum = flat_ptr<float>(*colsum, a, at::kFloat, exactly((M / 128) * N, 16), "gemm_w4: GELU backward's colsum");
    }
  } else if (epi != W4_EPI_NONE) {
    TORCH_CHECK(has(mask), "gemm_w4: epilogue mask must be a contiguous int32 GPU tensor of >= "
                           "ceil(M/256)*ceil(N/256)*2048 words");
    P.mask = reinterpret_cast<uint32_t*>(flat_ptr<int>(*mask, a, at::kInt, at_least((int64_t)P.tm * P.tn * 2048, 16),
                                                       "gemm_w4: epilogue mask (ceil(M/256)*ceil(N/256)*2048 words)"));
    dropout();
    P.mask_pp = mask_pp ? 1 : 0;
  }
  check_rc(dllm_gemm_w4(&P, b_kmajor ? 1 : 0, persist ? 1 : 0, (int)epi, stream()), "gemm_w4");
  return c;
}

int64_t gemm_w4_mask_words(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256) * 2048; }

// ------------------------------------------------------------------------------------------- LM head + CE
// LM head + cross-entropy on the w4 GEMM's CE epilogues (W4_EPI_CEF / W4_EPI_CEB): h [N, d] . w [n, d]^T
void lmhead_params(GemmW4Params& P, const Tensor& h, const Tensor& w, const Tensor& labels,
                   const optional<Tensor>& cbias, int64_t V) {
  const int64_t M = h.dim() == 2 ? h.size(0) : 0, N = w.dim() == 2 ? w.size(0) : 0;
  const auto hr = in16(h, h, kW4Tile, "lmhead", "h [N, d] (16-B aligned rows)");
  const auto wr = in16(w, h, kW4Tile, "lmhead", "w [n, d] (16-B aligned rows)");
  TORCH_CHECK(h.size(1) == w.size(1) && h.size(1) % 64 == 0 && M > 0 && N > 0,
              "lmhead: d must match and be a multiple of 64");
  TORCH_CHECK((M + 255) / 256 * ((N + 255) / 256) < INT_MAX && M < INT_MAX && N < INT_MAX, "gemm_w4: too large");
  set_gemm(P, hr, wr, kNoC, M, N, h.size(1));
  P.grp = 0;
  P.labels = flat_ptr<const int64_t>(labels, h, at::kLong, exactly(M), "lmhead: labels");
  P.cbias = flat_ptr<const float>(cbias, h, at::kFloat, exactly(V), "lmhead: bias");
}

// forward: loss_rows [N], lse [N] over the whole vocabulary w [V, d]; the logits are never written
std::vector<Tensor> lmhead_ce_fwd(const Tensor& h, const Tensor& w, const Tensor& labels,
                                  const optional<Tensor>& cbias, double eps, int64_t ignore) {
  GemmW4Params P{};
  const int64_t V = w.dim() == 2 ? w.size(0) : 0;
  lmhead_params(P, h, w, labels, cbias, V);
  const int64_t N = P.M;
  const int64_t np = (V + 127) / 128;
  auto f32 = h.options().dtype(at::kFloat);
  auto part = at::empty({N, np, 4}, f32);
  auto xlab = at::zeros({N}, f32);
  auto loss = at::empty({N}, f32);
  auto lse = at::empty({N}, f32);
  P.part = part.data_ptr<float>();
  P.xlab = xlab.data_ptr<float>();
  P.pstride = (int)np;
  P.c0 = 0; P.V = (int)V; P.skip = 0; P.eps = (float)eps; P.ignore = ignore;
  check_rc(dllm_gemm_w4(&P, 0, 1, W4_EPI_CEF, stream()), "lmhead_ce_fwd (gemm_w4 CEF)");
  check_rc(dllm_ce_merge(P.part, (int)np, np, P.xlab, P.labels, loss.data_ptr<float>(), lse.data_ptr<float>(), N,
                         (int)V, (float)eps, ignore, stream()),
           "lmhead_ce_fwd (merge)");
  return {loss, lse};
}

// backward of one vocabulary slice: out = dlogits of columns [c0, c0 + w_slice.size(0)) (bf16 [N, n], n % 8 == 0)
void lmhead_ce_bwd_slice(const Tensor& h, const Tensor& w_slice, const Tensor& labels, const Tensor& lse,
                         const Tensor& gscale, const optional<Tensor>& cbias, Tensor& out, int64_t c0, int64_t V,
                         double eps, int64_t ignore, int64_t skip) {
  GemmW4Params P{};
  lmhead_params(P, h, w_slice, labels, cbias, V);
  const int64_t N = P.M, n = P.N;
  TORCH_CHECK(n % 8 == 0 && c0 >= 0 && c0 + n <= V && skip >= 0 && skip < n, "lmhead_ce_bwd_slice: bad slice");
  const auto cr = rows<uint16_t>(out, h, at::kBFloat16, kW4Out.shape(N, n), "lmhead_ce_bwd_slice: out");
  P.C = cr.ptr;
  P.ldc = cr.ld;
  P.lse = flat_ptr<const float>(lse, h, at::kFloat, exactly(N), "lmhead_ce_bwd_slice: lse");
  P.gscale = flat_ptr<const float>(gscale, h, at::kFloat, scalar(), "lmhead_ce_bwd_slice: gscale");
  P.c0 = (int)c0; P.V = (int)V; P.skip = (int)skip; P.eps = (float)eps; P.ignore = ignore;
  check_rc(dllm_gemm_w4(&P, 0, 1, W4_EPI_CEB, stream()), "lmhead_ce_bwd_slice (gemm_w4 CEB)");
}

}  // namespace

void bind_gemm(pybind11::module& m) {
  m.def("gemm_wgrad_segs", &gemm_wgrad_segs, "c (+)= sum_i a_i^T b_i (deferred micro-batch segments, w4)",
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("beta") = true);
  m.def("gemm_wgrad", &gemm_wgrad, "c (+)= a^T b (token-major bf16 operands)", py::arg("a"), py::arg("b"), py::arg("c"),
        py::arg("beta") = true, py::arg("variant") = 0, py::arg("splits") = 0);
  m.def("gemm_wgrad_supported", &gemm_wgrad_supported);
  m.def("gemm_fused", &gemm_fused, "epi(a . b) with a fused bias / activation / dropout (or their backward) epilogue",
        py::arg("a"), py::arg("b"), py::arg("b_kmajor"), py::arg("epi"), py::arg("bias") = py::none(),
        py::arg("aux") = py::none(), py::arg("aux_out") = py::none(), py::arg("p") = 0.0, py::arg("seed") = 0,
        py::arg("variant") = -1, py::arg("mask") = py::none(), py::arg("colsum") = py::none());
  m.def("gemm_fused_supported", &gemm_fused_supported);
  m.def("gemm_geglu", &gemm_geglu, "gated-GELU FFN input GEMM: (h, G1, G2) from x and the stacked [wi_0; wi_1]");
  m.def("gemm_dgeglu", &gemm_dgeglu, "gated-GELU FFN backward GEMM: d(stacked wi output) from dy, wo, G1, G2");
  m.def("gemm_fused_variant", &gemm_fused_variant, "default kernel variant for reduction length K");
  m.def("gemm_w4", &gemm_w4, "out (+)= a . b (+ bias) on the one-wave-per-SIMD GEMM (csrc/gemm_w4.hip)", py::arg("a"),
        py::arg("b"), py::arg("b_kmajor"), py::arg("bias") = py::none(), py::arg("out") = py::none(),
        py::arg("accumulate") = false, py::arg("grp") = -1, py::arg("persist") = true, py::arg("epi") = 0,
        py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("mask") = py::none(), py::arg("mask_pp") = false,
        py::arg("aux") = py::none(), py::arg("aux_out") = py::none(), py::arg("colsum") = py::none());
  m.def("gemm_w4_mask_words", &gemm_w4_mask_words);
  m.def("lmhead_ce_fwd", &lmhead_ce_fwd, "LM-head GEMM + CE forward (gemm_w4 CE epilogue + row merge): (loss_rows, lse)");
  m.def("lmhead_ce_bwd_slice", &lmhead_ce_bwd_slice, "dlogits of one vocabulary slice from the GEMM's CE epilogue");
  m.def("gemm_w4_supported", &gemm_w4_supported);
}

}  // namespace dllm
