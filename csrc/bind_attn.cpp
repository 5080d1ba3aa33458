// Attention (csrc/attn.hip, csrc/attn_f32.hip, csrc/attn_hd.hip).
#include "bind_common.h"

#include <cmath>

namespace dllm {
namespace {

// One host path for the three kernel families (csrc/attn_params.h is the contract): csrc/attn.hip (bf16, head dim 64),
// csrc/attn_f32.hip (the same op at the reference's precision: fp32 in, fp32 out, f32 MFMA) and csrc/attn_hd.hip (bf16,
// head dims 32 .. 128 other than 64).  A family is its parameter block, its element type and its two launchers.
template <class P>
struct AttnFamily {
  at::ScalarType dtype;
  const char* takes;  // what a tensor of another dtype is told
  int (*fwd)(P*, hipStream_t);
  int (*bwd)(P*, hipStream_t);
  const char* fwd_name;
  const char* bwd_name;
};
const AttnFamily<AttnParams> kAttn{at::kBFloat16, "attention kernels take bf16", dllm_attn_fwd, dllm_attn_bwd,
                                   "attn_fwd", "attn_bwd"};
const AttnFamily<AttnF32Params> kAttnF32{at::kFloat, "fp32 attention kernels take fp32", dllm_attn_f32_fwd,
                                         dllm_attn_f32_bwd, "attn_f32_fwd", "attn_f32_bwd"};
const AttnFamily<AttnHdParams> kAttnHd{at::kBFloat16, "attn_hd kernels take bf16", dllm_attn_hd_fwd, dllm_attn_hd_bwd,
                                       "attn_hd_fwd", "attn_hd_bwd"};

// the 4-D checker: a [B, S, H, D] view of the family's dtype on q's device, 16-B vectors along the head dim
template <class P>
void check_bshd(const Tensor& t, const Tensor& q, const char* n, int64_t B, int64_t S, int64_t H, int64_t D,
                const AttnFamily<P>& f) {
  const std::string where = residency_fault(t, q);
  TORCH_CHECK(where.empty(), n, " ", where);
  TORCH_CHECK(t.scalar_type() == f.dtype, n, ": ", f.takes);
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == S && t.size(2) == H && t.size(3) == D, n,
              ": expected [B, S, H, ", D, "], got ", t.sizes());
  TORCH_CHECK(t.stride(3) == 1, n, ": head dim must be contiguous");
  const int64_t m = 16 / (int64_t)sizeof(typename P::elem);
  TORCH_CHECK(t.stride(0) % m == 0 && t.stride(1) % m == 0 && t.stride(2) % m == 0, n,
              ": strides must be multiples of ", m, " elements (16-B vector loads)");
  const std::string al = align_fault(t, 16);
  TORCH_CHECK(al.empty(), n, " ", al);
}

// a checked (check_bshd) or binding-allocated [B, S, H, D] view into the block: base pointer + batch / sequence / head strides (elements)
template <class U>
void set_view(const Tensor& t, U*& ptr, long& sb, long& ss, long& sh) {
  ptr = reinterpret_cast<U*>(t.data_ptr());
  sb = t.stride(0); ss = t.stride(1); sh = t.stride(2);
}

// shapes from q / k, the q / k / v views, masks, bias and dropout: everything forward and backward share
template <class P>
void fill_common(P& p, const AttnFamily<P>& f, int64_t D, const Tensor& q, const Tensor& k, const Tensor& v,
                 const optional<Tensor>& kpm, const optional<Tensor>& lut, double scale, bool causal, double drop,
                 int64_t seed) {
  const int64_t B = q.size(0), Sq = q.size(1), H = q.size(2), Sk = k.size(1);
  check_bshd(q, q, "q", B, Sq, H, D, f);
  check_bshd(k, q, "k", B, Sk, H, D, f);
  check_bshd(v, q, "v", B, Sk, H, D, f);
  TORCH_CHECK(Sq > 0 && Sk > 0, "empty attention");
  TORCH_CHECK(drop >= 0.0 && drop < 1.0, "dropout p must be in [0, 1)");
  set_view(q, p.q, p.q_sb, p.q_ss, p.q_sh);
  set_view(k, p.k, p.k_sb, p.k_ss, p.k_sh);
  set_view(v, p.v, p.v_sb, p.v_ss, p.v_sh);
  p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk; p.D = D;
  p.scale = (float)scale;
  p.causal = causal ? 1 : 0;
  p.causal_off = Sk - Sq;
  p.window = -1;  // set_window: csrc/attn_f32.hip and csrc/attn_hd.hip only
  p.q_seg = p.k_seg = p.q_blk = p.k_blk = nullptr;  // set_segments: the same two families only
  p.k_glob = nullptr;  // set_global: the same two families only
  p.k_gblk = nullptr;
  p.kl_ptr = p.kl_idx = p.ql_ptr = p.ql_idx = nullptr;  // set_lists: the same two families only
  p.Hl = 0;
  p.l_nnz = 0;
  p.p_drop = (float)drop;
  p.seed = (uint32_t)seed;
  p.thr = drop > 0.0 ? (uint32_t)std::min(65535.0, drop * 65536.0) : 0u;  // ops/rng.py threshold16
  if (has(kpm))
    TORCH_CHECK(kpm->dim() == 2 && kpm->size(0) == B && kpm->size(1) == Sk,
                "key_padding_mask must be uint8 [B, Sk] contiguous on GPU");
  p.kpm = flat_ptr<const uint8_t>(kpm, q, at::kByte, exactly(B * Sk), "key_padding_mask");
  if (has(lut))
    TORCH_CHECK(lut->dim() == 2 && lut->size(0) == H && lut->size(1) == Sq + Sk - 1,
                "bias_lut must be fp32 [H, Sq + Sk - 1] contiguous on GPU");
  p.lut = flat_ptr<const float>(lut, q, at::kFloat, exactly(H * (Sq + Sk - 1)), "bias_lut");
}

// forward outputs: o like q, lse fp32 [B, H, Sq]
template <class P>
std::vector<Tensor> fill_fwd(P& p, const Tensor& q) {
  Tensor o = at::empty({p.B, p.Sq, p.H, p.D}, q.options());
  Tensor lse = at::empty({p.B, p.H, p.Sq}, q.options().dtype(at::kFloat));
  set_view(o, p.o_out, p.o_sb, p.o_ss, p.o_sh);
  p.lse = lse.data_ptr<float>();
  return {o, lse};
}

// backward inputs (o, dout, lse) and outputs: dq / dk / dv may be caller-provided strided views (e.g. slices of one
// packed d(qkv) buffer), delta is scratch, dlut is zeroed for the kernels' atomics when wanted and there is a bias
struct AttnBwdOut { Tensor dq, dk, dv, delta, dlut; };
template <class P>
AttnBwdOut fill_bwd(P& p, const AttnFamily<P>& f, const Tensor& q, const Tensor& o, const Tensor& dout,
                    const Tensor& lse, const optional<Tensor>& dq_out, const optional<Tensor>& dk_out,
                    const optional<Tensor>& dv_out, bool want_dlut) {
  check_bshd(o, q, "o", p.B, p.Sq, p.H, p.D, f);
  check_bshd(dout, q, "dout", p.B, p.Sq, p.H, p.D, f);
  p.lse = flat_ptr<float>(lse, q, at::kFloat, exactly((int64_t)p.B * p.H * p.Sq), "attention: lse");
  auto pick = [&](const optional<Tensor>& t, int64_t S, const char* n) {
    if (has(t)) {
      check_bshd(*t, q, n, p.B, S, p.H, p.D, f);
      return *t;
    }
    return at::empty({p.B, S, p.H, p.D}, q.options());
  };
  auto f32 = q.options().dtype(at::kFloat);
  AttnBwdOut r{pick(dq_out, p.Sq, "dq_out"), pick(dk_out, p.Sk, "dk_out"), pick(dv_out, p.Sk, "dv_out"),
               at::empty({p.B, p.H, p.Sq}, f32), Tensor()};
  if (want_dlut && p.lut != nullptr) {
    r.dlut = at::zeros({p.H, p.Sq + p.Sk - 1}, f32);
    p.dlut = r.dlut.data_ptr<float>();
  }
  set_view(o, p.o, p.o_sb, p.o_ss, p.o_sh);
  set_view(dout, p.dout, p.do_sb, p.do_ss, p.do_sh);
  p.delta = r.delta.data_ptr<float>();
  set_view(r.dq, p.dq, p.dq_sb, p.dq_ss, p.dq_sh);
  set_view(r.dk, p.dk, p.dk_sb, p.dk_ss, p.dk_sh);
  set_view(r.dv, p.dv, p.dv_sb, p.dv_ss, p.dv_sh);
  return r;
}

// ---- csrc/attn_f32.hip and csrc/attn_hd.hip: a forward and a backward that differ by family and head dim only
// their grids put B * H on the y axis, and they index rows (B * H * Sq) and the LUT (Sq + Sk) with 32 bits
template <class P>
void check_limits_small(const P& p) {
  TORCH_CHECK((int64_t)p.B * p.H <= 65535, "attention: B * H > 65535 unsupported (grid y)");
  TORCH_CHECK((int64_t)p.B * p.H * p.Sq < (int64_t)1 << 31 && ((int64_t)p.Sq + p.Sk) < (1 << 30),
              "attention too large");
}

// the sliding window of csrc/attn_params.h: a band around the diagonal of a square, non-causal problem
template <class P>
void set_window(P& p, int64_t window) {
  if (window < 0) return;
  TORCH_CHECK(p.Sq == p.Sk, "attention: window needs Sq == Sk, got ", p.Sq, " and ", p.Sk);
  TORCH_CHECK(!p.causal, "attention: window with causal is unsupported");
  p.window = (int)std::min<int64_t>(window, INT_MAX);
}

// the segments of csrc/attn_params.h: ids [B, Sq] / [B, Sk] and their per-64-block (min, max) tables, all four or none
template <class P>
void set_segments(P& p, const Tensor& q, const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                  const optional<Tensor>& q_blk, const optional<Tensor>& k_blk) {
  const int n = has(q_seg) + has(k_seg) + has(q_blk) + has(k_blk);
  if (n == 0) return;
  TORCH_CHECK(n == 4, "attention: q_seg, k_seg, q_blk and k_blk are given together or not at all");
  TORCH_CHECK(p.window < 0, "attention: segments with a window are unsupported");
  auto ids = [&](const Tensor& t, const char* name, int64_t S, bool blk) {
    const int64_t n1 = blk ? (S + 63) / 64 : S;
    TORCH_CHECK(t.dim() == (blk ? 3 : 2) && t.size(0) == p.B && t.size(1) == n1 && (!blk || t.size(2) == 2), name,
                ": expected [", p.B, ", ", n1, blk ? ", 2" : "", "], got ", t.sizes());
    return flat_ptr<const int>(t, q, at::kInt, at_least(0), name);
  };
  p.q_seg = ids(*q_seg, "q_seg", p.Sq, false);
  p.k_seg = ids(*k_seg, "k_seg", p.Sk, false);
  p.q_blk = ids(*q_blk, "q_blk", p.Sq, true);
  p.k_blk = ids(*k_blk, "k_blk", p.Sk, true);
}

// the global keys of csrc/attn_params.h: flags [B, Sk] and the per-batch list of the 64-key blocks that hold one, both
// or neither, only with a window
template <class P>
void set_global(P& p, const Tensor& q, const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk) {
  if (!has(k_glob) && !has(k_gblk)) return;
  TORCH_CHECK(has(k_glob) && has(k_gblk), "attention: k_glob and k_gblk are given together or not at all");
  TORCH_CHECK(!p.causal, "attention: global keys with causal are unsupported");
  TORCH_CHECK(p.q_seg == nullptr, "attention: global keys with segments are unsupported");
  TORCH_CHECK(p.window >= 0, "attention: global keys need a window");
  TORCH_CHECK(!(std::is_same<P, AttnHdParams>::value && p.D == 32),
              "attn_hd: global keys at head dim 32 are not served (csrc/attn_hd.hip)");
  const int64_t nb = (p.Sk + 63) / 64;
  TORCH_CHECK(k_glob->dim() == 2 && k_glob->size(0) == p.B && k_glob->size(1) == p.Sk, "k_glob: expected [", p.B, ", ",
              p.Sk, "], got ", k_glob->sizes());
  TORCH_CHECK(k_gblk->dim() == 2 && k_gblk->size(0) == p.B && k_gblk->size(1) == nb + 1, "k_gblk: expected [", p.B,
              ", ", nb + 1, "], got ", k_gblk->sizes());
  p.k_glob = flat_ptr<const uint8_t>(*k_glob, q, at::kByte, at_least(0), "k_glob");
  p.k_gblk = flat_ptr<const int>(*k_gblk, q, at::kInt, at_least(0), "k_gblk");
}

// the block lists of csrc/attn_params.h: the CSR table of key blocks per (head, query block) and its transpose, all
// four or none, with nothing else that shapes the walk
template <class P>
void set_lists(P& p, const Tensor& q, const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
               const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx) {
  const int n = has(kl_ptr) + has(kl_idx) + has(ql_ptr) + has(ql_idx);
  if (n == 0) return;
  TORCH_CHECK(n == 4, "attention: kl_ptr, kl_idx, ql_ptr and ql_idx are given together or not at all");
  TORCH_CHECK(!p.causal, "attention: block lists with causal are unsupported");
  TORCH_CHECK(p.k_glob == nullptr, "attention: block lists with global keys are unsupported");  // (they bring a window)
  TORCH_CHECK(p.window < 0, "attention: block lists with a window are unsupported");
  TORCH_CHECK(p.q_seg == nullptr, "attention: block lists with segments are unsupported");
  TORCH_CHECK(!(std::is_same<P, AttnHdParams>::value && p.D == 32),
              "attn_hd: block lists at head dim 32 are not served (csrc/attn_hd.hip)");
  const int64_t nq = (p.Sq + 63) / 64, nk = (p.Sk + 63) / 64;
  TORCH_CHECK(kl_ptr->dim() == 2 && (kl_ptr->size(0) == p.H || kl_ptr->size(0) == 1) && kl_ptr->size(1) == nq + 1,
              "kl_ptr: expected [H or 1, ", nq + 1, "], got ", kl_ptr->sizes());
  TORCH_CHECK(ql_ptr->dim() == 2 && ql_ptr->size(0) == kl_ptr->size(0) && ql_ptr->size(1) == nk + 1,
              "ql_ptr: expected [", kl_ptr->size(0), ", ", nk + 1, "], got ", ql_ptr->sizes());
  TORCH_CHECK(kl_idx->dim() == 1 && ql_idx->dim() == 1 && kl_idx->numel() == ql_idx->numel() &&
                  kl_idx->numel() < INT_MAX,
              "kl_idx / ql_idx: expected two [nnz] tensors of one length, got ", kl_idx->sizes(), " and ",
              ql_idx->sizes());
  p.Hl = (int)kl_ptr->size(0);
  p.l_nnz = (int)kl_idx->numel();
  p.kl_ptr = flat_ptr<const int>(*kl_ptr, q, at::kInt, at_least(0), "kl_ptr");
  p.ql_ptr = flat_ptr<const int>(*ql_ptr, q, at::kInt, at_least(0), "ql_ptr");
  // an empty index tensor may have no storage: the kernels never read it (row ends are clamped to nnz), any non-null
  // pointer of the device will do
  p.kl_idx = p.l_nnz ? flat_ptr<const int>(*kl_idx, q, at::kInt, at_least(0), "kl_idx") : p.kl_ptr;
  p.ql_idx = p.l_nnz ? flat_ptr<const int>(*ql_idx, q, at::kInt, at_least(0), "ql_idx") : p.ql_ptr;
}

// the soft cap of csrc/attn_params.h: with nothing but kpm, causal, a window and dropout
template <class P>
void set_softcap(P& p, double softcap) {
  p.softcap = 0.f;
  if (softcap == 0.0) return;
  TORCH_CHECK(softcap > 0.0 && std::isfinite(softcap), "attention: softcap must be finite and >= 0, got ", softcap);
  TORCH_CHECK(p.lut == nullptr, "attention: a soft cap with a bias LUT is unsupported");
  TORCH_CHECK(p.q_seg == nullptr, "attention: a soft cap with segments is unsupported");
  TORCH_CHECK(p.k_glob == nullptr, "attention: a soft cap with global keys is unsupported");
  TORCH_CHECK(p.kl_ptr == nullptr, "attention: a soft cap with block lists is unsupported");
  TORCH_CHECK(!(std::is_same<P, AttnHdParams>::value && p.D == 32),
              "attn_hd: a soft cap at head dim 32 is not served (csrc/attn_hd.hip)");
  p.softcap = (float)softcap;
}

template <class P>
std::vector<Tensor> attn_small_fwd(const AttnFamily<P>& f, int64_t D, const Tensor& q, const Tensor& k,
                                   const Tensor& v, const optional<Tensor>& kpm, const optional<Tensor>& lut,
                                   double scale, bool causal, double p, int64_t seed, int64_t window,
                                   const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                   const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                   const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                   const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                   const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  P prm{};
  fill_common(prm, f, D, q, k, v, kpm, lut, scale, causal, p, seed);
  set_window(prm, window);
  set_segments(prm, q, q_seg, k_seg, q_blk, k_blk);
  set_global(prm, q, k_glob, k_gblk);
  set_lists(prm, q, kl_ptr, kl_idx, ql_ptr, ql_idx);
  set_softcap(prm, softcap);
  check_limits_small(prm);
  auto out = fill_fwd(prm, q);
  check_rc(f.fwd(&prm, stream()), f.fwd_name);
  return out;
}

template <class P>
std::vector<Tensor> attn_small_bwd(const AttnFamily<P>& f, int64_t D, const Tensor& dout, const Tensor& q,
                                   const Tensor& k, const Tensor& v, const Tensor& o, const Tensor& lse,
                                   const optional<Tensor>& kpm, const optional<Tensor>& lut, double scale, bool causal,
                                   double p, int64_t seed, bool need_dlut, const optional<Tensor>& dq_out,
                                   const optional<Tensor>& dk_out, const optional<Tensor>& dv_out, int64_t window,
                                   const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                   const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                   const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                   const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                   const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  P prm{};
  fill_common(prm, f, D, q, k, v, kpm, lut, scale, causal, p, seed);
  set_window(prm, window);
  set_segments(prm, q, q_seg, k_seg, q_blk, k_blk);
  set_global(prm, q, k_glob, k_gblk);
  set_lists(prm, q, kl_ptr, kl_idx, ql_ptr, ql_idx);
  set_softcap(prm, softcap);
  check_limits_small(prm);
  auto r = fill_bwd(prm, f, q, o, dout, lse, dq_out, dk_out, dv_out, need_dlut);
  check_rc(f.bwd(&prm, stream()), f.bwd_name);
  return {r.dq, r.dk, r.dv, r.dlut};
}

std::vector<Tensor> attn_f32_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& kpm,
                                 const optional<Tensor>& lut, double scale, bool causal, double p, int64_t seed,
                                 int64_t window,
                                 const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                 const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                 const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                 const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                 const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  return attn_small_fwd(kAttnF32, 64, q, k, v, kpm, lut, scale, causal, p, seed, window, q_seg, k_seg, q_blk,
                        k_blk, k_glob, k_gblk, kl_ptr, kl_idx,
                        ql_ptr, ql_idx, softcap);
}

std::vector<Tensor> attn_f32_bwd(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
                                 const Tensor& o, const Tensor& lse, const optional<Tensor>& kpm,
                                 const optional<Tensor>& lut, double scale, bool causal, double p, int64_t seed,
                                 bool need_dlut, const optional<Tensor>& dq_out, const optional<Tensor>& dk_out,
                                 const optional<Tensor>& dv_out, int64_t window,
                                 const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                 const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                 const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                 const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                 const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  return attn_small_bwd(kAttnF32, 64, dout, q, k, v, o, lse, kpm, lut, scale, causal, p, seed, need_dlut, dq_out,
                        dk_out, dv_out, window, q_seg, k_seg, q_blk, k_blk, k_glob, k_gblk, kl_ptr, kl_idx,
                        ql_ptr, ql_idx, softcap);
}

// the head dim of an attn_hd call: what csrc/attn_hd.hip is instantiated for (padded to 32, 16-B rows)
int64_t attn_hd_dim(const Tensor& q, const Tensor& k) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "attn_hd: q / k / v must be [B, S, H, D]");
  const int64_t D = q.size(3);
  TORCH_CHECK(D >= 32 && D <= 128 && D % 8 == 0, "attn_hd: head dim must be in 32 .. 128 and a multiple of 8, got ", D);
  return D;
}

std::vector<Tensor> attn_hd_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& kpm,
                                const optional<Tensor>& lut, double scale, bool causal, double p, int64_t seed,
                                int64_t window,
                                const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  return attn_small_fwd(kAttnHd, attn_hd_dim(q, k), q, k, v, kpm, lut, scale, causal, p, seed, window, q_seg, k_seg,
                        q_blk, k_blk, k_glob, k_gblk, kl_ptr, kl_idx,
                        ql_ptr, ql_idx, softcap);
}

std::vector<Tensor> attn_hd_bwd(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v,
                                const Tensor& o, const Tensor& lse, const optional<Tensor>& kpm,
                                const optional<Tensor>& lut, double scale, bool causal, double p, int64_t seed,
                                bool need_dlut, const optional<Tensor>& dq_out, const optional<Tensor>& dk_out,
                                const optional<Tensor>& dv_out, int64_t window,
                                const optional<Tensor>& q_seg, const optional<Tensor>& k_seg,
                                const optional<Tensor>& q_blk, const optional<Tensor>& k_blk,
                                const optional<Tensor>& k_glob, const optional<Tensor>& k_gblk,
                                const optional<Tensor>& kl_ptr, const optional<Tensor>& kl_idx,
                                const optional<Tensor>& ql_ptr, const optional<Tensor>& ql_idx, double softcap) {
  return attn_small_bwd(kAttnHd, attn_hd_dim(q, k), dout, q, k, v, o, lse, kpm, lut, scale, causal, p, seed,
                        need_dlut, dq_out, dk_out, dv_out, window, q_seg, k_seg, q_blk, k_blk, k_glob, k_gblk, kl_ptr, kl_idx,
                        ql_ptr, ql_idx, softcap);
}

// ---- csrc/attn.hip: the same helpers, plus its extras (dropout bit planes, saturated-bias ranges, rowrec, column sums)
// its K/V tile rings and key masks live in LDS (sequence length) and its plane / rowrec indices are 64-bit products
void check_limits_attn(const AttnParams& p) {
  TORCH_CHECK(p.Sk <= 16384 && p.Sq <= 16384, "attention: sequence length > 16384 unsupported");
  TORCH_CHECK((int64_t)p.B * p.H * p.Sq * p.Sk < (int64_t)1 << 40, "attention too large");
}

// sat_lo / sat_hi: LUT index ranges [0, sat_lo] and [sat_hi, L) of constant bias whose gradient is consumed per
// bucket only (ops/attention.py relative_bias_lut); negative = off
void set_sat(AttnParams& P, int64_t sat_lo, int64_t sat_hi) {
  P.sat_lo = INT_MIN / 2;
  P.sat_hi = INT_MAX / 2;
  if (P.lut == nullptr || sat_lo < 0 || sat_hi < 0) return;
  const int64_t L = (int64_t)P.Sq + P.Sk - 1;
  TORCH_CHECK(sat_lo < L && sat_hi > sat_lo && sat_hi <= L, "attention: bad saturated-bias bounds");
  P.sat_lo = (int)sat_lo;
  P.sat_hi = (int)sat_hi;
}

int64_t dmask_numel(const AttnParams& P) {
  const int64_t sq_pad = (P.Sq + 127) / 128 * 128, nkt = (P.Sk + 63) / 64;
  return (int64_t)P.B * P.H * nkt * 2 * sq_pad;
}

std::vector<Tensor> attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& kpm,
                             const optional<Tensor>& lut, double scale, bool causal, double p, int64_t seed,
                             int64_t sat_lo, int64_t sat_hi) {
  AttnParams P{};
  fill_common(P, kAttn, 64, q, k, v, kpm, lut, scale, causal, p, seed);
  check_limits_attn(P);
  set_sat(P, sat_lo, sat_hi);
  auto out = fill_fwd(P, q);
  // dropout keep bits: [B*H][ceil(Sk/64)][2][ceil(Sq/128)*128] uint32, written here, read by attn_bwd
  Tensor dmask;
  if (p > 0.0) {
    dmask = at::empty({dmask_numel(P)}, q.options().dtype(at::kInt));
    P.dmask = reinterpret_cast<uint32_t*>(dmask.data_ptr());
  }
  check_rc(kAttn.fwd(&P, stream()), kAttn.fwd_name);
  return {out[0], out[1], dmask};
}

// the dropout keep-bit planes attn_fwd would return for these shapes, p and seed, without running it
Tensor attn_dropout_mask(int64_t B, int64_t H, int64_t Sq, int64_t Sk, double p, int64_t seed, const Tensor& like) {
  TORCH_CHECK(p > 0.0 && B > 0 && H > 0 && Sq > 0 && Sk > 0 && like.is_cuda(), "attn_dropout_mask: bad arguments");
  AttnParams P{};
  P.B = B; P.H = H; P.Sq = Sq; P.Sk = Sk;
  P.p_drop = (float)p;
  P.seed = (uint32_t)seed;
  auto dmask = at::empty({dmask_numel(P)}, like.options().dtype(at::kInt));
  P.dmask = reinterpret_cast<uint32_t*>(dmask.data_ptr());
  check_rc(dllm_attn_dropout_mask(&P, stream()), "attn_dropout_mask");
  return dmask;
}

std::vector<Tensor> attn_bwd(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                             const Tensor& lse, const optional<Tensor>& kpm, const optional<Tensor>& lut,
                             double scale, bool causal, double p, int64_t seed, bool need_dlut,
                             const optional<Tensor>& dq_out, const optional<Tensor>& dk_out,
                             const optional<Tensor>& dv_out, const optional<Tensor>& dmask, int64_t sat_lo,
                             int64_t sat_hi, const optional<Tensor>& csq, const optional<Tensor>& csk,
                             const optional<Tensor>& csv) {
  AttnParams P{};
  fill_common(P, kAttn, 64, q, k, v, kpm, lut, scale, causal, p, seed);
  check_limits_attn(P);
  set_sat(P, sat_lo, sat_hi);
  if (p > 0.0) {
    TORCH_CHECK(has(dmask), "attn_bwd: dropout needs the bit planes attn_fwd returned");
    P.dmask = reinterpret_cast<uint32_t*>(
        flat_ptr<int>(*dmask, q, at::kInt, exactly(dmask_numel(P)), "attn_bwd: dmask (attn_fwd's bit planes)"));
  }
  // the kernels accumulate the LUT gradient whenever there is a bias: always allocated, returned when wanted
  auto r = fill_bwd(P, kAttn, q, o, dout, lse, dq_out, dk_out, dv_out, true);
  // per-row terms the dQ kernel hands to the dK/dV kernel ([B*H][sq_pad/64][4][64])
  Tensor rowrec = at::empty({(int64_t)P.B * P.H * ((P.Sq + 127) / 128 * 128) * 4}, r.delta.options());
  P.rowrec = rowrec.data_ptr<float>();
  // optional per-block column sums ([B * ceil(S / 128)][H * 64] fp32 views, unit column stride; dK / dV share a row
  // stride): the bias gradients of the q / k / v projections, summed over blocks by the caller
  auto cs = [&](const optional<Tensor>& t, int64_t S, const char* n, long* ld) -> float* {
    if (!has(t)) return nullptr;
    const auto m = rows<float>(*t, q, at::kFloat, Mat{1, 1}.shape(P.B * ((S + 127) / 128), (int64_t)P.H * 64).dense(), n,
                               ": expected fp32 [B * ceil(S / 128), H * 64] with unit column stride:");
    *ld = m.ld;
    return m.ptr;
  };
  long ldk = 0, ldv = 0;
  P.csq = cs(csq, P.Sq, "csq", &P.csq_ld);
  P.csk = cs(csk, P.Sk, "csk", &ldk);
  P.csv = cs(csv, P.Sk, "csv", &ldv);
  TORCH_CHECK((P.csk == nullptr) == (P.csv == nullptr) && ldk == ldv, "csk / csv: both or neither, one row stride");
  P.cskv_ld = ldk;
  check_rc(kAttn.bwd(&P, stream()), kAttn.bwd_name);
  return {r.dq, r.dk, r.dv, need_dlut ? r.dlut : Tensor()};
}

}  // namespace

void bind_attn(pybind11::module& m) {
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kpm"), py::arg("lut"),
        py::arg("scale"), py::arg("causal"), py::arg("p"), py::arg("seed"), py::arg("sat_lo") = -1,
        py::arg("sat_hi") = -1);
  m.def("attn_dropout_mask", &attn_dropout_mask);
  m.def("attn_bwd", &attn_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("kpm"), py::arg("lut"), py::arg("scale"), py::arg("causal"), py::arg("p"),
        py::arg("seed"), py::arg("need_dlut"), py::arg("dq_out") = py::none(), py::arg("dk_out") = py::none(),
        py::arg("dv_out") = py::none(), py::arg("dmask") = py::none(), py::arg("sat_lo") = -1,
        py::arg("sat_hi") = -1, py::arg("csq") = py::none(), py::arg("csk") = py::none(),
        py::arg("csv") = py::none());
  m.def("attn_f32_fwd", &attn_f32_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kpm"), py::arg("lut"),
        py::arg("scale"), py::arg("causal"), py::arg("p"), py::arg("seed"), py::arg("window") = -1,
        py::arg("q_seg") = py::none(), py::arg("k_seg") = py::none(), py::arg("q_blk") = py::none(), py::arg("k_blk") = py::none(),
        py::arg("k_glob") = py::none(), py::arg("k_gblk") = py::none(), py::arg("kl_ptr") = py::none(),
        py::arg("kl_idx") = py::none(), py::arg("ql_ptr") = py::none(), py::arg("ql_idx") = py::none(),
        py::arg("softcap") = 0.0);
  m.def("attn_f32_bwd", &attn_f32_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("kpm"), py::arg("lut"), py::arg("scale"), py::arg("causal"), py::arg("p"),
        py::arg("seed"), py::arg("need_dlut"), py::arg("dq_out") = py::none(), py::arg("dk_out") = py::none(),
        py::arg("dv_out") = py::none(), py::arg("window") = -1, py::arg("q_seg") = py::none(),
        py::arg("k_seg") = py::none(), py::arg("q_blk") = py::none(), py::arg("k_blk") = py::none(),
        py::arg("k_glob") = py::none(), py::arg("k_gblk") = py::none(), py::arg("kl_ptr") = py::none(),
        py::arg("kl_idx") = py::none(), py::arg("ql_ptr") = py::none(), py::arg("ql_idx") = py::none(),
        py::arg("softcap") = 0.0);
  m.def("attn_hd_fwd", &attn_hd_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kpm"), py::arg("lut"),
        py::arg("scale"), py::arg("causal"), py::arg("p"), py::arg("seed"), py::arg("window") = -1,
        py::arg("q_seg") = py::none(), py::arg("k_seg") = py::none(), py::arg("q_blk") = py::none(), py::arg("k_blk") = py::none(),
        py::arg("k_glob") = py::none(), py::arg("k_gblk") = py::none(), py::arg("kl_ptr") = py::none(),
        py::arg("kl_idx") = py::none(), py::arg("ql_ptr") = py::none(), py::arg("ql_idx") = py::none(),
        py::arg("softcap") = 0.0);
  m.def("attn_hd_bwd", &attn_hd_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("kpm"), py::arg("lut"), py::arg("scale"), py::arg("causal"), py::arg("p"),
        py::arg("seed"), py::arg("need_dlut"), py::arg("dq_out") = py::none(), py::arg("dk_out") = py::none(),
        py::arg("dv_out") = py::none(), py::arg("window") = -1, py::arg("q_seg") = py::none(),
        py::arg("k_seg") = py::none(), py::arg("q_blk") = py::none(), py::arg("k_blk") = py::none(),
        py::arg("k_glob") = py::none(), py::arg("k_gblk") = py::none(), py::arg("kl_ptr") = py::none(),
        py::arg("kl_idx") = py::none(), py::arg("ql_ptr") = py::none(), py::arg("ql_idx") = py::none(),
        py::arg("softcap") = 0.0);
}

}  // namespace dllm
