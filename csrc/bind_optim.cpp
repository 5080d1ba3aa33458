// Optimizer kernels: gradient norm and AdamW (csrc/adamw.hip), Adafactor (csrc/adafactor.hip).  They walk every
// buffer as one flat array with 16-B (the AdamW decay mask: 8-B) vector accesses.
#include "bind_common.h"

#include "adafactor_params.h"

namespace dllm {
namespace {

const at::ScalarType kParamDtypes[] = {at::kBFloat16, at::kFloat};
constexpr Flat kAnyScalar{0, true, false, 1};  // coef: an fp32 device scalar of any layout, as before

Tensor sq_norm(const Tensor& g) {
  const void* gp = flat_ptr<const void>(g, g, kParamDtypes, at_least(0, 16), "sq_norm: g");
  TORCH_CHECK(g.numel() % 4 == 0, "sq_norm: contiguous, numel % 4 == 0");
  auto f32 = g.options().dtype(at::kFloat);
  auto part = at::empty({1024}, f32);
  auto out = at::empty({}, f32);
  check_rc(dllm_sq_norm(gp, g.numel(), part.data_ptr<float>(), out.data_ptr<float>(), is_bf16(g), stream()),
           "sq_norm");
  return out;
}

void adamw_step(Tensor param, const optional<Tensor>& master, const Tensor& grad, Tensor m, Tensor v,
                const optional<Tensor>& wd_mask, const Tensor& coef, double lr, double b1, double b2, double eps,
                double wd, double bc1, double bc2, const optional<Tensor>& hyper) {
  void* param_p = flat_ptr<void>(param, param, kParamDtypes, at_least(0, 16), "adamw: param");
  const long n = param.numel();
  TORCH_CHECK(n % 4 == 0, "adamw: flat buffers must match, numel % 4 == 0");
  const void* grad_p = flat_ptr<const void>(grad, param, {param.scalar_type(), at::kFloat}, exactly(n, 16),
                                            "adamw: grad");
  float* m_p = flat_ptr<float>(m, param, at::kFloat, exactly(n, 16), "adamw: moment m");
  float* v_p = flat_ptr<float>(v, param, at::kFloat, exactly(n, 16), "adamw: moment v");
  float* master_p = flat_ptr<float>(master, param, at::kFloat, exactly(n, 16), "adamw: master");
  const uint8_t* mask_p = flat_ptr<const uint8_t>(wd_mask, param, at::kByte, exactly(n, 8), "adamw: wd_mask");
  const float* coef_p = flat_ptr<const float>(coef, param, at::kFloat, kAnyScalar, "adamw: coef");
  // [lr, lr / bc1, 1 / sqrt(bc2)]
  const float* hyper_p = flat_ptr<const float>(hyper, param, at::kFloat, at_least(3), "adamw: hyper");
  check_rc(dllm_adamw(param_p, master_p, grad_p, m_p, v_p, mask_p, coef_p, n, (float)lr, (float)b1, (float)b2,
                      (float)eps, (float)wd, (float)bc1, (float)bc2, is_bf16(param),
                      grad.scalar_type() == at::kFloat, hyper_p, stream()),
           "adamw");
}

// Adafactor (csrc/adafactor.hip).  adafactor_plan lays out the unit table the kernels walk: `units` is a CPU int64
// [U, 6] of (flat offset, rows, cols, R|V offset, C offset or -1, decay flag) per unit; the result is the [U + 1,
// AF_FIELDS] table (csrc/adafactor_params.h) with tile prefix sums and scratch offsets, the tile count and the sizes of
// the column- and row-partial scratch buffers (floats).
std::tuple<Tensor, int64_t, int64_t, int64_t> adafactor_plan(const Tensor& units) {
  TORCH_CHECK(!units.is_cuda() && units.scalar_type() == at::kLong && units.dim() == 2 && units.size(1) == 6 &&
                  units.is_contiguous() && units.size(0) >= 1, "adafactor_plan: units must be a CPU int64 [U, 6]");
  const int64_t U = units.size(0);
  const int64_t* u = units.data_ptr<int64_t>();  // host table, read here
  Tensor tab = at::zeros({U + 1, (int64_t)AF_FIELDS}, units.options());
  int64_t* t = tab.data_ptr<int64_t>();
  int64_t tiles = 0, colpart = 0, rowpart = 0;
  for (int64_t i = 0; i < U; ++i) {
    const int64_t off = u[i * 6 + 0], nr = u[i * 6 + 1], nc = u[i * 6 + 2], rv = u[i * 6 + 3], c = u[i * 6 + 4];
    TORCH_CHECK(off >= 0 && nr >= 1 && nc >= 1 && rv >= 0 && (c >= 0 || nr == 1), "adafactor_plan: unit ", i);
    int64_t* r = t + i * AF_FIELDS;
    const int64_t nchunk = (nc + AF_CC - 1) / AF_CC, nrb = (nr + AF_RB - 1) / AF_RB;
    r[AF_OFF] = off; r[AF_ROWS] = nr; r[AF_COLS] = nc; r[AF_RV] = rv; r[AF_C] = c < 0 ? -1 : c;
    r[AF_DECAY] = u[i * 6 + 5] != 0;
    r[AF_TILE0] = tiles; r[AF_NCHUNK] = nchunk; r[AF_SCAL] = i;
    r[AF_COLPART] = colpart; r[AF_ROWPART] = rowpart;
    r[AF_VEC] = nc % 4 == 0 && off % 4 == 0 && rv % 4 == 0 && (c < 0 || c % 4 == 0);
    tiles += nrb * nchunk;
    if (c >= 0) {
      colpart += (nrb * nc + 3) / 4 * 4;
      rowpart += nr * nchunk;
    }
  }
  t[U * AF_FIELDS + AF_TILE0] = tiles;
  return {tab, tiles, std::max<int64_t>(colpart, 4), std::max<int64_t>(rowpart, 4)};
}

std::vector<int64_t> adafactor_geometry() {
  return {AF_RB, AF_WC, AF_CC, AF_GRID_CAP, AF_FIN_SLICES, AF_FIN_COLS};
}

void adafactor_step(Tensor param, const optional<Tensor>& master, const Tensor& grad, Tensor rv, Tensor cst,
                    const Tensor& tab_dev, const Tensor& tab_host, Tensor scal, Tensor colpart, Tensor rowpart,
                    Tensor tpart, const Tensor& coef, double rel, double b2t, double eps1, double eps2, double clip_thr,
                    double wd, bool scale_param, const optional<Tensor>& hyper) {
  void* param_p = flat_ptr<void>(param, param, kParamDtypes, at_least(0, 16), "adafactor: param");
  const int64_t n = param.numel();
  const bool bf16 = is_bf16(param);
  const float* grad_p = flat_ptr<const float>(grad, param, at::kFloat, exactly(n, 16), "adafactor: grad");
  TORCH_CHECK(bf16 == has(master), "adafactor: bf16 parameters need an fp32 master, fp32 parameters take none");
  float* master_p = flat_ptr<float>(master, param, at::kFloat, exactly(n, 16), "adafactor: master");
  auto state = [&](const Tensor& t, const char* name) {  // sizes: against the table, below
    return flat_ptr<float>(t, param, at::kFloat, at_least(0, 16), "adafactor: ", name);
  };
  float *rv_p = state(rv, "rv"), *cst_p = state(cst, "c"), *scal_p = state(scal, "scal");
  float *colpart_p = state(colpart, "colpart"), *rowpart_p = state(rowpart, "rowpart"), *tpart_p = state(tpart, "tpart");
  const float* coef_p = flat_ptr<const float>(coef, param, at::kFloat, kAnyScalar, "adafactor: coef");
  const float* hyper_p = flat_ptr<const float>(hyper, param, at::kFloat, at_least(2), "adafactor: hyper [rel, beta2t]");
  TORCH_CHECK(!tab_host.is_cuda() && tab_host.scalar_type() == at::kLong && tab_host.dim() == 2 &&
                  tab_host.size(1) == AF_FIELDS && tab_host.size(0) >= 2 && tab_host.is_contiguous(),
              "adafactor: host table must be a CPU int64 [U + 1, fields]");
  TORCH_CHECK(tab_dev.sizes() == tab_host.sizes(), "adafactor: device table must be the host table's copy");
  const int64_t* tab_p = flat_ptr<const int64_t>(tab_dev, param, at::kLong, exactly(tab_host.numel()),
                                                 "adafactor: device table");
  // every range a kernel will touch, checked on the host copy of the table before anything is launched
  const int64_t U = tab_host.size(0) - 1;
  const int64_t* t = tab_host.data_ptr<int64_t>();  // host table, read here
  int64_t tiles = 0;
  for (int64_t i = 0; i < U; ++i) {
    const int64_t* r = t + i * AF_FIELDS;
    const int64_t nr = r[AF_ROWS], nc = r[AF_COLS], c = r[AF_C];
    TORCH_CHECK(nr >= 1 && nc >= 1 && nc <= n && nr <= n / nc && r[AF_OFF] >= 0 &&
                    r[AF_OFF] <= n - nr * nc,
                "adafactor: unit ", i, " lies outside the flat buffer");
    const int64_t nchunk = (nc + AF_CC - 1) / AF_CC, nrb = (nr + AF_RB - 1) / AF_RB;
    TORCH_CHECK(r[AF_TILE0] == tiles && r[AF_NCHUNK] == nchunk && r[AF_SCAL] >= 0 && r[AF_SCAL] < U,
                "adafactor: unit ", i, " has an inconsistent tile layout");
    TORCH_CHECK(r[AF_RV] >= 0 && r[AF_RV] + (c < 0 ? nc : nr) <= rv.numel() && (c >= 0 || nr == 1) &&
                    (c < 0 || c + nc <= cst.numel()), "adafactor: unit ", i, " state lies outside its buffer");
    if (c >= 0)
      TORCH_CHECK(r[AF_COLPART] >= 0 && r[AF_COLPART] + nrb * nc <= colpart.numel() && r[AF_ROWPART] >= 0 &&
                      r[AF_ROWPART] + nr * nchunk <= rowpart.numel(), "adafactor: unit ", i, " scratch out of range");
    if (r[AF_VEC])
      TORCH_CHECK(nc % 4 == 0 && r[AF_OFF] % 4 == 0 && r[AF_RV] % 4 == 0 && (c < 0 || (c % 4 == 0 &&
                      r[AF_COLPART] % 4 == 0)), "adafactor: unit ", i, " is not aligned for 16-byte access");
    tiles += nrb * nchunk;
  }
  TORCH_CHECK(t[U * AF_FIELDS + AF_TILE0] == tiles && tpart.numel() >= 2 * tiles && scal.numel() >= 4 * U &&
                  U <= INT_MAX, "adafactor: tile scratch / scalar array too small");
  check_rc(dllm_adafactor_step(param_p, master_p, grad_p, rv_p, cst_p, reinterpret_cast<const long*>(tab_p), (int)U,
                               (long)tiles, scal_p, colpart_p, rowpart_p, tpart_p, coef_p, (float)rel, (float)b2t,
                               (float)eps1, (float)eps2, (float)clip_thr, (float)wd, scale_param ? 1 : 0, bf16 ? 1 : 0,
                               hyper_p, stream()),
           "adafactor");
}

}  // namespace

void bind_optim(pybind11::module& m) {
  m.def("sq_norm", &sq_norm);
  m.def("adamw_step", &adamw_step, py::arg("param"), py::arg("master"), py::arg("grad"), py::arg("m"), py::arg("v"),
        py::arg("wd_mask"), py::arg("coef"), py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"),
        py::arg("bc1"), py::arg("bc2"), py::arg("hyper") = py::none());
  m.def("adafactor_plan", &adafactor_plan, "unit table, tile count and scratch sizes of csrc/adafactor.hip");
  m.def("adafactor_geometry", &adafactor_geometry, "[rows per tile, cols per wave, cols per tile, grid cap, ...]");
  m.def("adafactor_step", &adafactor_step, py::arg("param"), py::arg("master"), py::arg("grad"), py::arg("rv"),
        py::arg("c"), py::arg("table"), py::arg("table_host"), py::arg("scal"), py::arg("colpart"), py::arg("rowpart"),
        py::arg("tpart"), py::arg("coef"), py::arg("rel"), py::arg("beta2t"), py::arg("eps1"), py::arg("eps2"),
        py::arg("clip_threshold"), py::arg("weight_decay"), py::arg("scale_parameter"), py::arg("hyper") = py::none());
}

}  // namespace dllm
