// Python bindings for the gfx950 kernel library (one in-tree extension: distributed_llms_example_amd/_C): the module,
// assembled from the family files csrc/bind_<family>.cpp.  The launchers are declared in csrc/launchers.h; host-side
// validation (csrc/bind_common.h) runs BEFORE every launch, then the C-ABI launchers in csrc/*.hip run on the current
// torch HIP stream.
#include "bind_common.h"

namespace dllm {
namespace {

// Device step counter for graph-replayable dropout (csrc/common.h DLLM_SEED_STEP_TU): every dropout kernel mixes
// *step into its site seed; None turns it off (site seeds used as given).  The tensor must outlive its use.
void set_seed_step(const optional<Tensor>& step) {
  const uint32_t* p = nullptr;
  if (has(step))
    p = reinterpret_cast<const uint32_t*>(flat_ptr<const int>(*step, *step, at::kInt, exactly(1), "set_seed_step: step"));
#define DLLM_SET_SEED_STEP(tu) check_rc(dllm_set_seed_step_##tu(p), "set_seed_step(" #tu ")");
  DLLM_SEED_STEP_TUS(DLLM_SET_SEED_STEP)
#undef DLLM_SET_SEED_STEP
}

}  // namespace
}  // namespace dllm

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 (MI355X) kernel library for distributed_llms_example_amd";
  m.def("set_seed_step", &dllm::set_seed_step, "device step counter mixed into every dropout site seed (None: off)");
  dllm::bind_rowwise(m);
  dllm::bind_loss(m);
  dllm::bind_optim(m);
  dllm::bind_attn(m);
  dllm::bind_gemm(m);
  dllm::bind_generate(m);
  dllm::bind_lora(m);
  dllm::bind_reducer(m);
  m.attr("arch") = "gfx950";
}
