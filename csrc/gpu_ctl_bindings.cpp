// Torch extension bindings for the device-state maintenance kernels
// (csrc/hip/membership.hip): ops that change the HBM-resident routing state
// between ticks.  Module `pushcdn_gpu_ctl`, apart from the data-plane module
// `pushcdn_gpu`; the argument checks are the same `Op` (csrc/binding_checks.h).

#include "binding_checks.h"
#include "hip/membership.h"

// K8: apply coalesced membership rows.  R, the recipient count, is
// ring_wpos' length; every recipient needs a bit in the [256][W] bitmap.
void membership_apply(torch::Tensor sub_bitmap, torch::Tensor ring_wpos, torch::Tensor recs) {
    Op a("membership_apply");
    uint64_t* bitmap = a.ptr<uint64_t>(sub_bitmap, "sub_bitmap", 0, mat(256, -1));
    const int32_t W = a.i32(sub_bitmap.size(1), "W");
    int64_t* wpos = a.ptr<int64_t>(ring_wpos, "ring_wpos", 0, vec());
    const int32_t R = a.i32(ring_wpos.numel(), "ring_wpos length", 0, int64_t(W) * 64);
    const int64_t* rows = a.ptr<int64_t>(recs, "recs", 0, mat(-1, MEMBERSHIP_WORDS));
    const int32_t n = a.i32(recs.size(0), "n");
    hipStream_t s = a.begin();
    if (n == 0) return;
    launch_k8_membership_apply(bitmap, wpos, rows, n, W, R, s);
    a.launched();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // grid cap of K8, for the test that exercises its grid-stride loop
    m.attr("_K8_MAX_BLOCKS") = py::int_(K8_MAX_BLOCKS);
    m.def("membership_apply", &membership_apply,
          "K8: coalesced membership rows -> subscription bitmap bits + ring cursor resets");
}
