// Torch extension bindings for the loss-accounting kernels
// (csrc/hip/accounting.hip).  Module `pushcdn_gpu_acct`, apart from the
// data-plane module `pushcdn_gpu` and the maintenance module
// `pushcdn_gpu_ctl`; the argument checks are the same `Op`
// (csrc/binding_checks.h).

#include <optional>

#include "binding_checks.h"
#include "hip/accounting.h"

// K9: demand[r] += ring bytes this tick wants to deliver to r.  R, the
// recipient count, is demand's length and must be n_users + n_peers; the mask
// has one word per 64 recipients.  owner = None: the tick routes no Directs;
// origin = None: every message is local-origin.
void recipient_demand(torch::Tensor demand, torch::Tensor mask_t, torch::Tensor ring_len,
                      torch::Tensor disc, std::optional<torch::Tensor> owner,
                      std::optional<torch::Tensor> origin, int64_t n_users, int64_t n_peers) {
    Op a("recipient_demand");
    uint64_t* dem = a.ptr<uint64_t>(demand, "demand", 0, vec());
    const int32_t nu = a.i32(n_users, "n_users");
    const int32_t np = a.i32(n_peers, "n_peers", 0, INT32_MAX - n_users);
    const int32_t R = a.i32(demand.numel(), "demand length", int64_t(nu) + np, int64_t(nu) + np);
    const int32_t W = (R + 63) / 64;
    const int32_t M = a.i32(ring_len.numel(), "M");
    const uint64_t* mask = a.ptr<uint64_t>(mask_t, "mask_t", 0, mat(W, M));
    const int32_t* len = a.ptr<int32_t>(ring_len, "ring_len", 0, vec());
    const int32_t* dsc = a.same<int32_t>(disc, "disc", M, "one per ring_len", vec());
    const int32_t* own = owner
        ? a.same<int32_t>(*owner, "owner", M, "one per ring_len", vec()) : nullptr;
    const int32_t* org = origin
        ? a.same<int32_t>(*origin, "origin", M, "one per ring_len", vec()) : nullptr;
    hipStream_t s = a.begin();
    if (M == 0 || R == 0) return;
    launch_k9_recipient_demand(mask, len, dsc, own, org, M, W, nu, np, dem, s);
    a.launched();
}

// K10: compact list of the recipients whose demand differs from their cursor,
// and the count into pinned host memory with one 4-byte asynchronous copy.
// Does NOT synchronise: the drain's own synchronisation on the same stream
// (the cursor readback) makes n_host readable.
void loss_scan(torch::Tensor demand, torch::Tensor ring_wpos, torch::Tensor lossy,
               torch::Tensor n_lossy, torch::Tensor n_host) {
    Op a("loss_scan");
    uint64_t* dem = a.ptr<uint64_t>(demand, "demand", 0, vec());
    const int32_t R = a.i32(demand.numel(), "demand length");
    const int64_t* wpos = a.same<int64_t>(ring_wpos, "ring_wpos", R, "one per demand", vec());
    // [>= R][2]: a row per recipient, so the list cannot overflow
    LossRec* list =
        reinterpret_cast<LossRec*>(a.ptr<int64_t>(lossy, "lossy", int64_t(R) * 2, mat(-1, 2)));
    int32_t* n = a.ptr<int32_t>(n_lossy, "n_lossy", 1, vec());
    int32_t* h = a.ptr<int32_t>(n_host, "n_host", 1, vec(), Op::kPinnedHost);
    hipStream_t s = a.begin();
    a.check(launch_k10_loss_scan(dem, wpos, list, n, R, s), "zeroing n_lossy");
    a.launched();
    a.check(hipMemcpyAsync(h, n, sizeof(int32_t), hipMemcpyDeviceToHost, s), "copy");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // waves that split one mask word's message range, for the tests' shapes
    m.attr("_K9_WAVES") = py::int_(K9_WAVES);
    m.def("recipient_demand", &recipient_demand,
          "K9: per-recipient ring bytes demanded by one tick, added to demand",
          py::arg("demand"), py::arg("mask_t"), py::arg("ring_len"), py::arg("disc"),
          py::arg("owner"), py::arg("origin"), py::arg("n_users"), py::arg("n_peers"));
    m.def("loss_scan", &loss_scan,
          "K10: (recipient, demand - cursor) list of the lossy recipients; demand zeroed");
}
