// Torch extension bindings for the framed drain (csrc/hip/framed_drain.hip).
// Module `pushcdn_gpu_drain`, apart from the data-plane module `pushcdn_gpu`,
// the maintenance module `pushcdn_gpu_ctl` and the loss-accounting module
// `pushcdn_gpu_acct`; the argument checks are the same `Op`
// (csrc/binding_checks.h).

#include "binding_checks.h"
#include "hip/framed_drain.h"

// K11: every ring's records as [u32 BE len][message] frames in seq order,
// into staging[dst_off[r] : dst_off[r] + wpos[r]]; frame_len[r] bytes of
// frame_cnt[r] frames, or frame_cnt[r] = -1 and the raw prefix (an
// out-of-order ring of more than FRAME_SORT_MAX records).  wpos is only read.
// max_chunks: the copy grid's second dimension, at least
// ceil(max wpos / CHUNK_BYTES); -1 sizes it for a full ring.
void frame_rings(torch::Tensor egress, int64_t ring_bytes, torch::Tensor wpos,
                 torch::Tensor dst_off, torch::Tensor staging, torch::Tensor frame_len,
                 torch::Tensor frame_cnt, torch::Tensor index, int64_t max_chunks) {
    Op a("frame_rings");
    const int32_t n = a.i32(wpos.numel(), "ring count");
    a.ring_bytes(ring_bytes);
    const int64_t full = (ring_bytes + K11_CHUNK - 1) / K11_CHUNK;
    a.i32(full, "ring_bytes in copy chunks", 0, 65535);
    const int32_t chunks = a.i32(max_chunks < 0 ? full : max_chunks, "max_chunks", 0, 65535);
    const uint8_t* eg = a.ptr<uint8_t>(egress, "egress", n * ring_bytes, vec());
    const int64_t* wp = a.ptr<int64_t>(wpos, "wpos", 0, vec());
    const int64_t* doff = a.same<int64_t>(dst_off, "dst_off", n, "one per wpos", vec());
    uint8_t* st = a.ptr<uint8_t>(staging, "staging", 0, vec());
    int64_t* fl = a.same<int64_t>(frame_len, "frame_len", n, "one per wpos", vec());
    int32_t* fc = a.same<int32_t>(frame_cnt, "frame_cnt", n, "one per wpos", vec());
    // one 16 B entry per 16 B of staging: a record is at least that long
    FrameIdx* ix = reinterpret_cast<FrameIdx*>(
        a.ptr<int32_t>(index, "index", staging.numel() / 16 * 4, mat(-1, 4)));
    hipStream_t s = a.begin();
    if (n == 0) return;
    launch_k11_frame_rings(eg, ring_bytes, wp, doff, st, staging.numel(), fl, fc, ix, n, chunks,
                           s);
    a.launched();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // the ring-mode rule's constant and the copy grid's chunk, for the engine
    // and the tests
    m.attr("FRAME_SORT_MAX") = py::int_(FRAME_SORT_MAX);
    m.attr("CHUNK_BYTES") = py::int_(K11_CHUNK);
    m.def("frame_rings", &frame_rings,
          "K11: egress rings as socket-ready length-prefixed frames in seq order",
          py::arg("egress"), py::arg("ring_bytes"), py::arg("wpos"), py::arg("dst_off"),
          py::arg("staging"), py::arg("frame_len"), py::arg("frame_cnt"), py::arg("index"),
          py::arg("max_chunks") = -1);
}
