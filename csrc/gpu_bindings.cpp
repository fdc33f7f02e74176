// Torch extension bindings for the MI355X broker data-plane kernels
// (csrc/hip/dataplane.hip). PyTorch owns every HBM buffer; these calls
// invoke the extern "C" launchers defined next to the kernels and declared
// in csrc/hip/dataplane.h and csrc/hip/bls_kernels.h.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip/bls_kernels.h"
#include "hip/dataplane.h"

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be on the GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static inline PairRec* pair_ptr(torch::Tensor& pairs) {
    TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 4 && pairs.dtype() == torch::kInt32
                && pairs.is_contiguous(), "pairs must be a contiguous int32 [cap, 4] tensor");
    return (PairRec*)pairs.data_ptr<int32_t>();
}

static inline hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

// Options for a new tensor of `dtype` on the device of `like`.
static inline torch::TensorOptions opts(torch::ScalarType dtype, const torch::Tensor& like) {
    return torch::TensorOptions().dtype(dtype).device(like.device());
}

// The flat K3 kernels index units with an exact u32 magic division
// (csrc/common/divmagic.h) that holds only for d <= 2^21 and f < 2^31, and
// truncate the flat unit index to u32: refuse shapes outside that envelope
// instead of silently misplacing records.
static inline void check_flat_shape(const torch::Tensor& pairs, int64_t units_per_pair) {
    TORCH_CHECK(units_per_pair >= 1 && units_per_pair <= (int64_t(1) << 21),
                "units_per_pair must be in [1, 2^21], got ", units_per_pair);
    TORCH_CHECK(pairs.size(0) * units_per_pair < (int64_t(1) << 31),
                "pair capacity * units_per_pair must be < 2^31, got ", pairs.size(0), " * ",
                units_per_pair);
}

std::vector<torch::Tensor> parse_batch(torch::Tensor buf, torch::Tensor offsets,
                                       uint64_t hash_seed) {
    CHECK_DEV(buf); CHECK_CONTIG(buf); CHECK_DEV(offsets); CHECK_CONTIG(offsets);
    TORCH_CHECK(buf.dtype() == torch::kUInt8 && offsets.dtype() == torch::kInt64);
    int32_t M = (int32_t)offsets.size(0) - 1;
    TORCH_CHECK(M >= 0);
    auto o32 = opts(torch::kInt32, buf);
    auto o64 = opts(torch::kInt64, buf);
    auto disc = torch::empty({M}, o32);
    auto payload_off = torch::empty({M}, o64);
    auto payload_len = torch::empty({M}, o32);
    auto topics_off = torch::empty({M}, o64);
    auto topics_cnt = torch::empty({M}, o32);
    auto recip_hash = torch::empty({M}, o64);  // bit-cast u64
    auto timestamp = torch::empty({M}, o64);
    if (M > 0) {
        ParseOut out{disc.data_ptr<int32_t>(), payload_off.data_ptr<int64_t>(),
                     payload_len.data_ptr<int32_t>(), topics_off.data_ptr<int64_t>(),
                     topics_cnt.data_ptr<int32_t>(),
                     (uint64_t*)recip_hash.data_ptr<int64_t>(),
                     (uint64_t*)timestamp.data_ptr<int64_t>()};
        launch_k4_parse(buf.data_ptr<uint8_t>(), offsets.data_ptr<int64_t>(), M, hash_seed,
                        out, cur_stream());
    }
    return {disc, payload_off, payload_len, topics_off, topics_cnt, recip_hash, timestamp};
}

// Shared part of the three K2a wrappers: M and W from disc and the bitmap,
// the mask allocation ([M][W], or [W][M] when transposed) and the M > 0
// guard around launch(mask, M, W).  Each wrapper does its own checks first.
template <typename Launch>
static torch::Tensor k2a_mask(const torch::Tensor& sub_bitmap, const torch::Tensor& buf,
                              const torch::Tensor& disc, bool transposed, Launch launch) {
    int32_t W = (int32_t)sub_bitmap.size(1);
    int32_t M = (int32_t)disc.size(0);
    auto mask = transposed ? torch::empty({(int64_t)W, M}, opts(torch::kInt64, buf))
                           : torch::empty({M, (int64_t)W}, opts(torch::kInt64, buf));
    if (M > 0) launch((uint64_t*)mask.data_ptr<int64_t>(), M, W);
    return mask;
}

torch::Tensor topic_mask(torch::Tensor sub_bitmap, torch::Tensor buf, torch::Tensor topics_off,
                         torch::Tensor topics_cnt, torch::Tensor disc) {
    CHECK_DEV(sub_bitmap); CHECK_CONTIG(sub_bitmap);
    TORCH_CHECK(sub_bitmap.dim() == 2 && sub_bitmap.size(0) == 256);
    return k2a_mask(sub_bitmap, buf, disc, false, [&](uint64_t* mask, int32_t M, int32_t W) {
        launch_k2a_topic_mask((const uint64_t*)sub_bitmap.data_ptr<int64_t>(),
                              buf.data_ptr<uint8_t>(), topics_off.data_ptr<int64_t>(),
                              topics_cnt.data_ptr<int32_t>(), disc.data_ptr<int32_t>(), mask, M,
                              W, cur_stream());
    });
}

std::vector<torch::Tensor> assign_emit(torch::Tensor mask, torch::Tensor payload_off,
                                       torch::Tensor payload_len, torch::Tensor ring_wpos,
                                       int64_t ring_bytes, int64_t n_users) {
    CHECK_DEV(mask); CHECK_CONTIG(mask);
    int32_t M = (int32_t)mask.size(0);
    int32_t W = (int32_t)mask.size(1);
    TORCH_CHECK(ring_bytes % 16 == 0, "ring_bytes must be a multiple of 16");
    auto o32 = opts(torch::kInt32, mask);
    auto counts = torch::zeros({n_users}, o32);
    launch_k2b_count((const uint64_t*)mask.data_ptr<int64_t>(), M, W, (int32_t)n_users,
                     counts.data_ptr<int32_t>(), cur_stream());
    auto cum = counts.cumsum(0).to(torch::kInt32);
    auto pair_base = (cum - counts).contiguous();  // exclusive scan
    int64_t total = cum[n_users - 1].item<int32_t>();  // one small D2H sync
    auto pairs = torch::empty({total, 4}, o32);
    auto drops = torch::zeros({1}, o32);
    launch_k2b_emit((const uint64_t*)mask.data_ptr<int64_t>(), payload_off.data_ptr<int64_t>(),
                    payload_len.data_ptr<int32_t>(), pair_base.data_ptr<int32_t>(), M, W,
                    (int32_t)n_users, ring_bytes, (uint64_t*)ring_wpos.data_ptr<int64_t>(),
                    pair_ptr(pairs), (uint32_t*)drops.data_ptr<int32_t>(), cur_stream());
    // split the AoS records back into the golden-test API's three tensors
    auto pair_user = pairs.select(1, 0).contiguous();
    auto pair_msg = pairs.select(1, 1).contiguous();
    auto pair_dst = pairs.slice(1, 2, 4).contiguous().view(torch::kInt64).squeeze(1);
    return {pair_user, pair_msg, pair_dst, drops};
}

void fanout(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
            torch::Tensor pair_user, torch::Tensor pair_msg, torch::Tensor pair_dst,
            torch::Tensor msg_seq, torch::Tensor egress) {
    CHECK_DEV(egress); CHECK_CONTIG(egress);
    int32_t n_pairs = (int32_t)pair_user.size(0);
    if (n_pairs == 0) return;
    auto pairs = torch::empty({n_pairs, 4}, opts(torch::kInt32, buf));
    pairs.select(1, 0).copy_(pair_user);
    pairs.select(1, 1).copy_(pair_msg);
    pairs.slice(1, 2, 4).view(torch::kInt64).squeeze(1).copy_(pair_dst);
    launch_k3_fanout(buf.data_ptr<uint8_t>(), payload_off.data_ptr<int64_t>(),
                     payload_len.data_ptr<int32_t>(), pair_ptr(pairs),
                     (const uint32_t*)msg_seq.data_ptr<int32_t>(), n_pairs,
                     egress.data_ptr<uint8_t>(), cur_stream());
}

torch::Tensor direct_lookup(torch::Tensor table_keys, torch::Tensor table_vals,
                            torch::Tensor query) {
    CHECK_DEV(table_keys); CHECK_DEV(query);
    int64_t S = table_keys.size(0);
    TORCH_CHECK((S & (S - 1)) == 0, "table size must be a power of two");
    int32_t N = (int32_t)query.size(0);
    auto owner = torch::empty({N}, opts(torch::kInt32, query));
    if (N > 0) {
        launch_k5_direct_lookup((const uint64_t*)table_keys.data_ptr<int64_t>(),
                                table_vals.data_ptr<int32_t>(), S,
                                (const uint64_t*)query.data_ptr<int64_t>(), N,
                                owner.data_ptr<int32_t>(), cur_stream());
    }
    return owner;
}

void apply_subs(torch::Tensor sub_bitmap, torch::Tensor buf, torch::Tensor topics_off,
                torch::Tensor topics_cnt, torch::Tensor disc, torch::Tensor user_idx) {
    CHECK_DEV(sub_bitmap); CHECK_CONTIG(sub_bitmap);
    int32_t W = (int32_t)sub_bitmap.size(1);
    int32_t M = (int32_t)disc.size(0);
    if (M == 0) return;
    launch_k2c_apply_subs((uint64_t*)sub_bitmap.data_ptr<int64_t>(), buf.data_ptr<uint8_t>(),
                          topics_off.data_ptr<int64_t>(), topics_cnt.data_ptr<int32_t>(),
                          disc.data_ptr<int32_t>(), user_idx.data_ptr<int32_t>(), M, W,
                          cur_stream());
}

torch::Tensor bls_verify_batch(torch::Tensor vks, torch::Tensor sigs, torch::Tensor msgs,
                               torch::Tensor moff) {
    CHECK_DEV(vks); CHECK_DEV(sigs); CHECK_DEV(msgs); CHECK_DEV(moff);
    CHECK_CONTIG(vks); CHECK_CONTIG(sigs); CHECK_CONTIG(msgs); CHECK_CONTIG(moff);
    int32_t N = (int32_t)moff.size(0) - 1;
    TORCH_CHECK(vks.numel() == (int64_t)N * 128 && sigs.numel() == (int64_t)N * 64);
    auto ok = torch::zeros({N}, opts(torch::kInt32, vks));
    if (N > 0) {
        launch_k1_bls_verify(vks.data_ptr<uint8_t>(), sigs.data_ptr<uint8_t>(),
                             msgs.data_ptr<uint8_t>(), moff.data_ptr<int64_t>(), N,
                             ok.data_ptr<int32_t>(), cur_stream());
    }
    return ok;
}

void compact_rings(torch::Tensor egress, int64_t ring_bytes, torch::Tensor wpos,
                   torch::Tensor dst_off, torch::Tensor staging, int64_t max_chunks) {
    CHECK_DEV(egress); CHECK_DEV(wpos); CHECK_DEV(dst_off); CHECK_DEV(staging);
    CHECK_CONTIG(egress); CHECK_CONTIG(wpos); CHECK_CONTIG(dst_off); CHECK_CONTIG(staging);
    TORCH_CHECK(wpos.dtype() == torch::kInt64 && dst_off.dtype() == torch::kInt64);
    int32_t n = (int32_t)wpos.size(0);
    launch_k7_compact_rings(egress.data_ptr<uint8_t>(), ring_bytes,
                            wpos.data_ptr<int64_t>(), dst_off.data_ptr<int64_t>(),
                            staging.data_ptr<uint8_t>(), n, (int32_t)max_chunks,
                            cur_stream());
}

torch::Tensor precompute_g2_lines(torch::Tensor device_probe) {
    // fixed-g2 Miller-loop line coefficients (128 records x 192 B); computed
    // once per process by a 1-thread kernel, consumed by bls_verify_batch2
    auto out = torch::zeros({128 * 192}, opts(torch::kUInt8, device_probe));
    auto n = torch::zeros({1}, opts(torch::kInt32, device_probe));
    launch_k1_precompute_g2_lines(out.data_ptr<uint8_t>(), n.data_ptr<int32_t>(),
                                  cur_stream());
    return out;
}

torch::Tensor bls_verify_batch2(torch::Tensor vks, torch::Tensor sigs, torch::Tensor msgs,
                                torch::Tensor moff, torch::Tensor g2_lines) {
    CHECK_DEV(vks); CHECK_DEV(sigs); CHECK_DEV(msgs); CHECK_DEV(moff); CHECK_DEV(g2_lines);
    CHECK_CONTIG(vks); CHECK_CONTIG(sigs); CHECK_CONTIG(msgs); CHECK_CONTIG(moff);
    CHECK_CONTIG(g2_lines);
    int32_t N = (int32_t)moff.size(0) - 1;
    TORCH_CHECK(vks.numel() == (int64_t)N * 128 && sigs.numel() == (int64_t)N * 64);
    auto ok = torch::zeros({N}, opts(torch::kInt32, vks));
    if (N > 0) {
        launch_k1_bls_verify2(vks.data_ptr<uint8_t>(), sigs.data_ptr<uint8_t>(),
                              msgs.data_ptr<uint8_t>(), moff.data_ptr<int64_t>(),
                              g2_lines.data_ptr<uint8_t>(), N, ok.data_ptr<int32_t>(),
                              cur_stream());
    }
    return ok;
}

torch::Tensor bls_verify_batch_wave(torch::Tensor vks, torch::Tensor sigs,
                                    torch::Tensor msgs, torch::Tensor moff,
                                    torch::Tensor g2_lines, torch::Tensor rand_r) {
    CHECK_DEV(vks); CHECK_DEV(sigs); CHECK_DEV(msgs); CHECK_DEV(moff); CHECK_DEV(g2_lines);
    CHECK_DEV(rand_r);
    CHECK_CONTIG(vks); CHECK_CONTIG(sigs); CHECK_CONTIG(msgs); CHECK_CONTIG(moff);
    CHECK_CONTIG(g2_lines); CHECK_CONTIG(rand_r);
    int32_t N = (int32_t)moff.size(0) - 1;
    TORCH_CHECK(vks.numel() == (int64_t)N * 128 && sigs.numel() == (int64_t)N * 64);
    TORCH_CHECK(rand_r.numel() >= N && rand_r.dtype() == torch::kInt64);
    auto ok = torch::zeros({N}, opts(torch::kInt32, vks));
    if (N > 0) {
        launch_k1_bls_verify_wave(vks.data_ptr<uint8_t>(), sigs.data_ptr<uint8_t>(),
                                  msgs.data_ptr<uint8_t>(), moff.data_ptr<int64_t>(),
                                  g2_lines.data_ptr<uint8_t>(),
                                  (const uint64_t*)rand_r.data_ptr<int64_t>(), N,
                                  ok.data_ptr<int32_t>(), cur_stream());
    }
    return ok;
}

torch::Tensor hash_to_g1_batch(torch::Tensor msgs, torch::Tensor moff) {
    CHECK_DEV(msgs); CHECK_DEV(moff);
    int32_t N = (int32_t)moff.size(0) - 1;
    auto out = torch::zeros({N, 64}, opts(torch::kUInt8, msgs));
    if (N > 0) {
        launch_k1_hash_to_g1(msgs.data_ptr<uint8_t>(), moff.data_ptr<int64_t>(), N,
                             out.data_ptr<uint8_t>(), cur_stream());
    }
    return out;
}

void fanout_wave(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                 torch::Tensor pairs,
                 torch::Tensor msg_seq, torch::Tensor n_pairs, torch::Tensor egress,
                 int64_t nt, int64_t grid) {
    CHECK_DEV(egress); CHECK_CONTIG(egress);
    launch_k3_fanout_wave(buf.data_ptr<uint8_t>(), payload_off.data_ptr<int64_t>(),
                          payload_len.data_ptr<int32_t>(), pair_ptr(pairs),
                          (const uint32_t*)msg_seq.data_ptr<int32_t>(),
                          n_pairs.data_ptr<int32_t>(), (int32_t)pairs.size(0),
                          egress.data_ptr<uint8_t>(), (int)nt,
                          (int)grid, cur_stream());
}

void fanout_ref(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                torch::Tensor pairs,
                torch::Tensor msg_seq, torch::Tensor n_pairs, torch::Tensor egress,
                int64_t nt, int64_t grid, int64_t ref_threshold, int64_t ref_base) {
    CHECK_DEV(egress); CHECK_CONTIG(egress);
    TORCH_CHECK(ref_threshold >= 0 && ref_threshold <= INT32_MAX,
                "ref_threshold must fit an int32 length");
    TORCH_CHECK(ref_base >= 0, "ref_base must not be negative");
    launch_k3_fanout_ref(buf.data_ptr<uint8_t>(), payload_off.data_ptr<int64_t>(),
                         payload_len.data_ptr<int32_t>(), pair_ptr(pairs),
                         (const uint32_t*)msg_seq.data_ptr<int32_t>(),
                         n_pairs.data_ptr<int32_t>(), (int32_t)pairs.size(0),
                         (int32_t)ref_threshold, ref_base,
                         egress.data_ptr<uint8_t>(), (int)nt,
                         (int)grid, cur_stream());
}

void fanout_flat2(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                  torch::Tensor pairs,
                  int64_t seq_base, torch::Tensor n_pairs, int64_t units_per_pair,
                  torch::Tensor egress, int64_t nt, int64_t grid, int64_t uniform_len) {
    CHECK_DEV(egress); CHECK_CONTIG(egress);
    pair_ptr(pairs);
    check_flat_shape(pairs, units_per_pair);
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k3_fanout_flat2(buf.data_ptr<uint8_t>(), payload_off.data_ptr<int64_t>(),
                           payload_len.data_ptr<int32_t>(), pair_ptr(pairs),
                           (uint32_t)seq_base, n_pairs.data_ptr<int32_t>(), capacity,
                           (int32_t)units_per_pair, (int32_t)uniform_len,
                           egress.data_ptr<uint8_t>(), (int)nt, (int)grid, cur_stream());
}

void fanout_flat3(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                  torch::Tensor pairs,
                  torch::Tensor seq_state, torch::Tensor n_pairs, int64_t units_per_pair,
                  torch::Tensor egress, int64_t nt, int64_t grid, int64_t uniform_len) {
    CHECK_DEV(egress); CHECK_CONTIG(egress);
    pair_ptr(pairs);
    check_flat_shape(pairs, units_per_pair);
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k3_fanout_flat3(buf.data_ptr<uint8_t>(), payload_off.data_ptr<int64_t>(),
                           payload_len.data_ptr<int32_t>(), pair_ptr(pairs),
                           (const uint32_t*)seq_state.data_ptr<int32_t>(),
                           n_pairs.data_ptr<int32_t>(), capacity, (int32_t)units_per_pair,
                           (int32_t)uniform_len, egress.data_ptr<uint8_t>(), (int)nt,
                           (int)grid, cur_stream());
}

void seq_advance(torch::Tensor seq_state, int64_t m) {
    launch_k_seq_advance((uint32_t*)seq_state.data_ptr<int32_t>(), (int32_t)m, cur_stream());
}

torch::Tensor topic_mask_t(torch::Tensor sub_bitmap, torch::Tensor buf,
                           torch::Tensor topics_off, torch::Tensor topics_cnt,
                           torch::Tensor disc) {
    CHECK_DEV(sub_bitmap); CHECK_CONTIG(sub_bitmap);
    return k2a_mask(sub_bitmap, buf, disc, true, [&](uint64_t* mask_t, int32_t M, int32_t W) {
        launch_k2a_topic_mask_t((const uint64_t*)sub_bitmap.data_ptr<int64_t>(),
                                buf.data_ptr<uint8_t>(), topics_off.data_ptr<int64_t>(),
                                topics_cnt.data_ptr<int32_t>(), disc.data_ptr<int32_t>(),
                                mask_t, M, W, cur_stream());
    });
}

void assign_emit_fused_t(torch::Tensor mask_t, torch::Tensor payload_len,
                         torch::Tensor ring_wpos, int64_t ring_bytes, int64_t n_users,
                         torch::Tensor pairs, torch::Tensor drops, torch::Tensor n_pairs,
                         int64_t uniform_rec) {
    CHECK_DEV(mask_t); CHECK_CONTIG(mask_t);
    int32_t W = (int32_t)mask_t.size(0);
    int32_t M = (int32_t)mask_t.size(1);
    TORCH_CHECK(ring_bytes % 16 == 0);
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k2b_fused_t((const uint64_t*)mask_t.data_ptr<int64_t>(),
                       payload_len.data_ptr<int32_t>(), M, W, (int32_t)n_users, ring_bytes,
                       capacity, (int32_t)uniform_rec,
                       (uint64_t*)ring_wpos.data_ptr<int64_t>(),
                       n_pairs.data_ptr<int32_t>(), pair_ptr(pairs),
                       (uint32_t*)drops.data_ptr<int32_t>(), cur_stream());
}

void assign_emit_blocks_t(torch::Tensor mask_t, torch::Tensor ring_wpos,
                          int64_t ring_bytes, int64_t n_users,
                          torch::Tensor bcount, torch::Tensor pprefix, torch::Tensor ubase,
                          torch::Tensor ufit, torch::Tensor udst,
                          torch::Tensor pairs, torch::Tensor drops, torch::Tensor n_pairs,
                          int64_t uniform_rec) {
    CHECK_DEV(mask_t); CHECK_CONTIG(mask_t);
    int32_t W = (int32_t)mask_t.size(0);
    int32_t M = (int32_t)mask_t.size(1);
    TORCH_CHECK(ring_bytes % 16 == 0 && uniform_rec > 0);
    int64_t NB = (M + 31) / 32;
    TORCH_CHECK(bcount.numel() >= NB * W * 64 && pprefix.numel() >= NB * W * 64,
                "k2b block scratch too small");
    TORCH_CHECK(ubase.numel() >= W * 64 && ufit.numel() >= W * 64 && udst.numel() >= W * 64);
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k2b_blocks_t((const uint64_t*)mask_t.data_ptr<int64_t>(), M, W, (int32_t)n_users,
                        ring_bytes, capacity, (int32_t)uniform_rec,
                        (uint64_t*)ring_wpos.data_ptr<int64_t>(),
                        n_pairs.data_ptr<int32_t>(),
                        bcount.data_ptr<int32_t>(), pprefix.data_ptr<int32_t>(),
                        ubase.data_ptr<int32_t>(), ufit.data_ptr<int32_t>(),
                        udst.data_ptr<int64_t>(),
                        pair_ptr(pairs),
                        (uint32_t*)drops.data_ptr<int32_t>(), cur_stream());
}

void emit_direct(torch::Tensor disc, torch::Tensor owner, torch::Tensor payload_off,
                 torch::Tensor payload_len, int64_t ring_bytes, torch::Tensor ring_wpos,
                 torch::Tensor n_pairs, torch::Tensor pairs, torch::Tensor drops) {
    int32_t M = (int32_t)disc.size(0);
    if (M == 0) return;
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k5b_emit_direct(disc.data_ptr<int32_t>(), owner.data_ptr<int32_t>(),
                           payload_off.data_ptr<int64_t>(), payload_len.data_ptr<int32_t>(),
                           M, ring_bytes, capacity, (uint64_t*)ring_wpos.data_ptr<int64_t>(),
                           n_pairs.data_ptr<int32_t>(), pair_ptr(pairs),
                           (uint32_t*)drops.data_ptr<int32_t>(), cur_stream());
}

torch::Tensor topic_mask_origin_t(torch::Tensor sub_bitmap, torch::Tensor buf,
                                  torch::Tensor topics_off, torch::Tensor topics_cnt,
                                  torch::Tensor disc, torch::Tensor origin, int64_t n_users) {
    CHECK_DEV(sub_bitmap); CHECK_CONTIG(sub_bitmap); CHECK_DEV(origin); CHECK_CONTIG(origin);
    TORCH_CHECK(origin.dtype() == torch::kInt32 && origin.numel() == disc.size(0),
                "origin must be an int32 [M] tensor");
    TORCH_CHECK(n_users >= 0 && n_users <= sub_bitmap.size(1) * 64, "n_users outside the bitmap");
    return k2a_mask(sub_bitmap, buf, disc, true, [&](uint64_t* mask_t, int32_t M, int32_t W) {
        launch_k2a_topic_mask_origin_t(
            (const uint64_t*)sub_bitmap.data_ptr<int64_t>(), buf.data_ptr<uint8_t>(),
            topics_off.data_ptr<int64_t>(), topics_cnt.data_ptr<int32_t>(),
            disc.data_ptr<int32_t>(), origin.data_ptr<int32_t>(), mask_t, M, W,
            (int32_t)n_users, cur_stream());
    });
}

void emit_direct_peers(torch::Tensor disc, torch::Tensor owner, torch::Tensor origin,
                       torch::Tensor payload_off, torch::Tensor payload_len,
                       int64_t ring_bytes, int64_t n_users, int64_t n_peers,
                       torch::Tensor ring_wpos, torch::Tensor n_pairs, torch::Tensor pairs,
                       torch::Tensor drops) {
    int32_t M = (int32_t)disc.size(0);
    if (M == 0) return;
    CHECK_DEV(origin); CHECK_CONTIG(origin); CHECK_DEV(ring_wpos); CHECK_CONTIG(ring_wpos);
    TORCH_CHECK(origin.dtype() == torch::kInt32 && origin.numel() == M,
                "origin must be an int32 [M] tensor");
    TORCH_CHECK(owner.numel() == M && payload_len.numel() == M);
    TORCH_CHECK(n_users >= 0 && n_peers >= 0 && ring_wpos.numel() >= n_users + n_peers,
                "ring_wpos must cover n_users + n_peers rings");
    int32_t capacity = (int32_t)pairs.size(0);
    launch_k5b_emit_direct_peers(
        disc.data_ptr<int32_t>(), owner.data_ptr<int32_t>(), origin.data_ptr<int32_t>(),
        payload_off.data_ptr<int64_t>(), payload_len.data_ptr<int32_t>(), M,
        (int32_t)n_users, (int32_t)n_peers, ring_bytes, capacity,
        (uint64_t*)ring_wpos.data_ptr<int64_t>(), n_pairs.data_ptr<int32_t>(),
        pair_ptr(pairs), (uint32_t*)drops.data_ptr<int32_t>(), cur_stream());
}

void direct_apply(torch::Tensor table_keys, torch::Tensor table_vals, torch::Tensor up_keys,
                  torch::Tensor up_owners, torch::Tensor del_keys, torch::Tensor n_failed) {
    CHECK_DEV(table_keys); CHECK_DEV(table_vals); CHECK_DEV(up_keys); CHECK_DEV(up_owners);
    CHECK_DEV(del_keys); CHECK_DEV(n_failed);
    CHECK_CONTIG(table_keys); CHECK_CONTIG(table_vals); CHECK_CONTIG(up_keys);
    CHECK_CONTIG(up_owners); CHECK_CONTIG(del_keys);
    int64_t S = table_keys.size(0);
    TORCH_CHECK(S > 0 && (S & (S - 1)) == 0, "table size must be a power of two");
    TORCH_CHECK(table_vals.numel() == S && table_keys.dtype() == torch::kInt64
                && table_vals.dtype() == torch::kInt32);
    TORCH_CHECK(up_keys.dtype() == torch::kInt64 && del_keys.dtype() == torch::kInt64
                && up_owners.dtype() == torch::kInt32 && n_failed.dtype() == torch::kInt32);
    TORCH_CHECK(up_owners.numel() == up_keys.numel() && n_failed.numel() >= 1);
    launch_k6_direct_apply((uint64_t*)table_keys.data_ptr<int64_t>(),
                           table_vals.data_ptr<int32_t>(), S,
                           (const uint64_t*)up_keys.data_ptr<int64_t>(),
                           up_owners.data_ptr<int32_t>(), (int32_t)up_keys.numel(),
                           (const uint64_t*)del_keys.data_ptr<int64_t>(),
                           (int32_t)del_keys.numel(),
                           (uint32_t*)n_failed.data_ptr<int32_t>(), cur_stream());
}

// The fused uniform broadcast tick (launch_tick_uniform_broadcast): one call
// per tick, no allocation and no synchronisation.  scratch64 / scratch32 are
// engine-owned and at least uniform_tick_scratch_sizes(M, W, rec) long.
void tick_uniform_broadcast(torch::Tensor buf, torch::Tensor offsets, uint64_t hash_seed,
                            torch::Tensor sub_bitmap, torch::Tensor ring_wpos,
                            int64_t ring_bytes, int64_t n_users, torch::Tensor pairs,
                            torch::Tensor drops, torch::Tensor n_pairs, torch::Tensor n_sparse,
                            torch::Tensor scratch64, torch::Tensor scratch32,
                            int64_t uniform_len, int64_t seq_base, torch::Tensor egress,
                            int64_t nt, int64_t dense) {
    CHECK_DEV(buf); CHECK_CONTIG(buf); CHECK_DEV(offsets); CHECK_CONTIG(offsets);
    CHECK_DEV(sub_bitmap); CHECK_CONTIG(sub_bitmap); CHECK_DEV(ring_wpos); CHECK_CONTIG(ring_wpos);
    CHECK_DEV(egress); CHECK_CONTIG(egress); CHECK_DEV(scratch64); CHECK_DEV(scratch32);
    CHECK_DEV(drops); CHECK_DEV(n_pairs); CHECK_DEV(n_sparse);
    TORCH_CHECK(buf.dtype() == torch::kUInt8 && offsets.dtype() == torch::kInt64
                && egress.dtype() == torch::kUInt8);
    TORCH_CHECK(sub_bitmap.dim() == 2 && sub_bitmap.size(0) == 256);
    const int64_t M = offsets.size(0) - 1, W = sub_bitmap.size(1);
    if (M <= 0) return;
    TORCH_CHECK(uniform_len >= 0 && uniform_len < (int64_t(1) << 30));
    const int64_t rec = (uniform_len + 16 + 15) & ~int64_t(15);
    TORCH_CHECK(ring_bytes % 16 == 0 && n_users >= 0 && n_users <= W * 64
                && ring_wpos.numel() >= n_users && ring_wpos.dtype() == torch::kInt64
                && egress.numel() >= n_users * ring_bytes,
                "rings do not cover n_users");
    TORCH_CHECK(buf.numel() >= M * uniform_len, "batch shorter than M uniform messages");
    check_flat_shape(pairs, rec / 16);
    // the image kernel's unit index and the dense fan-out's 1-D grid
    TORCH_CHECK(M * (rec / 16) < (int64_t(1) << 31)
                && dense_grid_x((int32_t)n_users, DENSE_GROUP, dense_geom((int32_t)(rec / 16)).n_chunks)
                       * k2b_blocks(M) < (int64_t(1) << 31),
                "batch too large for the dense fan-out");
    TORCH_CHECK(scratch64.dtype() == torch::kInt64 && scratch32.dtype() == torch::kInt32
                && scratch64.is_contiguous() && scratch32.is_contiguous()
                && (uintptr_t)scratch64.data_ptr<int64_t>() % 16 == 0
                && scratch64.numel() >= uniform_tick_scratch64(M, W, rec / 16)
                && scratch32.numel() >= uniform_tick_scratch32(M, W),
                "fused tick scratch too small");
    UniformTick t;
    t.buf = buf.data_ptr<uint8_t>();
    t.offsets = offsets.data_ptr<int64_t>();
    t.M = (int32_t)M;
    t.hash_seed = hash_seed;
    t.sub_bitmap = (const uint64_t*)sub_bitmap.data_ptr<int64_t>();
    t.W = (int32_t)W;
    t.n_users = (int32_t)n_users;
    t.ring_bytes = ring_bytes;
    t.capacity = (int32_t)pairs.size(0);
    t.uniform_len = (int32_t)uniform_len;
    t.rec = (int32_t)rec;
    t.seq_base = (uint32_t)seq_base;
    t.ring_wpos = (uint64_t*)ring_wpos.data_ptr<int64_t>();
    t.n_pairs = n_pairs.data_ptr<int32_t>();
    t.n_sparse = n_sparse.data_ptr<int32_t>();
    t.pairs = pair_ptr(pairs);
    t.drops = (uint32_t*)drops.data_ptr<int32_t>();
    t.scratch64 = scratch64.data_ptr<int64_t>();
    t.scratch32 = scratch32.data_ptr<int32_t>();
    t.egress = egress.data_ptr<uint8_t>();
    t.nt = (int)nt;
    t.dense = (int)dense;
    launch_tick_uniform_broadcast(&t, cur_stream());
}

std::vector<int64_t> uniform_tick_scratch_sizes(int64_t M, int64_t W, int64_t rec) {
    return {uniform_tick_scratch64(M, W, rec / 16), uniform_tick_scratch32(M, W)};
}

// Fused drain: one kernel copies the cursors to `staging` and zeroes them,
// one async copy lands them in the engine's pinned `host` buffer, one stream
// synchronise makes that buffer readable.
void drain_cursors(torch::Tensor ring_wpos, torch::Tensor staging, torch::Tensor host) {
    CHECK_DEV(ring_wpos); CHECK_CONTIG(ring_wpos); CHECK_DEV(staging); CHECK_CONTIG(staging);
    TORCH_CHECK(!host.is_cuda() && host.is_pinned() && host.is_contiguous(),
                "host must be a pinned CPU tensor");
    TORCH_CHECK(ring_wpos.dtype() == torch::kInt64 && staging.dtype() == torch::kInt64
                && host.dtype() == torch::kInt64);
    const int64_t n = ring_wpos.numel();
    TORCH_CHECK(staging.numel() >= n && host.numel() >= n && n <= INT32_MAX);
    if (n == 0) return;
    hipStream_t s = cur_stream();
    launch_drain_cursors(ring_wpos.data_ptr<int64_t>(), staging.data_ptr<int64_t>(), (int32_t)n,
                         s);
    hipError_t e = hipMemcpyAsync(host.data_ptr<int64_t>(), staging.data_ptr<int64_t>(),
                                  (size_t)n * 8, hipMemcpyDeviceToHost, s);
    TORCH_CHECK(e == hipSuccess, "drain_cursors copy: ", hipGetErrorString(e));
    e = hipStreamSynchronize(s);
    TORCH_CHECK(e == hipSuccess, "drain_cursors sync: ", hipGetErrorString(e));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("tick_uniform_broadcast", &tick_uniform_broadcast,
          "fused uniform broadcast tick: K4, K2a, K2b tiles, dense + sparse fan-out");
    m.def("uniform_tick_scratch_sizes", &uniform_tick_scratch_sizes,
          "(int64, int32) scratch elements tick_uniform_broadcast needs for (M, W, rec)");
    m.def("drain_cursors", &drain_cursors,
          "fused drain: cursors -> pinned host buffer, cursors zeroed, stream synchronised",
          py::call_guard<py::gil_scoped_release>());
    m.def("topic_mask_origin_t", &topic_mask_origin_t,
          "K2a transposed with per-message origin: remote-origin rows keep user bits only");
    m.def("emit_direct_peers", &emit_direct_peers,
          "K5b with peer recipient slots (owner -(p+2) -> ring n_users+p, local origin only)");
    m.def("direct_apply", &direct_apply,
          "K6: batched DirectMap upserts/deletes on the device table");
    m.def("parse_batch", &parse_batch, "K4: on-device capnp parse of a message batch",
          py::arg("buf"), py::arg("offsets"), py::arg("hash_seed") = 0);
    m.def("topic_mask", &topic_mask, "K2a: per-message subscriber mask");
    m.def("assign_emit", &assign_emit, "K2b: per-user FIFO ring assignment + pair list");
    m.def("fanout", &fanout, "K3: N-way payload fan-out into egress rings");
    m.def("direct_lookup", &direct_lookup, "K5: batched direct-route hash probe");
    m.def("apply_subs", &apply_subs, "K2c: apply subscribe/unsubscribe batch to bitmap");
    m.def("bls_verify_batch", &bls_verify_batch, "K1: batched BLS-over-BN254 verification");
    m.def("compact_rings", &compact_rings,
          "K7: gather used egress-ring prefixes into one staging buffer");
    m.def("precompute_g2_lines", &precompute_g2_lines,
          "fixed-g2 Miller line coefficients for K1 v2 (once per process)");
    m.def("bls_verify_batch2", &bls_verify_batch2,
          "K1 v2: 2-lane Fp2-decomposed batched BLS verification");
    m.def("_k1_dbg_wave",
          [](torch::Tensor vks, torch::Tensor sigs, torch::Tensor msgs, torch::Tensor moff,
             torch::Tensor g2_lines, torch::Tensor rand_r, int64_t mode) {
              int32_t N = (int32_t)moff.size(0) - 1;
              auto ok = torch::zeros({N}, opts(torch::kInt32, vks));
              launch_k1_dbg_wave(vks.data_ptr<uint8_t>(), sigs.data_ptr<uint8_t>(),
                                 msgs.data_ptr<uint8_t>(), moff.data_ptr<int64_t>(),
                                 g2_lines.data_ptr<uint8_t>(),
                                 (const uint64_t*)rand_r.data_ptr<int64_t>(), N,
                                 (int32_t)mode, ok.data_ptr<int32_t>(), cur_stream());
              return ok;
          });
    m.def("bls_verify_batch_wave", &bls_verify_batch_wave,
          "K1 v3: wave-batched product verification (shared final exp, "
          "exact per-item fallback)");
    m.def("hash_to_g1_batch", &hash_to_g1_batch, "K1 helper: batched hash-to-G1");
    m.def("fanout_wave", &fanout_wave, "K3v2: wave-per-pair fan-out (nt flag, device count)");
    m.def("fanout_ref", &fanout_ref,
          "K3r: fan-out with by-reference records at or above ref_threshold");
    m.def("fanout_flat2", &fanout_flat2, "K3v4: flat fan-out, seq from base, capacity clamp");
    m.def("fanout_flat3", &fanout_flat3, "K3v5: graph-capturable (device seq counter)");
    m.def("seq_advance", &seq_advance, "bump the device seq counter (inside the graph)");
    m.def("topic_mask_t", &topic_mask_t, "K2a transposed: mask[W][M]");
    m.def("emit_direct", &emit_direct,
          "K5b: on-device direct-delivery pair emission (no host sync)");
    m.def("assign_emit_fused_t", &assign_emit_fused_t,
          "K2b fused on transposed mask (wave-aggregated claims, uniform-rec fast path)");
    m.def("assign_emit_blocks_t", &assign_emit_blocks_t,
          "K2b block-parallel (P1 count / P2 bases / P3 emit) for uniform records");
}
