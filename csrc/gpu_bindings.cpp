// Torch extension bindings for the MI355X broker data-plane kernels
// (csrc/hip/dataplane.hip). PyTorch owns every HBM buffer; these calls
// invoke the extern "C" launchers defined next to the kernels and declared
// in csrc/hip/dataplane.h and csrc/hip/bls_kernels.h.
//
// This file is the native boundary: the only place where a Python tensor
// becomes a raw pointer.  Every op below is an `Op` (the checks, in
// csrc/binding_checks.h), a list of (tensor, element type, length) reads
// through Op::ptr, and one launch.

#include "binding_checks.h"
#include "hip/bls_kernels.h"
#include "hip/dataplane.h"

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
    Op a("parse_batch");
    const uint8_t* b = a.ptr<uint8_t>(buf, "buf");
    const int64_t* off = a.ptr<int64_t>(offsets, "offsets", 1);
    const int32_t M = a.i32(offsets.numel() - 1, "M");
    hipStream_t s = a.begin();
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
        ParseOut out{a.ptr<int32_t>(disc, "disc"), a.ptr<int64_t>(payload_off, "payload_off"),
                     a.ptr<int32_t>(payload_len, "payload_len"),
                     a.ptr<int64_t>(topics_off, "topics_off"),
                     a.ptr<int32_t>(topics_cnt, "topics_cnt"),
                     a.ptr<uint64_t>(recip_hash, "recip_hash"),
                     a.ptr<uint64_t>(timestamp, "timestamp")};
        launch_k4_parse(b, off, M, hash_seed, out, s);
        a.launched();
    }
    return {disc, payload_off, payload_len, topics_off, topics_cnt, recip_hash, timestamp};
}

// What the K2a ops and K2c share: the [256][W] bitmap, the batch and the
// three per-message columns parse_batch made.  M is disc's length.
struct TopicArgs {
    uint64_t* sub_bitmap;
    const uint8_t* buf;
    const int64_t* topics_off;
    const int32_t* topics_cnt;
    const int32_t* disc;
    int32_t M, W;
};

static TopicArgs topic_args(Op& a, const torch::Tensor& sub_bitmap, const torch::Tensor& buf,
                            const torch::Tensor& topics_off, const torch::Tensor& topics_cnt,
                            const torch::Tensor& disc) {
    TopicArgs t;
    t.sub_bitmap = a.ptr<uint64_t>(sub_bitmap, "sub_bitmap", 0, mat(256, -1));
    t.buf = a.ptr<uint8_t>(buf, "buf");
    t.disc = a.ptr<int32_t>(disc, "disc");
    t.topics_off = a.same<int64_t>(topics_off, "topics_off", disc.numel(), "one per disc");
    t.topics_cnt = a.same<int32_t>(topics_cnt, "topics_cnt", disc.numel(), "one per disc");
    t.M = a.i32(disc.numel(), "M");
    t.W = a.i32(sub_bitmap.size(1), "W");
    return t;
}

torch::Tensor topic_mask(torch::Tensor sub_bitmap, torch::Tensor buf, torch::Tensor topics_off,
                         torch::Tensor topics_cnt, torch::Tensor disc) {
    Op a("topic_mask");
    const TopicArgs t = topic_args(a, sub_bitmap, buf, topics_off, topics_cnt, disc);
    hipStream_t s = a.begin();
    auto mask = torch::empty({t.M, t.W}, opts(torch::kInt64, buf));
    if (t.M > 0) {
        launch_k2a_topic_mask(t.sub_bitmap, t.buf, t.topics_off, t.topics_cnt, t.disc,
                              a.ptr<uint64_t>(mask, "mask"), t.M, t.W, s);
        a.launched();
    }
    return mask;
}

std::vector<torch::Tensor> assign_emit(torch::Tensor mask, torch::Tensor payload_off,
                                       torch::Tensor payload_len, torch::Tensor ring_wpos,
                                       int64_t ring_bytes, int64_t n_users) {
    Op a("assign_emit");
    const uint64_t* mk = a.ptr<uint64_t>(mask, "mask", 0, mat());
    const int32_t M = a.i32(mask.size(0), "M");
    const int32_t W = a.i32(mask.size(1), "W");
    // n = 0 would read cum[-1] below
    const int32_t n = a.i32(n_users, "n_users", 1, int64_t(W) * 64);
    a.ring_bytes(ring_bytes);
    const int64_t* poff = a.ptr<int64_t>(payload_off, "payload_off", M);
    const int32_t* plen = a.ptr<int32_t>(payload_len, "payload_len", M);
    uint64_t* wpos = a.ptr<uint64_t>(ring_wpos, "ring_wpos", n);
    hipStream_t s = a.begin();
    auto o32 = opts(torch::kInt32, mask);
    auto counts = torch::zeros({n}, o32);
    launch_k2b_count(mk, M, W, n, a.ptr<int32_t>(counts, "counts"), s);
    a.launched();
    auto cum = counts.cumsum(0).to(torch::kInt32);
    auto pair_base = (cum - counts).contiguous();  // exclusive scan
    int64_t total = cum[n - 1].item<int32_t>();  // one small D2H sync
    auto pairs = torch::empty({total, 4}, o32);
    auto drops = torch::zeros({1}, o32);
    launch_k2b_emit(mk, poff, plen, a.ptr<int32_t>(pair_base, "pair_base"), M, W, n, ring_bytes,
                    wpos, a.pairs(pairs), a.ptr<uint32_t>(drops, "drops"), s);
    a.launched();
    // split the AoS records back into the golden-test API's three tensors
    auto pair_user = pairs.select(1, 0).contiguous();
    auto pair_msg = pairs.select(1, 1).contiguous();
    auto pair_dst = pairs.slice(1, 2, 4).contiguous().view(torch::kInt64).squeeze(1);
    return {pair_user, pair_msg, pair_dst, drops};
}

void fanout(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
            torch::Tensor pair_user, torch::Tensor pair_msg, torch::Tensor pair_dst,
            torch::Tensor msg_seq, torch::Tensor egress) {
    Op a("fanout");
    const uint8_t* b = a.ptr<uint8_t>(buf, "buf");
    const int64_t L = payload_off.numel();
    const int64_t* poff = a.ptr<int64_t>(payload_off, "payload_off");
    const int32_t* plen = a.same<int32_t>(payload_len, "payload_len", L, "one per payload_off");
    const int32_t n_pairs = a.i32(pair_user.numel(), "pair count");
    a.ptr<int32_t>(pair_user, "pair_user");
    a.same<int32_t>(pair_msg, "pair_msg", n_pairs, "one per pair_user");
    a.same<int64_t>(pair_dst, "pair_dst", n_pairs, "one per pair_user");
    const uint32_t* seq = a.same<uint32_t>(msg_seq, "msg_seq", L, "one per payload_off");
    uint8_t* eg = a.ptr<uint8_t>(egress, "egress");
    hipStream_t s = a.begin();
    if (n_pairs == 0) return;
    auto pairs = torch::empty({n_pairs, 4}, opts(torch::kInt32, buf));
    pairs.select(1, 0).copy_(pair_user);
    pairs.select(1, 1).copy_(pair_msg);
    pairs.slice(1, 2, 4).view(torch::kInt64).squeeze(1).copy_(pair_dst);
    launch_k3_fanout(b, poff, plen, a.pairs(pairs), seq, n_pairs, eg, s);
    a.launched();
}

torch::Tensor direct_lookup(torch::Tensor table_keys, torch::Tensor table_vals,
                            torch::Tensor query) {
    Op a("direct_lookup");
    const uint64_t* keys = a.ptr<uint64_t>(table_keys, "table_keys", 1, vec());
    const int64_t S = table_keys.numel();
    TORCH_CHECK((S & (S - 1)) == 0, a.name(), ": table_keys must have a power-of-two length, got ",
                S);
    const int32_t* vals = a.same<int32_t>(table_vals, "table_vals", S, "one per table_keys", vec());
    const uint64_t* q = a.ptr<uint64_t>(query, "query");
    const int32_t N = a.i32(query.numel(), "N");
    hipStream_t s = a.begin();
    auto owner = torch::empty({N}, opts(torch::kInt32, query));
    if (N > 0) {
        launch_k5_direct_lookup(keys, vals, S, q, N, a.ptr<int32_t>(owner, "owner"), s);
        a.launched();
    }
    return owner;
}

void apply_subs(torch::Tensor sub_bitmap, torch::Tensor buf, torch::Tensor topics_off,
                torch::Tensor topics_cnt, torch::Tensor disc, torch::Tensor user_idx) {
    Op a("apply_subs");
    const TopicArgs t = topic_args(a, sub_bitmap, buf, topics_off, topics_cnt, disc);
    const int32_t* uidx = a.same<int32_t>(user_idx, "user_idx", t.M, "one per disc");
    hipStream_t s = a.begin();
    if (t.M == 0) return;
    launch_k2c_apply_subs(t.sub_bitmap, t.buf, t.topics_off, t.topics_cnt, t.disc, uidx, t.M,
                          t.W, s);
    a.launched();
}

// What the K1 ops share: N items = moff's length - 1, vks [N][128], sigs
// [N][64], the flat messages; g2_lines and rand_r where the op takes them.
// An op that takes no vks / sigs / g2_lines / rand_r passes nullptr.
struct K1Args {
    const uint8_t* vks = nullptr;
    const uint8_t* sigs = nullptr;
    uint8_t* msgs;
    const int64_t* moff;
    const uint8_t* g2_lines = nullptr;
    const uint64_t* rand_r = nullptr;
    int32_t N;
};

static K1Args k1_args(Op& a, const torch::Tensor* vks, const torch::Tensor* sigs,
                      const torch::Tensor& msgs, const torch::Tensor& moff,
                      const torch::Tensor* g2_lines = nullptr,
                      const torch::Tensor* rand_r = nullptr) {
    K1Args k;
    const int64_t N = moff.numel() - 1;
    if (vks) k.vks = a.same<uint8_t>(*vks, "vks", N * 128, "128 per interval of moff");
    if (sigs) k.sigs = a.same<uint8_t>(*sigs, "sigs", N * 64, "64 per interval of moff");
    k.msgs = a.ptr<uint8_t>(msgs, "msgs");
    k.moff = a.ptr<int64_t>(moff, "moff", 1, vec());
    if (g2_lines) k.g2_lines = a.ptr<uint8_t>(*g2_lines, "g2_lines", 128 * 192);
    if (rand_r) k.rand_r = a.ptr<uint64_t>(*rand_r, "rand_r", N);
    k.N = a.i32(N, "N");
    return k;
}

torch::Tensor bls_verify_batch(torch::Tensor vks, torch::Tensor sigs, torch::Tensor msgs,
                               torch::Tensor moff) {
    Op a("bls_verify_batch");
    const K1Args k = k1_args(a, &vks, &sigs, msgs, moff);
    hipStream_t s = a.begin();
    auto ok = torch::zeros({k.N}, opts(torch::kInt32, vks));
    if (k.N > 0) {
        launch_k1_bls_verify(k.vks, k.sigs, k.msgs, k.moff, k.N, a.ptr<int32_t>(ok, "ok"), s);
        a.launched();
    }
    return ok;
}

void compact_rings(torch::Tensor egress, int64_t ring_bytes, torch::Tensor wpos,
                   torch::Tensor dst_off, torch::Tensor staging, int64_t max_chunks) {
    Op a("compact_rings");
    const int32_t n = a.i32(wpos.numel(), "ring count");
    const int32_t chunks = a.i32(max_chunks, "max_chunks");
    TORCH_CHECK(ring_bytes >= 0, a.name(), ": ring_bytes = ", ring_bytes, " is negative");
    const uint8_t* eg = a.ptr<uint8_t>(egress, "egress", n * ring_bytes);
    const int64_t* wp = a.ptr<int64_t>(wpos, "wpos", 0, vec());
    const int64_t* doff = a.ptr<int64_t>(dst_off, "dst_off", n);
    uint8_t* st = a.ptr<uint8_t>(staging, "staging");
    hipStream_t s = a.begin();
    if (n == 0 || chunks == 0) return;
    launch_k7_compact_rings(eg, ring_bytes, wp, doff, st, n, chunks, s);
    a.launched();
}

torch::Tensor precompute_g2_lines(torch::Tensor device_probe) {
    // fixed-g2 Miller-loop line coefficients (128 records x 192 B); computed
    // once per process by a 1-thread kernel, consumed by bls_verify_batch2
    Op a("precompute_g2_lines");
    a.ptr<uint8_t>(device_probe, "device_probe");
    hipStream_t s = a.begin();
    auto out = torch::zeros({128 * 192}, opts(torch::kUInt8, device_probe));
    auto n = torch::zeros({1}, opts(torch::kInt32, device_probe));
    launch_k1_precompute_g2_lines(a.ptr<uint8_t>(out, "out"), a.ptr<int32_t>(n, "n"), s);
    a.launched();
    return out;
}

torch::Tensor bls_verify_batch2(torch::Tensor vks, torch::Tensor sigs, torch::Tensor msgs,
                                torch::Tensor moff, torch::Tensor g2_lines) {
    Op a("bls_verify_batch2");
    const K1Args k = k1_args(a, &vks, &sigs, msgs, moff, &g2_lines);
    hipStream_t s = a.begin();
    auto ok = torch::zeros({k.N}, opts(torch::kInt32, vks));
    if (k.N > 0) {
        launch_k1_bls_verify2(k.vks, k.sigs, k.msgs, k.moff, k.g2_lines, k.N,
                              a.ptr<int32_t>(ok, "ok"), s);
        a.launched();
    }
    return ok;
}

torch::Tensor bls_verify_batch_wave(torch::Tensor vks, torch::Tensor sigs,
                                    torch::Tensor msgs, torch::Tensor moff,
                                    torch::Tensor g2_lines, torch::Tensor rand_r) {
    Op a("bls_verify_batch_wave");
    const K1Args k = k1_args(a, &vks, &sigs, msgs, moff, &g2_lines, &rand_r);
    hipStream_t s = a.begin();
    auto ok = torch::zeros({k.N}, opts(torch::kInt32, vks));
    if (k.N > 0) {
        launch_k1_bls_verify_wave(k.vks, k.sigs, k.msgs, k.moff, k.g2_lines, k.rand_r, k.N,
                                  a.ptr<int32_t>(ok, "ok"), s);
        a.launched();
    }
    return ok;
}

torch::Tensor hash_to_g1_batch(torch::Tensor msgs, torch::Tensor moff) {
    Op a("hash_to_g1_batch");
    const K1Args k = k1_args(a, nullptr, nullptr, msgs, moff);
    hipStream_t s = a.begin();
    auto out = torch::zeros({k.N, 64}, opts(torch::kUInt8, msgs));
    if (k.N > 0) {
        launch_k1_hash_to_g1(k.msgs, k.moff, k.N, a.ptr<uint8_t>(out, "out"), s);
        a.launched();
    }
    return out;
}

// What the pair-list fan-outs share: the batch, the per-message offset and
// length columns (one length), the pair list with its device-side count,
// and the egress rings.
struct FanoutArgs {
    const uint8_t* buf;
    const int64_t* payload_off;
    const int32_t* payload_len;
    const PairRec* pairs;
    const int32_t* n_pairs;
    uint8_t* egress;
    int32_t capacity;
    int nt, grid;    // nt is a flag
    int64_t n_msgs;  // the columns' length, for a msg_seq column to match
};

static FanoutArgs fanout_args(Op& a, const torch::Tensor& buf, const torch::Tensor& payload_off,
                              const torch::Tensor& payload_len, const torch::Tensor& pairs,
                              const torch::Tensor& n_pairs, const torch::Tensor& egress,
                              int64_t nt, int64_t grid) {
    FanoutArgs f;
    f.buf = a.ptr<uint8_t>(buf, "buf");
    f.n_msgs = payload_off.numel();
    f.payload_off = a.ptr<int64_t>(payload_off, "payload_off");
    f.payload_len = a.same<int32_t>(payload_len, "payload_len", f.n_msgs, "one per payload_off");
    f.pairs = a.pairs(pairs);
    f.capacity = a.i32(pairs.size(0), "pair capacity");
    f.n_pairs = a.ptr<int32_t>(n_pairs, "n_pairs", 1);
    f.egress = a.ptr<uint8_t>(egress, "egress");
    f.nt = nt != 0;
    f.grid = a.i32(grid, "grid");
    return f;
}

void fanout_wave(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                 torch::Tensor pairs,
                 torch::Tensor msg_seq, torch::Tensor n_pairs, torch::Tensor egress,
                 int64_t nt, int64_t grid) {
    Op a("fanout_wave");
    const FanoutArgs f = fanout_args(a, buf, payload_off, payload_len, pairs, n_pairs, egress,
                                     nt, grid);
    const uint32_t* seq = a.same<uint32_t>(msg_seq, "msg_seq", f.n_msgs, "one per payload_off");
    hipStream_t s = a.begin();
    launch_k3_fanout_wave(f.buf, f.payload_off, f.payload_len, f.pairs, seq, f.n_pairs,
                          f.capacity, f.egress, f.nt, f.grid, s);
    a.launched();
}

void fanout_ref(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                torch::Tensor pairs,
                torch::Tensor msg_seq, torch::Tensor n_pairs, torch::Tensor egress,
                int64_t nt, int64_t grid, int64_t ref_threshold, int64_t ref_base) {
    Op a("fanout_ref");
    const FanoutArgs f = fanout_args(a, buf, payload_off, payload_len, pairs, n_pairs, egress,
                                     nt, grid);
    const uint32_t* seq = a.same<uint32_t>(msg_seq, "msg_seq", f.n_msgs, "one per payload_off");
    const int32_t thr = a.i32(ref_threshold, "ref_threshold");
    TORCH_CHECK(ref_base >= 0, a.name(), ": ref_base = ", ref_base, " must not be negative");
    hipStream_t s = a.begin();
    launch_k3_fanout_ref(f.buf, f.payload_off, f.payload_len, f.pairs, seq, f.n_pairs,
                         f.capacity, thr, ref_base, f.egress, f.nt, f.grid, s);
    a.launched();
}

// fanout_flat2 (seq_state == nullptr: the seq base comes by value, mod 2^32)
// and fanout_flat3 (the seq base is read from the device counter seq_state).
static void fanout_flat(const char* op, const torch::Tensor& buf,
                        const torch::Tensor& payload_off, const torch::Tensor& payload_len,
                        const torch::Tensor& pairs, int64_t seq_base,
                        const torch::Tensor* seq_state, const torch::Tensor& n_pairs,
                        int64_t units_per_pair, const torch::Tensor& egress, int64_t nt,
                        int64_t grid, int64_t uniform_len) {
    Op a(op);
    const FanoutArgs f = fanout_args(a, buf, payload_off, payload_len, pairs, n_pairs, egress,
                                     nt, grid);
    const uint32_t* state = seq_state ? a.ptr<uint32_t>(*seq_state, "seq_state", 1) : nullptr;
    check_flat_shape(pairs, units_per_pair);
    const int32_t units = a.i32(units_per_pair, "units_per_pair");
    const int32_t ulen = a.i32(uniform_len, "uniform_len");
    hipStream_t s = a.begin();
    if (state)
        launch_k3_fanout_flat3(f.buf, f.payload_off, f.payload_len, f.pairs, state, f.n_pairs,
                               f.capacity, units, ulen, f.egress, f.nt, f.grid, s);
    else
        launch_k3_fanout_flat2(f.buf, f.payload_off, f.payload_len, f.pairs, (uint32_t)seq_base,
                               f.n_pairs, f.capacity, units, ulen, f.egress, f.nt, f.grid, s);
    a.launched();
}

void fanout_flat2(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                  torch::Tensor pairs,
                  int64_t seq_base, torch::Tensor n_pairs, int64_t units_per_pair,
                  torch::Tensor egress, int64_t nt, int64_t grid, int64_t uniform_len) {
    fanout_flat("fanout_flat2", buf, payload_off, payload_len, pairs, seq_base, nullptr, n_pairs,
                units_per_pair, egress, nt, grid, uniform_len);
}

void fanout_flat3(torch::Tensor buf, torch::Tensor payload_off, torch::Tensor payload_len,
                  torch::Tensor pairs,
                  torch::Tensor seq_state, torch::Tensor n_pairs, int64_t units_per_pair,
                  torch::Tensor egress, int64_t nt, int64_t grid, int64_t uniform_len) {
    fanout_flat("fanout_flat3", buf, payload_off, payload_len, pairs, 0, &seq_state, n_pairs,
                units_per_pair, egress, nt, grid, uniform_len);
}

void seq_advance(torch::Tensor seq_state, int64_t m) {
    Op a("seq_advance");
    uint32_t* state = a.ptr<uint32_t>(seq_state, "seq_state", 1);
    const int32_t m32 = a.i32(m, "m");
    launch_k_seq_advance(state, m32, a.begin());
    a.launched();
}

torch::Tensor topic_mask_t(torch::Tensor sub_bitmap, torch::Tensor buf,
                           torch::Tensor topics_off, torch::Tensor topics_cnt,
                           torch::Tensor disc) {
    Op a("topic_mask_t");
    const TopicArgs t = topic_args(a, sub_bitmap, buf, topics_off, topics_cnt, disc);
    hipStream_t s = a.begin();
    auto mask_t = torch::empty({t.W, t.M}, opts(torch::kInt64, buf));
    if (t.M > 0) {
        launch_k2a_topic_mask_t(t.sub_bitmap, t.buf, t.topics_off, t.topics_cnt, t.disc,
                                a.ptr<uint64_t>(mask_t, "mask_t"), t.M, t.W, s);
        a.launched();
    }
    return mask_t;
}

// What the two transposed K2b ops share: mask_t [W][M], the recipient count
// n within the mask's 64 W bits, one cursor per recipient, the pair list and
// its two counters.
struct EmitArgs {
    const uint64_t* mask_t;
    uint64_t* ring_wpos;
    PairRec* pairs;
    uint32_t* drops;
    int32_t* n_pairs;
    int32_t M, W, n, capacity;
};

static EmitArgs emit_args(Op& a, const torch::Tensor& mask_t, const torch::Tensor& ring_wpos,
                          int64_t ring_bytes, int64_t n_users, const torch::Tensor& pairs,
                          const torch::Tensor& drops, const torch::Tensor& n_pairs) {
    EmitArgs e;
    e.mask_t = a.ptr<uint64_t>(mask_t, "mask_t", 0, mat());
    e.W = a.i32(mask_t.size(0), "W");
    e.M = a.i32(mask_t.size(1), "M");
    e.n = a.i32(n_users, "n_users", 0, int64_t(e.W) * 64);
    a.ring_bytes(ring_bytes);
    e.ring_wpos = a.ptr<uint64_t>(ring_wpos, "ring_wpos", e.n);
    e.pairs = a.pairs(pairs);
    e.capacity = a.i32(pairs.size(0), "pair capacity");
    e.drops = a.ptr<uint32_t>(drops, "drops", 1);
    e.n_pairs = a.ptr<int32_t>(n_pairs, "n_pairs", 1);
    return e;
}

void assign_emit_fused_t(torch::Tensor mask_t, torch::Tensor payload_len,
                         torch::Tensor ring_wpos, int64_t ring_bytes, int64_t n_users,
                         torch::Tensor pairs, torch::Tensor drops, torch::Tensor n_pairs,
                         int64_t uniform_rec) {
    Op a("assign_emit_fused_t");
    const EmitArgs e = emit_args(a, mask_t, ring_wpos, ring_bytes, n_users, pairs, drops, n_pairs);
    const int32_t* plen = a.ptr<int32_t>(payload_len, "payload_len", e.M);
    const int32_t rec = a.i32(uniform_rec, "uniform_rec");
    hipStream_t s = a.begin();
    if (e.n == 0) return;  // no recipient: nothing to claim, and no grid to launch
    launch_k2b_fused_t(e.mask_t, plen, e.M, e.W, e.n, ring_bytes, e.capacity, rec, e.ring_wpos,
                       e.n_pairs, e.pairs, e.drops, s);
    a.launched();
}

void assign_emit_blocks_t(torch::Tensor mask_t, torch::Tensor ring_wpos,
                          int64_t ring_bytes, int64_t n_users,
                          torch::Tensor bcount, torch::Tensor pprefix, torch::Tensor ubase,
                          torch::Tensor ufit, torch::Tensor udst,
                          torch::Tensor pairs, torch::Tensor drops, torch::Tensor n_pairs,
                          int64_t uniform_rec) {
    Op a("assign_emit_blocks_t");
    const EmitArgs e = emit_args(a, mask_t, ring_wpos, ring_bytes, n_users, pairs, drops, n_pairs);
    const int32_t rec = a.i32(uniform_rec, "uniform_rec", 1);
    const int64_t W64 = int64_t(e.W) * 64, NB = k2b_blocks(e.M);
    int32_t* bc = a.ptr<int32_t>(bcount, "bcount", NB * W64);
    int32_t* pp = a.ptr<int32_t>(pprefix, "pprefix", NB * W64);
    int32_t* ub = a.ptr<int32_t>(ubase, "ubase", W64);
    int32_t* uf = a.ptr<int32_t>(ufit, "ufit", W64);
    int64_t* ud = a.ptr<int64_t>(udst, "udst", W64);
    hipStream_t s = a.begin();
    if (e.n == 0) return;  // as in assign_emit_fused_t
    launch_k2b_blocks_t(e.mask_t, e.M, e.W, e.n, ring_bytes, e.capacity, rec, e.ring_wpos,
                        e.n_pairs, bc, pp, ub, uf, ud, e.pairs, e.drops, s);
    a.launched();
}

// What the two K5b ops share: four per-message columns of disc's length M
// (origin is a fifth where the op takes it), the cursors, the pair list and
// its two counters.
struct DirectArgs {
    const int32_t* disc;
    const int32_t* owner;
    const int64_t* payload_off;
    const int32_t* payload_len;
    int32_t M, capacity;
};

static DirectArgs direct_args(Op& a, const torch::Tensor& disc, const torch::Tensor& owner,
                              const torch::Tensor& payload_off, const torch::Tensor& payload_len,
                              int64_t ring_bytes) {
    DirectArgs d;
    d.disc = a.ptr<int32_t>(disc, "disc");
    d.M = a.i32(disc.numel(), "M");
    d.owner = a.same<int32_t>(owner, "owner", d.M, "one per disc");
    d.payload_off = a.same<int64_t>(payload_off, "payload_off", d.M, "one per disc");
    d.payload_len = a.same<int32_t>(payload_len, "payload_len", d.M, "one per disc");
    a.ring_bytes(ring_bytes);
    return d;
}

void emit_direct(torch::Tensor disc, torch::Tensor owner, torch::Tensor payload_off,
                 torch::Tensor payload_len, int64_t ring_bytes, torch::Tensor ring_wpos,
                 torch::Tensor n_pairs, torch::Tensor pairs, torch::Tensor drops) {
    Op a("emit_direct");
    const DirectArgs d = direct_args(a, disc, owner, payload_off, payload_len, ring_bytes);
    uint64_t* wpos = a.ptr<uint64_t>(ring_wpos, "ring_wpos");
    int32_t* np = a.ptr<int32_t>(n_pairs, "n_pairs", 1);
    PairRec* pr = a.pairs(pairs);
    const int32_t capacity = a.i32(pairs.size(0), "pair capacity");
    uint32_t* dr = a.ptr<uint32_t>(drops, "drops", 1);
    hipStream_t s = a.begin();
    if (d.M == 0) return;
    launch_k5b_emit_direct(d.disc, d.owner, d.payload_off, d.payload_len, d.M, ring_bytes,
                           capacity, wpos, np, pr, dr, s);
    a.launched();
}

torch::Tensor topic_mask_origin_t(torch::Tensor sub_bitmap, torch::Tensor buf,
                                  torch::Tensor topics_off, torch::Tensor topics_cnt,
                                  torch::Tensor disc, torch::Tensor origin, int64_t n_users) {
    Op a("topic_mask_origin_t");
    const TopicArgs t = topic_args(a, sub_bitmap, buf, topics_off, topics_cnt, disc);
    const int32_t* org = a.same<int32_t>(origin, "origin", t.M, "one per disc");
    const int32_t n = a.i32(n_users, "n_users", 0, int64_t(t.W) * 64);
    hipStream_t s = a.begin();
    auto mask_t = torch::empty({t.W, t.M}, opts(torch::kInt64, buf));
    if (t.M > 0) {
        launch_k2a_topic_mask_origin_t(t.sub_bitmap, t.buf, t.topics_off, t.topics_cnt, t.disc,
                                       org, a.ptr<uint64_t>(mask_t, "mask_t"), t.M, t.W, n, s);
        a.launched();
    }
    return mask_t;
}

void emit_direct_peers(torch::Tensor disc, torch::Tensor owner, torch::Tensor origin,
                       torch::Tensor payload_off, torch::Tensor payload_len,
                       int64_t ring_bytes, int64_t n_users, int64_t n_peers,
                       torch::Tensor ring_wpos, torch::Tensor n_pairs, torch::Tensor pairs,
                       torch::Tensor drops) {
    Op a("emit_direct_peers");
    const DirectArgs d = direct_args(a, disc, owner, payload_off, payload_len, ring_bytes);
    const int32_t* org = a.same<int32_t>(origin, "origin", d.M, "one per disc");
    const int32_t n = a.i32(n_users, "n_users");
    const int32_t p = a.i32(n_peers, "n_peers");
    uint64_t* wpos = a.ptr<uint64_t>(ring_wpos, "ring_wpos", int64_t(n) + p);
    int32_t* np = a.ptr<int32_t>(n_pairs, "n_pairs", 1);
    PairRec* pr = a.pairs(pairs);
    const int32_t capacity = a.i32(pairs.size(0), "pair capacity");
    uint32_t* dr = a.ptr<uint32_t>(drops, "drops", 1);
    hipStream_t s = a.begin();
    if (d.M == 0) return;
    launch_k5b_emit_direct_peers(d.disc, d.owner, org, d.payload_off, d.payload_len, d.M, n, p,
                                 ring_bytes, capacity, wpos, np, pr, dr, s);
    a.launched();
}

void direct_apply(torch::Tensor table_keys, torch::Tensor table_vals, torch::Tensor up_keys,
                  torch::Tensor up_owners, torch::Tensor del_keys, torch::Tensor n_failed) {
    Op a("direct_apply");
    uint64_t* keys = a.ptr<uint64_t>(table_keys, "table_keys", 1, vec());
    const int64_t S = table_keys.numel();
    TORCH_CHECK((S & (S - 1)) == 0, a.name(), ": table_keys must have a power-of-two length, got ",
                S);
    int32_t* vals = a.same<int32_t>(table_vals, "table_vals", S, "one per table_keys");
    const uint64_t* up = a.ptr<uint64_t>(up_keys, "up_keys");
    const int32_t n_up = a.i32(up_keys.numel(), "upsert count");
    const int32_t* owners = a.same<int32_t>(up_owners, "up_owners", n_up, "one per up_keys");
    const uint64_t* del = a.ptr<uint64_t>(del_keys, "del_keys");
    const int32_t n_del = a.i32(del_keys.numel(), "delete count");
    uint32_t* failed = a.ptr<uint32_t>(n_failed, "n_failed", 1);
    hipStream_t s = a.begin();
    launch_k6_direct_apply(keys, vals, S, up, owners, n_up, del, n_del, failed, s);
    a.launched();
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
    Op a("tick_uniform_broadcast");
    UniformTick t;
    t.uniform_len = a.i32(uniform_len, "uniform_len", 0, (int64_t(1) << 30) - 1);
    const int64_t rec = (uniform_len + 16 + 15) & ~int64_t(15);
    t.rec = a.i32(rec, "rec");
    t.buf = a.ptr<uint8_t>(buf, "buf");
    t.offsets = a.ptr<int64_t>(offsets, "offsets", 1);
    const int64_t M = offsets.numel() - 1;
    t.M = a.i32(M, "M");
    t.hash_seed = hash_seed;
    t.sub_bitmap = a.ptr<uint64_t>(sub_bitmap, "sub_bitmap", 0, mat(256, -1));
    const int64_t W = sub_bitmap.size(1);
    t.W = a.i32(W, "W");
    t.n_users = a.i32(n_users, "n_users", 0, W * 64);
    a.ring_bytes(ring_bytes);
    t.ring_bytes = ring_bytes;
    t.ring_wpos = a.ptr<uint64_t>(ring_wpos, "ring_wpos", n_users);
    t.pairs = a.pairs(pairs);
    t.capacity = a.i32(pairs.size(0), "pair capacity");
    t.drops = a.ptr<uint32_t>(drops, "drops", 1);
    t.n_pairs = a.ptr<int32_t>(n_pairs, "n_pairs", 1);
    t.n_sparse = a.ptr<int32_t>(n_sparse, "n_sparse", 1);
    t.scratch64 = a.ptr<int64_t>(scratch64, "scratch64", uniform_tick_scratch64(M, W, rec / 16));
    t.scratch32 = a.ptr<int32_t>(scratch32, "scratch32", uniform_tick_scratch32(M, W));
    t.egress = a.ptr<uint8_t>(egress, "egress", n_users * ring_bytes);
    t.seq_base = (uint32_t)seq_base;  // sequence numbers count mod 2^32
    t.nt = nt != 0;
    t.dense = dense != 0;
    TORCH_CHECK(buf.numel() >= M * uniform_len, a.name(), ": buf has ", buf.numel(),
                " bytes, shorter than M = ", M, " messages of uniform_len = ", uniform_len);
    check_flat_shape(pairs, rec / 16);
    // the image kernel's unit index and the fan-out's 1-D grid: the dense
    // workgroups and the sparse tail behind them
    TORCH_CHECK(M * (rec / 16) < (int64_t(1) << 31)
                && dense_grid_x(t.n_users, DENSE_GROUP, dense_geom((int32_t)(rec / 16)).n_chunks)
                       * k2b_blocks(M) + SPARSE_TAIL_BLOCKS < (int64_t(1) << 31),
                a.name(), ": batch too large for the dense fan-out");
    TORCH_CHECK((uintptr_t)t.scratch64 % 16 == 0, a.name(), ": scratch64 must be 16-byte aligned");
    hipStream_t s = a.begin();
    if (M == 0) return;
    launch_tick_uniform_broadcast(&t, s);
    a.launched();
}

std::vector<int64_t> uniform_tick_scratch_sizes(int64_t M, int64_t W, int64_t rec) {
    return {uniform_tick_scratch64(M, W, rec / 16), uniform_tick_scratch32(M, W)};
}

// Fused drain: one kernel stores the cursors into the engine's pinned `host`
// buffer, through that buffer's device-visible address, and zeroes them; one
// stream synchronise makes the buffer readable.  A pinned buffer without a
// device-visible address takes two hops: the kernel stores to `staging` and
// an async copy lands that in `host`.  Pinned memory always has such an
// address on the hardware this is built for, so no GPU test reaches the two
// hops; they are the path this op took before it stored directly.
void drain_cursors(torch::Tensor ring_wpos, torch::Tensor staging, torch::Tensor host) {
    Op a("drain_cursors");
    int64_t* wpos = a.ptr<int64_t>(ring_wpos, "ring_wpos");
    const int32_t n = a.i32(ring_wpos.numel(), "cursor count");
    int64_t* st = a.ptr<int64_t>(staging, "staging", n);
    int64_t* h = a.ptr<int64_t>(host, "host", n, {}, Op::kPinnedHost);
    hipStream_t s = a.begin();
    if (n == 0) return;
    void* h_dev = nullptr;
    if (hipHostGetDevicePointer(&h_dev, h, 0) == hipSuccess && h_dev != nullptr) {
        launch_drain_cursors(wpos, (int64_t*)h_dev, n, s);
        a.launched();
    } else {
        (void)hipGetLastError();  // clear it: the two hops below need no device view
        launch_drain_cursors(wpos, st, n, s);
        a.launched();
        a.check(hipMemcpyAsync(h, st, (size_t)n * 8, hipMemcpyDeviceToHost, s), "copy");
    }
    a.check(hipStreamSynchronize(s), "sync");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    // largest batch tick_uniform_broadcast routes in one kernel (tick_geom.h)
    m.attr("_ROUTE_MAX_M") = py::int_(ROUTE_MAX_M);
    // flat workgroups behind the dense ones in its fan-out launch (tick_geom.h)
    m.attr("_SPARSE_TAIL_BLOCKS") = py::int_(SPARSE_TAIL_BLOCKS);
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
