// Native framed-socket pump: an epoll thread that owns connected TCP
// sockets and does all per-frame work in C++ — reading 4-byte-BE
// length-delimited frames into complete messages and flushing queued
// outbound frames with writev-style batching.  Python (asyncio) exchanges
// WHOLE message batches with the pump and is woken through an eventfd it
// watches with loop.add_reader, so the per-message hot path never enters
// the interpreter.
//
// This is the MI355X-native equivalent of the reference's tokio connection
// core (cdn-proto/src/connection/protocols/mod.rs:139-217: dedicated
// reader/writer actors per connection): same framing
// (read/write_length_delimited, :311-394), same max-size guard, same
// soft-close flush semantics.
#pragma once

#include <arpa/inet.h>
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/epoll.h>
#include <sys/eventfd.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <algorithm>
#include <thread>
#include <tuple>
#include <vector>

#include "../wire/message.h"

namespace net {

// wire framing limit — mirrors proto/transports/base.py MAX_MESSAGE_SIZE
constexpr uint64_t kMaxMessageSize = (0xFFFFFFFFull) / 8;

// Structural classification of one wire frame for the C++ ingest path —
// the data-plane fields the broker routes on, WITHOUT copying the payload
// (offset/length views into the frame; host mirror of the K4 kernel's
// output shape). disc = -1 marks a malformed frame (caller disconnects,
// reference user/handler.rs:109 semantics).
struct FrameMeta {
    int32_t disc = -1;
    uint32_t topics_off = 0, topics_cnt = 0;   // Broadcast/Sub/Unsub, frame-relative
    uint32_t recip_off = 0, recip_len = 0;     // Direct, frame-relative
};

inline FrameMeta classify_frame(const uint8_t* buf, size_t len) {
    FrameMeta m;
    if (len < 16) return m;
    uint32_t seg_m1, nw;
    memcpy(&seg_m1, buf, 4);
    memcpy(&nw, buf + 4, 4);
    if (seg_m1 != 0 || 8 + (uint64_t)nw * 8 > len) return m;
    wire::Reader r{buf + 8, nw};
    size_t mt;
    uint16_t mdw, mpw;
    if (!r.struct_ptr(0, &mt, &mdw, &mpw) || mdw < 1 || mpw < 1) return m;
    uint64_t w0;
    r.u64(mt, &w0);
    uint16_t disc = (uint16_t)w0;
    size_t up = mt + mdw;
    // offset-returning byte-list decode (no copy)
    auto list_view = [&](size_t pw, uint32_t* off, uint32_t* n) -> bool {
        uint64_t v;
        if (!r.u64(pw, &v)) return false;
        if (v == 0) { *off = 0; *n = 0; return true; }
        if ((v & 3) != 1) return false;
        int64_t b = (v >> 2) & 0x3fffffff;
        if (b & 0x20000000) b -= 0x40000000;
        if (((v >> 32) & 7) != 2) return false;
        uint64_t count = (v >> 35) & 0x1fffffff;
        int64_t t = (int64_t)pw + 1 + b;
        if (t < 0 || (uint64_t)t * 8 + count > (uint64_t)nw * 8) return false;
        *off = (uint32_t)(8 + t * 8);
        *n = (uint32_t)count;
        return true;
    };
    switch (disc) {
    case wire::DIRECT: {
        size_t it; uint16_t idw, ipw;
        if (!r.struct_ptr(up, &it, &idw, &ipw) || ipw < 2) return m;
        if (!list_view(it + idw, &m.recip_off, &m.recip_len)) return m;
        break;
    }
    case wire::BROADCAST: {
        size_t it; uint16_t idw, ipw;
        if (!r.struct_ptr(up, &it, &idw, &ipw) || ipw < 2) return m;
        if (!list_view(it + idw, &m.topics_off, &m.topics_cnt)) return m;
        break;
    }
    case wire::SUBSCRIBE:
    case wire::UNSUBSCRIBE:
        if (!list_view(up, &m.topics_off, &m.topics_cnt)) return m;
        break;
    case wire::AUTHENTICATE_WITH_KEY:
    case wire::AUTHENTICATE_WITH_PERMIT:
    case wire::AUTHENTICATE_RESPONSE:
    case wire::USER_SYNC:
    case wire::TOPIC_SYNC:
        break;
    default:
        return m;
    }
    m.disc = disc;
    return m;
}

struct Conn {
    int fd = -1;
    // inbound frame assembly (state machine): header bytes accumulate in
    // hdr; the body is received DIRECTLY into `frame` — a 100 MiB message
    // lands in its final buffer with zero intermediate copies (round-1's
    // rbuf accumulate+slice+erase path cost ~3 extra passes per byte)
    uint8_t hdr[4];
    size_t hdr_have = 0;
    std::string frame;                   // body in flight
    size_t frame_have = 0;
    uint64_t frame_need = 0;             // 0 = still reading the header
    std::deque<std::string> inbox;       // complete frames (payload only)
    // C++ ingest mode (GPU broker data plane): complete frames accumulate
    // in ONE contiguous buffer with offsets + routing metadata; Python
    // pulls a whole tick's worth in one call (recv_ingest)
    bool ingest = false;
    bool paused = false;                 // EPOLLIN parked: ibuf over budget
    std::string ibuf;
    std::vector<int64_t> ioffs;          // frame end offsets into ibuf
    std::vector<FrameMeta> imeta;
    // outbound
    std::deque<std::string> outbox;      // framed bytes (header+payload)
    size_t out_off = 0;                  // offset into outbox.front()
    bool want_write = false;
    bool closed = false;
    bool soft_closing = false;           // flush outbox then close
    bool forget_pending = false;         // erase once flushed + closed
    uint64_t in_bytes = 0, out_bytes = 0;
};

// ingest-mode read backpressure threshold: above this, stop reading the
// socket until Python drains (TCP window then backpressures the sender —
// the reference's limiter-blocks-the-reader behavior, protocols/mod.rs:328)
constexpr size_t kIngestPauseBytes = 32u << 20;

class Pump {
public:
    Pump() {
        epfd_ = epoll_create1(EPOLL_CLOEXEC);
        evfd_ = eventfd(0, EFD_CLOEXEC | EFD_NONBLOCK);
        wakefd_ = eventfd(0, EFD_CLOEXEC | EFD_NONBLOCK);
        struct epoll_event ev {};
        ev.events = EPOLLIN;
        ev.data.u64 = kWakeToken;
        epoll_ctl(epfd_, EPOLL_CTL_ADD, wakefd_, &ev);
        thread_ = std::thread([this] { run(); });
    }

    ~Pump() { stop(); }

    void stop() {
        bool expected = false;
        if (!stopping_.compare_exchange_strong(expected, true)) return;
        wake();
        if (thread_.joinable()) thread_.join();
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : conns_)
            if (kv.second.fd >= 0) ::close(kv.second.fd);
        conns_.clear();
        if (epfd_ >= 0) ::close(epfd_);
        if (evfd_ >= 0) ::close(evfd_);
        if (wakefd_ >= 0) ::close(wakefd_);
        epfd_ = evfd_ = wakefd_ = -1;
    }

    // fd for Python's loop.add_reader: becomes readable whenever any
    // connection has new inbound frames or changes state
    int notify_fd() const { return evfd_; }

    // register a CONNECTED socket; the pump takes ownership of the fd
    int64_t add(int fd) {
        int flags = fcntl(fd, F_GETFL, 0);
        fcntl(fd, F_SETFL, flags | O_NONBLOCK);
        int one = 1;
        setsockopt(fd, IPPROTO_TCP, 1 /*TCP_NODELAY*/, &one, sizeof(one));
        int bufsz = 4 << 20;  // large frames: fewer syscalls per message
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &bufsz, sizeof(bufsz));
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &bufsz, sizeof(bufsz));
        int64_t id;
        {
            std::lock_guard<std::mutex> g(mu_);
            id = next_id_++;
            conns_[id].fd = fd;
        }
        struct epoll_event ev {};
        ev.events = EPOLLIN;
        ev.data.u64 = (uint64_t)id;
        epoll_ctl(epfd_, EPOLL_CTL_ADD, fd, &ev);
        return id;
    }

    // queue one frame; returns false if the connection is gone
    bool send(int64_t id, const char* data, size_t len) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end() || it->second.closed || it->second.soft_closing)
            return false;
        std::string framed;
        framed.resize(4 + len);
        uint32_t be = htonl((uint32_t)len);
        memcpy(&framed[0], &be, 4);
        memcpy(&framed[4], data, len);
        it->second.outbox.emplace_back(std::move(framed));
        it->second.want_write = true;
        wake();
        return true;
    }

    // enqueue every record of a drained egress ring as one frame each —
    // ring layout: {u32 len, u32 seq, 8B pad} + payload, 16-aligned
    // (pushcdn_amd/broker/gpu_engine.py ring_rec / parse_ring_records).
    // The payload IS a serialized wire message, so it goes out verbatim.
    // Returns (records enqueued, payload bytes) — (0,0) if the conn is gone.
    // `ref` / `ref_len`: the reference buffer by-reference records point
    // into (nullptr = none; see build_ring_frames).
    std::pair<int64_t, int64_t> send_ring(int64_t id, const uint8_t* ring, size_t wpos,
                                          const uint8_t* ref = nullptr, size_t ref_len = 0) {
        std::string buf;
        auto r = build_ring_frames(ring, wpos, &buf, ref, ref_len);
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end() || it->second.closed || it->second.soft_closing)
            return {0, 0};
        if (r.first) {
            it->second.outbox.emplace_back(std::move(buf));
            it->second.want_write = true;
            wake();
        }
        return r;
    }

    // Batched egress drain: ONE call for a whole tick's worth of users.
    // `base` is the compacted staging buffer (K7 gather of every used ring
    // prefix, D2H'd in one copy); user j's records occupy
    // [starts[j], ends[j]).  The coalesced per-user frame buffers are
    // built OUTSIDE the pump mutex (and the caller releases the GIL), so
    // neither the epoll thread nor the event loop stalls behind the
    // memcpy; the lock is held only to push finished buffers.  Per-user
    // record counts are returned; -1 marks a connection that is gone
    // (caller evicts — reference user/sender.rs:16-33).
    // returns per-user [count, payload_bytes] interleaved; count -1 = gone
    std::vector<int64_t> send_rings_batch(const uint8_t* base,
                                          const std::vector<int64_t>& ids,
                                          const std::vector<int64_t>& starts,
                                          const std::vector<int64_t>& ends,
                                          const uint8_t* ref = nullptr,
                                          size_t ref_len = 0) {
        size_t n_users = ids.size();
        std::vector<int64_t> counts(n_users, 0);
        std::vector<std::string> bufs(n_users);
        std::vector<int64_t> payload(n_users, 0);
        for (size_t j = 0; j < n_users; ++j) {
            auto r = build_ring_frames(base + starts[j],
                                       (size_t)(ends[j] - starts[j]), &bufs[j],
                                       ref, ref_len);
            counts[j] = r.first;
            payload[j] = r.second;
        }
        bool any = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t j = 0; j < n_users; ++j) {
                auto it = conns_.find(ids[j]);
                if (it == conns_.end() || it->second.closed || it->second.soft_closing) {
                    counts[j] = -1;
                    continue;
                }
                if (counts[j] > 0) {
                    it->second.outbox.emplace_back(std::move(bufs[j]));
                    it->second.want_write = true;
                    any = true;
                }
            }
        }
        if (any) wake();
        std::vector<int64_t> out(2 * n_users);
        for (size_t j = 0; j < n_users; ++j) {
            out[2 * j] = counts[j];
            out[2 * j + 1] = counts[j] < 0 ? 0 : payload[j];
        }
        return out;
    }

    // One bounds-checked walk over the length prefixes of `len` bytes that
    // claim to be `cnt` frames [u32 BE length][body] back to back (the framed
    // drain's output, gpu_engine.drain_framed): true iff there are exactly
    // cnt frames, each at most kMaxMessageSize, tiling [0, len) exactly.
    // Reads 4 bytes per frame and no body.
    static bool check_frames(const uint8_t* p, size_t len, int64_t cnt) {
        if (cnt < 0) return false;
        size_t pos = 0;
        int64_t n = 0;
        while (pos < len) {
            if (len - pos < 4 || n == cnt) return false;
            uint32_t be;
            memcpy(&be, p + pos, 4);
            const uint64_t body = ntohl(be);
            if (body > kMaxMessageSize || body > len - pos - 4) return false;
            pos += 4 + (size_t)body;
            ++n;
        }
        return n == cnt;
    }

    // send_rings_batch for a framed drain: entry j is lens[j] bytes at
    // base + starts[j] that already ARE cnts[j] socket-ready frames in
    // arrival order, so they are checked (check_frames) and queued verbatim
    // with one copy: no record parse, no sort, no second body copy.  An entry
    // that fails the check queues nothing and reports count -2: a bad prefix
    // must never reach a client, it would desynchronise the stream for good.
    // cnts[j] == -1: the entry is a raw ring prefix (the drain's ring mode)
    // and goes through build_ring_frames as in send_rings_batch.
    // Returns per-entry [count, payload_bytes] interleaved; count -1 = the
    // connection is gone.  Everything but the outbox push happens outside
    // the mutex.
    std::vector<int64_t> send_framed_batch(const uint8_t* base,
                                           const std::vector<int64_t>& ids,
                                           const std::vector<int64_t>& starts,
                                           const std::vector<int64_t>& lens,
                                           const std::vector<int64_t>& cnts) {
        size_t n_users = ids.size();
        std::vector<int64_t> counts(n_users, 0);
        std::vector<std::string> bufs(n_users);
        std::vector<int64_t> payload(n_users, 0);
        for (size_t j = 0; j < n_users; ++j) {
            const uint8_t* p = base + starts[j];
            const size_t len = (size_t)lens[j];
            if (cnts[j] == -1) {
                auto r = build_ring_frames(p, len, &bufs[j]);
                counts[j] = r.first;
                payload[j] = r.second;
            } else if (check_frames(p, len, cnts[j])) {
                bufs[j].assign((const char*)p, len);
                counts[j] = cnts[j];
                payload[j] = (int64_t)len - 4 * cnts[j];
            } else {
                counts[j] = -2;
            }
        }
        bool any = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t j = 0; j < n_users; ++j) {
                auto it = conns_.find(ids[j]);
                if (it == conns_.end() || it->second.closed || it->second.soft_closing) {
                    counts[j] = -1;
                    continue;
                }
                if (counts[j] > 0) {
                    it->second.outbox.emplace_back(std::move(bufs[j]));
                    it->second.want_write = true;
                    any = true;
                }
            }
        }
        if (any) wake();
        std::vector<int64_t> out(2 * n_users);
        for (size_t j = 0; j < n_users; ++j) {
            out[2 * j] = counts[j];
            out[2 * j + 1] = counts[j] < 0 ? 0 : payload[j];
        }
        return out;
    }

    // bytes queued but not yet written (backpressure signal for Python)
    int64_t send_backlog(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return -1;
        int64_t n = 0;
        for (auto& s : it->second.outbox) n += (int64_t)s.size();
        return n - (int64_t)it->second.out_off;
    }

    // ids whose inbox or closed-state changed since the last poll
    std::vector<int64_t> poll_dirty() {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<int64_t> out(dirty_.begin(), dirty_.end());
        dirty_.clear();
        uint64_t junk;
        while (read(evfd_, &junk, 8) == 8) {}
        return out;
    }

    // enable C++ ingest mode for a connection (GPU broker user plane):
    // frames accumulate contiguously with routing metadata; Python pulls a
    // tick's worth at a time with recv_ingest
    void set_ingest(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return;
        auto& c = it->second;
        c.ingest = true;
        // frames that raced in through the normal inbox re-route
        while (!c.inbox.empty()) {
            std::string& f = c.inbox.front();
            c.imeta.push_back(classify_frame((const uint8_t*)f.data(), f.size()));
            c.ibuf.append(f);
            c.ioffs.push_back((int64_t)c.ibuf.size());
            c.inbox.pop_front();
        }
    }

    struct IngestBatch {
        std::string blob;                // concatenated frame bytes
        std::vector<int64_t> offs;       // frame END offsets
        std::vector<FrameMeta> meta;
        bool closed = false;
    };

    // pull everything the pump has classified for this connection (ONE
    // Python call per tick per connection instead of one per message)
    IngestBatch recv_ingest(int64_t id) {
        IngestBatch out;
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) {
            out.closed = true;
            return out;
        }
        auto& c = it->second;
        out.blob.swap(c.ibuf);
        out.offs.swap(c.ioffs);
        out.meta.swap(c.imeta);
        out.closed = c.closed;
        if (c.paused && c.fd >= 0) {
            c.paused = false;
            update_interest(id, c);
            wake();
        }
        return out;
    }

    // enqueue PRE-FRAMED bytes verbatim (a batch of [4B len][frame] records
    // built by the caller) — the sender-side batch analog of send()
    bool send_raw(int64_t id, const char* data, size_t len) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end() || it->second.closed || it->second.soft_closing)
            return false;
        it->second.outbox.emplace_back(data, len);
        it->second.want_write = true;
        wake();
        return true;
    }

    // drain EVERYTHING, returning only (count, bytes, last frame, closed) —
    // the counting-subscriber path for benchmarks/relays where per-frame
    // Python objects are pure overhead
    std::tuple<int64_t, int64_t, std::string, bool> recv_drain(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return {0, 0, std::string(), true};
        auto& c = it->second;
        int64_t n = 0, bytes = 0;
        std::string last;
        while (!c.inbox.empty()) {
            last = std::move(c.inbox.front());
            c.inbox.pop_front();
            ++n;
            bytes += (int64_t)last.size();
        }
        return {n, bytes, std::move(last), c.closed};
    }

    // drain up to max_frames complete inbound frames; empty vector + closed
    // flag tells Python the peer is gone
    std::pair<std::vector<std::string>, bool> recv_batch(int64_t id, size_t max_frames) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return {{}, true};
        std::vector<std::string> out;
        auto& c = it->second;
        while (!c.inbox.empty() && out.size() < max_frames) {
            out.emplace_back(std::move(c.inbox.front()));
            c.inbox.pop_front();
        }
        bool closed = c.closed && c.inbox.empty();
        return {std::move(out), closed};
    }

    // flush pending writes, then close (reference soft-close semantics)
    void soft_close(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return;
        it->second.soft_closing = true;
        wake();
    }

    void hard_close(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return;
        close_locked(it->second);
        wake();
    }

    // drop Python's handle; a soft-closing connection is erased by the
    // pump thread AFTER its outbox flush completes (never cut short)
    void forget(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return;
        if (it->second.fd >= 0 && it->second.soft_closing) {
            it->second.forget_pending = true;
            wake();
            return;
        }
        if (it->second.fd >= 0) close_locked(it->second);
        conns_.erase(it);
    }

    std::pair<uint64_t, uint64_t> byte_counters(int64_t id) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = conns_.find(id);
        if (it == conns_.end()) return {0, 0};
        return {it->second.in_bytes, it->second.out_bytes};
    }

private:
    static constexpr uint64_t kWakeToken = ~0ull;

    void wake() {
        uint64_t one = 1;
        ssize_t r = write(wakefd_, &one, 8);
        (void)r;
    }

    void notify_python() {
        uint64_t one = 1;
        ssize_t r = write(evfd_, &one, 8);
        (void)r;
    }

    // parse one drained ring, restore per-tick arrival order, and COALESCE
    // all frames into a single buffer (one big send() instead of one
    // syscall per delivery).  Ring write order is claim order and K5b's
    // atomic direct-delivery claims may interleave within a tick — the seq
    // header restores arrival order (wrap-aware), same as the Python drain
    // (gpu_engine.parse_ring_records).  Broadcast-only rings are already
    // in order, so the common case skips the sort entirely.  No lock
    // needed: reads caller memory, writes caller-owned `out`.
    //
    // By-reference records ({u32 len | kRefFlag, u32 seq, u64 ref_off}, no
    // payload in the ring; gpu_engine.py "by-reference delivery") take
    // their frame body from ref + ref_off.  One whose range leaves
    // [0, ref_len) ends parsing like a malformed inline record; without a
    // reference buffer the inline length check already stops at the flag.
    static constexpr uint32_t kRefFlag = 0x80000000u;
    static std::pair<int64_t, int64_t> build_ring_frames(const uint8_t* ring, size_t wpos,
                                                         std::string* out,
                                                         const uint8_t* ref = nullptr,
                                                         size_t ref_len = 0) {
        int64_t n = 0, payload_bytes = 0;
        size_t pos = 0;
        std::vector<std::pair<uint32_t, std::pair<const uint8_t*, uint32_t>>> recs;  // seq -> (src, len)
        bool ordered = true;
        while (pos + 16 <= wpos) {
            uint32_t len, seq;
            memcpy(&len, ring + pos, 4);
            memcpy(&seq, ring + pos + 4, 4);
            const uint8_t* src;
            size_t stride;
            if (ref != nullptr && (len & kRefFlag)) {
                len &= ~kRefFlag;
                uint64_t ref_off;
                memcpy(&ref_off, ring + pos + 8, 8);
                if (len > kMaxMessageSize || ref_off > ref_len || len > ref_len - ref_off) break;
                src = ref + ref_off;
                stride = 16;
            } else {
                if (len > kMaxMessageSize || pos + 16 + len > wpos) break;
                src = ring + pos + 16;
                stride = 16 + (((size_t)len + 15) & ~(size_t)15);
            }
            if (!recs.empty() && (uint32_t)(seq - recs.back().first) > 0x80000000u)
                ordered = false;
            recs.push_back({seq, {src, len}});
            ++n;
            payload_bytes += (int64_t)len;
            pos += stride;
        }
        if (!ordered && recs.size() > 1) {
            uint32_t base = recs[0].first;
            for (auto& r : recs) if (r.first - base > 0x80000000u) base = r.first;
            std::stable_sort(recs.begin(), recs.end(),
                             [base](const auto& x, const auto& y) {
                                 return (uint32_t)(x.first - base) < (uint32_t)(y.first - base);
                             });
        }
        if (n) {
            out->resize((size_t)payload_bytes + 4 * (size_t)n);
            size_t w = 0;
            for (auto& r : recs) {
                uint32_t be = htonl(r.second.second);
                memcpy(&(*out)[w], &be, 4);
                memcpy(&(*out)[w + 4], r.second.first, r.second.second);
                w += 4 + r.second.second;
            }
        }
        return {n, payload_bytes};
    }

    void close_locked(Conn& c) {
        if (c.fd >= 0) {
            epoll_ctl(epfd_, EPOLL_CTL_DEL, c.fd, nullptr);
            ::close(c.fd);
            c.fd = -1;
        }
        c.closed = true;
    }

    void update_interest(int64_t id, Conn& c) {
        if (c.fd < 0) return;
        struct epoll_event ev {};
        ev.events = (c.paused ? 0 : EPOLLIN) | (c.want_write ? EPOLLOUT : 0);
        ev.data.u64 = (uint64_t)id;
        epoll_ctl(epfd_, EPOLL_CTL_MOD, c.fd, &ev);
    }

    // finish the frame in flight: route it to the inbox / ingest buffer
    void complete_frame(Conn& c) {
        if (c.ingest) {
            c.imeta.push_back(classify_frame((const uint8_t*)c.frame.data(),
                                             c.frame.size()));
            c.ibuf.append(c.frame);
            c.ioffs.push_back((int64_t)c.ibuf.size());
            c.frame.clear();
        } else {
            c.inbox.emplace_back(std::move(c.frame));
            c.frame = std::string();
        }
        c.frame_have = 0;
        c.frame_need = 0;
        c.hdr_have = 0;
    }

    // reads everything available; returns true if new complete frames landed
    bool do_read(Conn& c) {
        bool new_frames = false;
        static thread_local std::vector<char> tmpv(1 << 20);
        char* tmp = tmpv.data();
        while (true) {
            ssize_t n;
            if (c.frame_need > 0 && c.frame_need - c.frame_have >= (64 << 10)) {
                // big body: receive straight into the destination buffer
                n = ::recv(c.fd, &c.frame[c.frame_have], c.frame_need - c.frame_have, 0);
                if (n > 0) {
                    c.in_bytes += (uint64_t)n;
                    c.frame_have += (size_t)n;
                    if (c.frame_have == c.frame_need) {
                        complete_frame(c);
                        new_frames = true;
                    }
                    continue;
                }
            } else {
                n = ::recv(c.fd, tmp, tmpv.size(), 0);
                if (n > 0) {
                    c.in_bytes += (uint64_t)n;
                    size_t off = 0;
                    while (off < (size_t)n) {
                        if (c.frame_need == 0) {
                            size_t take = std::min((size_t)n - off, 4 - c.hdr_have);
                            memcpy(c.hdr + c.hdr_have, tmp + off, take);
                            c.hdr_have += take;
                            off += take;
                            if (c.hdr_have < 4) break;
                            uint32_t be;
                            memcpy(&be, c.hdr, 4);
                            uint64_t len = ntohl(be);
                            if (len > kMaxMessageSize) { close_locked(c); return true; }
                            c.frame_need = len;
                            c.frame_have = 0;
                            c.frame.resize(len);
                            if (len == 0) {
                                complete_frame(c);
                                new_frames = true;
                            }
                            continue;
                        }
                        size_t take = std::min((size_t)n - off,
                                               (size_t)(c.frame_need - c.frame_have));
                        memcpy(&c.frame[c.frame_have], tmp + off, take);
                        c.frame_have += take;
                        off += take;
                        if (c.frame_have == c.frame_need) {
                            complete_frame(c);
                            new_frames = true;
                        }
                    }
                    if (c.ingest && c.ibuf.size() > kIngestPauseBytes) {
                        c.paused = true;  // re-armed by recv_ingest's drain
                        break;
                    }
                    if (n < (ssize_t)tmpv.size()) continue;  // might be more
                    continue;
                }
            }
            if (n == 0) {
                close_locked(c);
                return true;
            }
            if (errno == EAGAIN || errno == EWOULDBLOCK) break;
            if (errno == EINTR) continue;
            close_locked(c);
            return true;
        }
        return new_frames;
    }

    // writes as much of the outbox as the socket accepts
    void do_write(Conn& c) {
        while (!c.outbox.empty()) {
            auto& front = c.outbox.front();
            ssize_t n = ::send(c.fd, front.data() + c.out_off,
                               front.size() - c.out_off, MSG_NOSIGNAL);
            if (n > 0) {
                c.out_bytes += (uint64_t)n;
                c.out_off += (size_t)n;
                if (c.out_off == front.size()) {
                    c.outbox.pop_front();
                    c.out_off = 0;
                }
            } else {
                if (errno == EAGAIN || errno == EWOULDBLOCK) return;
                if (errno == EINTR) continue;
                close_locked(c);
                return;
            }
        }
        c.want_write = false;
        if (c.soft_closing) close_locked(c);
    }

    void run() {
        std::vector<struct epoll_event> evs(256);
        while (!stopping_.load()) {
            int n = epoll_wait(epfd_, evs.data(), (int)evs.size(), 200);
            if (n < 0) {
                if (errno == EINTR) continue;
                break;
            }
            bool notify = false;
            std::lock_guard<std::mutex> g(mu_);
            // service wakeups (new outbox content / soft closes)
            for (int i = 0; i < n; ++i) {
                if (evs[i].data.u64 == kWakeToken) {
                    uint64_t junk;
                    while (read(wakefd_, &junk, 8) == 8) {}
                    continue;
                }
                int64_t id = (int64_t)evs[i].data.u64;
                auto it = conns_.find(id);
                if (it == conns_.end()) continue;
                Conn& c = it->second;
                if (c.fd < 0) continue;
                if (evs[i].events & (EPOLLIN | EPOLLHUP | EPOLLERR)) {
                    bool was_closed = c.closed;
                    bool frames = do_read(c);
                    if (c.fd >= 0 && c.paused) update_interest(id, c);  // park EPOLLIN
                    if (frames || (c.closed && !was_closed)) {
                        notify = true;
                        dirty_.insert(id);
                    }
                }
                if (c.fd >= 0 && (evs[i].events & EPOLLOUT)) do_write(c);
            }
            // apply pending write interest / flush fresh outboxes
            std::vector<int64_t> to_erase;
            for (auto& kv : conns_) {
                Conn& c = kv.second;
                if (c.fd < 0) {
                    if (c.forget_pending) to_erase.push_back(kv.first);
                    continue;
                }
                if (c.want_write || c.soft_closing) {
                    do_write(c);  // opportunistic immediate flush
                    if (c.fd >= 0) update_interest(kv.first, c);
                    if (c.closed) { notify = true; dirty_.insert(kv.first); }
                }
            }
            for (int64_t id : to_erase) conns_.erase(id);
            if (notify) notify_python();
        }
    }

    int epfd_ = -1, evfd_ = -1, wakefd_ = -1;
    std::atomic<bool> stopping_{false};
    std::thread thread_;
    std::mutex mu_;
    std::map<int64_t, Conn> conns_;
    std::set<int64_t> dirty_;
    int64_t next_id_ = 1;
};

}  // namespace net
