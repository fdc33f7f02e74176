// Stand-alone test of the pump's framed-drain entry points
// (Pump::check_frames, Pump::send_framed_batch) over seeded, mutated buffers.
// Every buffer handed over is a heap allocation of exactly its length, so a
// read past the end is an AddressSanitizer report when this is built with
// -fsanitize=address,undefined (tests/test_framed_native.py does).

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <sys/socket.h>
#include <unistd.h>

#include "../net/pump.h"

static int checks = 0;
#define CHECK(x)                                                                    \
    do {                                                                            \
        if (!(x)) {                                                                 \
            fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                               \
        }                                                                           \
        ++checks;                                                                   \
    } while (0)

using Buf = std::vector<uint8_t>;

// The specification, written the slow way: split, then compare.
static bool naive_check(const Buf& b, int64_t cnt) {
    size_t pos = 0;
    int64_t n = 0;
    while (pos != b.size()) {
        if (b.size() - pos < 4) return false;
        uint64_t len = ((uint64_t)b[pos] << 24) | ((uint64_t)b[pos + 1] << 16)
                       | ((uint64_t)b[pos + 2] << 8) | b[pos + 3];
        if (len > net::kMaxMessageSize) return false;
        if (len > b.size() - pos - 4) return false;
        pos += 4 + (size_t)len;
        ++n;
    }
    return n == cnt;
}

static Buf frames(std::mt19937& rng, int64_t* cnt) {
    Buf out;
    *cnt = (int64_t)(rng() % 9);
    for (int64_t i = 0; i < *cnt; ++i) {
        uint32_t len = (rng() % 4 == 0) ? 0 : (uint32_t)(rng() % 300);
        out.push_back((uint8_t)(len >> 24));
        out.push_back((uint8_t)(len >> 16));
        out.push_back((uint8_t)(len >> 8));
        out.push_back((uint8_t)len);
        for (uint32_t k = 0; k < len; ++k) out.push_back((uint8_t)rng());
    }
    return out;
}

static bool pump_check(const Buf& b, int64_t cnt) {
    // an exact-size copy: data() of an empty vector may be null, which is fine
    Buf copy(b);
    return net::Pump::check_frames(copy.data(), copy.size(), cnt);
}

static int test_check_frames() {
    std::mt19937 rng(0xF7A3ED);
    int accepted = 0, refused = 0;
    for (int round = 0; round < 4000; ++round) {
        int64_t cnt;
        Buf good = frames(rng, &cnt);
        CHECK(pump_check(good, cnt));
        CHECK(!pump_check(good, cnt + 1));
        CHECK(!pump_check(good, -1));
        if (cnt > 0) CHECK(!pump_check(good, cnt - 1));
        Buf bad = good;
        switch (rng() % 5) {
        case 0:   // flip a bit anywhere (a body bit leaves it valid)
            if (!bad.empty()) bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
            break;
        case 1:   // cut the tail
            if (!bad.empty()) bad.resize(rng() % bad.size());
            break;
        case 2:   // trailing partial frame
            for (unsigned k = 1 + rng() % 6; k > 0; --k) bad.push_back((uint8_t)(rng() % 3));
            break;
        case 3:   // a huge prefix at the front
            if (bad.size() >= 4) { bad[0] = 0xFF; bad[1] = (uint8_t)rng(); }
            break;
        default:  // random bytes
            bad.assign(rng() % 64, 0);
            for (auto& x : bad) x = (uint8_t)(rng() % 4);
            break;
        }
        for (int64_t c = cnt - 1; c <= cnt + 1; ++c) {
            const bool want = c >= 0 && naive_check(bad, c);
            CHECK(pump_check(bad, c) == want);
            want ? ++accepted : ++refused;
        }
    }
    CHECK(accepted > 100 && refused > 1000);   // both sides were exercised
    return 0;
}

static bool read_exact(int fd, size_t n, std::string* out) {
    out->resize(n);
    size_t have = 0;
    while (have < n) {
        ssize_t r = ::read(fd, &(*out)[have], n - have);
        if (r <= 0) return false;
        have += (size_t)r;
    }
    return true;
}

static int test_send_framed_batch() {
    std::mt19937 rng(20240611);
    net::Pump pump;
    int sv[2];
    CHECK(socketpair(AF_UNIX, SOCK_STREAM, 0, sv) == 0);
    int64_t id = pump.add(sv[0]);
    int gone_sv[2];
    CHECK(socketpair(AF_UNIX, SOCK_STREAM, 0, gone_sv) == 0);
    int64_t gone = pump.add(gone_sv[0]);
    pump.hard_close(gone);
    std::string expect;
    for (int round = 0; round < 300; ++round) {
        // three entries in one staging buffer: good, mutated, good
        int64_t c0, c1, c2;
        Buf a = frames(rng, &c0), b = frames(rng, &c1), c = frames(rng, &c2);
        if (!b.empty()) b[rng() % b.size()] ^= 0x80;
        if (rng() % 2) b.push_back(1);
        Buf staging;
        staging.insert(staging.end(), a.begin(), a.end());
        staging.insert(staging.end(), b.begin(), b.end());
        staging.insert(staging.end(), c.begin(), c.end());
        const bool b_ok = naive_check(b, c1);
        auto out = pump.send_framed_batch(
            staging.data(), {id, id, id, gone},
            {0, (int64_t)a.size(), (int64_t)(a.size() + b.size()), 0},
            {(int64_t)a.size(), (int64_t)b.size(), (int64_t)c.size(), (int64_t)a.size()},
            {c0, c1, c2, c0});
        CHECK(out.size() == 8);
        CHECK(out[0] == c0 && out[1] == (int64_t)a.size() - 4 * c0);
        if (b_ok) CHECK(out[2] == c1 && out[3] == (int64_t)b.size() - 4 * c1);
        else CHECK(out[2] == -2 && out[3] == 0);
        CHECK(out[4] == c2 && out[5] == (int64_t)c.size() - 4 * c2);
        CHECK(out[6] == -1 && out[7] == 0);
        expect.append((const char*)a.data(), a.size());
        if (b_ok) expect.append((const char*)b.data(), b.size());
        expect.append((const char*)c.data(), c.size());
    }
    // a ring-mode entry: two records out of order
    Buf ring(64, 0);
    const uint32_t l0 = 3, s0 = 9, l1 = 2, s1 = 8;
    memcpy(&ring[0], &l0, 4);  memcpy(&ring[4], &s0, 4);  memcpy(&ring[16], "abc", 3);
    memcpy(&ring[32], &l1, 4); memcpy(&ring[36], &s1, 4); memcpy(&ring[48], "de", 2);
    auto out = pump.send_framed_batch(ring.data(), {id}, {0}, {64}, {-1});
    CHECK(out[0] == 2 && out[1] == 5);
    expect.append(std::string("\0\0\0\2de\0\0\0\3abc", 13));
    // everything accepted arrives, byte for byte, and nothing else
    std::string got;
    CHECK(read_exact(sv[1], expect.size(), &got));
    CHECK(got == expect);
    pump.soft_close(id);
    char extra;
    CHECK(::read(sv[1], &extra, 1) == 0);      // EOF: not one stray byte
    ::close(sv[1]);
    ::close(gone_sv[1]);
    pump.stop();
    return 0;
}

int main() {
    if (test_check_frames()) return 1;
    if (test_send_framed_batch()) return 1;
    printf("framed pump OK: %d checks\n", checks);
    return 0;
}
