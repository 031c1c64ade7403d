// frame_host_check.cpp — the host arithmetic of device framing on the CPU, under sanitizers.
//
// Includes only statsd-router_amd/csrc/frame_host.hpp (the framed size and ends of datagrams left in their
// slots) and host/sr_slots.h (the offset-to-slot search the router core uses to find a framed line in its
// slot). Every arena is a heap block of exactly the bytes the contract names, so a read past a datagram's
// kept bytes or past the ends is an AddressSanitizer report. Built and run by
// tests/test_frame_host_check.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o frame_host_check tools/frame_host_check.cpp
// Exit status 0 and "ok" on stdout: every check passed.
#include "../host/sr_slots.h"
#include "../statsd-router_amd/csrc/frame_host.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace srk;

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint32_t rnd(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

// udp_read_cb's framing, written out the slow way (sr-main.c:163-173)
static void frame_ref(std::vector<uint8_t> &out, const uint8_t *src, size_t len) {
    const size_t n = len < 4095 ? len : 4095;
    if (n == 0) return;
    out.insert(out.end(), src, src + n);
    if (src[n - 1] != '\n') out.push_back('\n');
}

// One arena of datagrams with the given lengths, `stride` apart, every one ending (or not) in '\n'.
static void run_case(const std::vector<uint32_t> &lengths, size_t stride, int newline_mode, uint64_t seed) {
    const size_t count = lengths.size();
    std::vector<uint16_t> lens(count);
    size_t bytes = 0;
    for (size_t j = 0; j < count; ++j) {
        lens[j] = (uint16_t)(lengths[j] < 65535 ? lengths[j] : 65535);
        const size_t kept = lengths[j] < 4095 ? lengths[j] : 4095;
        if (kept) bytes = j * stride + kept;   // the arena ends with the last kept byte
    }
    uint8_t *arena = (uint8_t *)malloc(bytes ? bytes : 1);
    CHECK(arena);
    memset(arena, 0xA5, bytes ? bytes : 1);
    std::vector<uint8_t> want;
    std::vector<uint32_t> want_ends(count);
    for (size_t j = 0; j < count; ++j) {
        const size_t kept = lengths[j] < 4095 ? lengths[j] : 4095;
        uint8_t *d = arena + j * stride;
        for (size_t i = 0; i < kept; ++i) d[i] = (uint8_t)rnd(seed);
        if (kept) {
            const int nl = newline_mode == 2 ? (int)(rnd(seed) & 1u) : newline_mode;
            d[kept - 1] = nl ? (uint8_t)'\n' : (uint8_t)(d[kept - 1] == '\n' ? 'x' : d[kept - 1]);
        }
        frame_ref(want, d, kept);
        want_ends[j] = (uint32_t)want.size();
    }
    // sizes and ends; ends == NULL gives the same total
    uint32_t *ends = (uint32_t *)malloc((count ? count : 1) * sizeof(uint32_t));
    CHECK(ends);
    CHECK(frame_slots_size(arena, stride, lens.data(), count, ends) == want.size());
    CHECK(frame_slots_size(arena, stride, lens.data(), count, nullptr) == want.size());
    for (size_t j = 0; j < count; ++j) CHECK(ends[j] == want_ends[j]);
    // every datagram's first and last framed byte map back to it, and to the right byte of its slot; runs
    // of empty datagrams are never the answer
    for (size_t j = 0; j < count; ++j) {
        const uint32_t start = j ? ends[j - 1] : 0u, end = ends[j];
        if (end == start) continue;
        const uint32_t probes[3] = {start, end - 1u, start + (end - start) / 2u};
        for (uint32_t off : probes) {
            CHECK(sr_slot_of(ends, count, off) == j);
            const size_t kept = lengths[j] < 4095 ? lengths[j] : 4095;
            const uint32_t in = off - start;
            const uint8_t *at = sr_slot_addr(arena, stride, ends, count, off);
            CHECK(at == arena + j * stride + in);
            if (in < kept) CHECK(*at == want[off]);
            else CHECK(in == kept && want[off] == '\n');   // the appended byte: the core writes it into the slot
        }
    }
    if (count && ends[count - 1]) CHECK(sr_slot_of(ends, count, ends[count - 1] - 1u) < count);
    free(ends);
    free(arena);
}

int main() {
    const std::vector<uint32_t> edges = {0, 1, 2, 15, 16, 17, 4094, 4095, 4096, 5000, 65535};
    for (size_t stride : {(size_t)4096, (size_t)4097, (size_t)4111, (size_t)70000})
        for (int mode = 0; mode < 3; ++mode) {
            run_case(edges, stride, mode, 1 + mode);
            std::vector<uint32_t> rev(edges.rbegin(), edges.rend());
            run_case(rev, stride, mode, 7 + mode);
        }
    // runs of empty datagrams: at the front, in the middle, at the end, and nothing else
    run_case({0, 0, 0, 5, 0, 0, 1, 1, 0, 0, 0, 4095, 0}, 4096, 2, 21);
    run_case({0, 0, 0, 0}, 4096, 0, 22);
    run_case({}, 4096, 0, 23);
    run_case({1}, 4096, 1, 24);   // a datagram that is just "\n"
    run_case({1}, 4096, 0, 25);
    // only 1-byte datagrams, and a long random mix
    run_case(std::vector<uint32_t>(300, 1u), 4096, 2, 26);
    uint64_t s = 99;
    std::vector<uint32_t> mix(2000);
    for (auto &v : mix) v = (rnd(s) % 7 == 0) ? 0u : rnd(s) % 5000u;
    run_case(mix, 4096, 2, 27);
    puts("ok");
    return 0;
}
