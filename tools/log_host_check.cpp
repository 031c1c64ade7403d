// log_host_check.cpp — the log messages' headers (statsd-router_amd/csrc/log_host.hpp) against snprintf with the
// reference's format strings (sr-main.c:91,102,115,142,174,184), as a stand-alone host program for a
// sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -o log_host_check tools/log_host_check.cpp && ./log_host_check
// Every header is written into a buffer of exactly kLogMaxHeader bytes on the heap, so one byte too many is
// an error the sanitizer reports. Prints "ok" or the first difference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../statsd-router_amd/csrc/log_host.hpp"

using namespace srk;

static int check(uint32_t kind, uint64_t hash, uint32_t len, uint32_t route) {
    char want[256];
    int n;
    switch (kind) {
    case LOG_GOT_PACKET: n = snprintf(want, sizeof want, "%s: got packet ", "udp_read_cb"); break;
    case LOG_BAD_LENGTH: n = snprintf(want, sizeof want, "%s: invalid length %d of metric ", "udp_read_cb", (int)len); break;
    case LOG_BAD_FORMAT: n = snprintf(want, sizeof want, "%s: invalid metric ", "process_data_line"); break;
    case LOG_HASH:
        n = snprintf(want, sizeof want, "%s: hash = %lx, length = %d, line = ", "find_downstream", (unsigned long)hash, (int)len);
        break;
    case LOG_PUSH: n = snprintf(want, sizeof want, "%s: pushing to downstream %d", "find_downstream", (int)route); break;
    default: n = snprintf(want, sizeof want, "%s: all downstreams are dead", "find_downstream"); break;
    }
    uint8_t *got = (uint8_t *)malloc(kLogMaxHeader);
    const uint32_t k = log_header(got, kind, hash, len, route);
    const int bad = k != (uint32_t)n || k != log_header_len(kind, hash, len, route) || k > kLogMaxHeader || memcmp(got, want, k) != 0;
    if (bad) printf("kind %u hash %llx len %u route %u: got %u bytes, want %d: %s\n", kind, (unsigned long long)hash, len, route, k, n, want);
    free(got);
    return bad;
}

int main() {
    static const uint64_t hashes[] = {0, 1, 9, 0xa, 0xf, 0x10, 0xff, 0x100, 0xabcdef, 0xffffffffull, 0x100000000ull,
                                      0x7fffffffffffffffull, 0x8000000000000000ull, 0xfedcba9876543210ull, ~0ull};
    static const uint32_t nums[] = {0, 1, 5, 6, 9, 10, 99, 100, 999, 1000, 1449, 1450, 4096, 9999, 10000, 65532, 65535};
    for (uint32_t kind = 0; kind <= LOG_DEAD; ++kind)
        for (uint64_t h : hashes)
            for (uint32_t a : nums)
                for (uint32_t b : nums)
                    if (check(kind, h, a, b)) return 1;
    for (int i = 0; i < 64; ++i)
        if (check(LOG_HASH, 1ull << i, 1449, 0) || check(LOG_HASH, (1ull << i) - 1, 6, 0)) return 1;
    if (log_keep(35, 65, 4096, 0) != 4196 || log_keep(35, 65, 4096, 2047) != 2047 || log_keep(0, 24, 0, 2047) != 24 ||
        log_keep(2, 41, 0, 43) != 43 || log_keep(2, 41, 0, 42) != 42) {
        printf("log_keep\n");
        return 1;
    }
    if (!log_kind_warn(LOG_BAD_LENGTH) || !log_kind_warn(LOG_BAD_FORMAT) || !log_kind_warn(LOG_DEAD) || log_kind_warn(LOG_GOT_PACKET) ||
        log_kind_warn(LOG_HASH) || log_kind_warn(LOG_PUSH)) {
        printf("log_kind_warn\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
