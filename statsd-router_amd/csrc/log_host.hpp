// log_host.hpp — the log messages' constant texts and number formats (no HIP, no libc beyond the fixed-width
// types), shared by the device formatter (log_kernel.hpp) and by stand-alone host programs.
//
// A message is prefix[level] + header + span + '\n' (DESIGN.md §5.8). The header is everything the reference
// prints before its final "%.*s": the constant text and the numbers ("%lx": lower-case hex without leading
// zeros; "%d": decimal). The span is a run of input bytes cut before its first NUL. Texts as
// host/sr_core.c:254-309 (sr-main.c:91,102,115,142,174,184).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SR_LOG_HD __host__ __device__ inline
#else
#define SR_LOG_HD inline
#endif

namespace srk {

constexpr uint32_t kLogMaxPrefix = 256;   // bytes of one caller-supplied prefix
constexpr uint32_t kLogMaxHeader = 65;    // "find_downstream: hash = " + 16 + ", length = " + 5 + ", line = "
constexpr uint32_t kLogMaxBatch = 1u << 30;   // a group's byte sums stay below 2^32

enum LogKind : uint32_t {
    LOG_GOT_PACKET = 0,   // TRACE udp_read_cb: got packet <datagram>
    LOG_BAD_LENGTH = 1,   // WARN  udp_read_cb: invalid length %d of metric <line with '\n'>
    LOG_BAD_FORMAT = 2,   // WARN  process_data_line: invalid metric <line without '\n'>
    LOG_HASH = 3,         // TRACE find_downstream: hash = %lx, length = %d, line = <line with '\n'>
    LOG_PUSH = 4,         // TRACE find_downstream: pushing to downstream %d
    LOG_DEAD = 5,         // WARN  find_downstream: all downstreams are dead
};

// 0: TRACE, 1: WARN (the index of the message's prefix)
SR_LOG_HD uint32_t log_kind_warn(uint32_t kind) { return kind == LOG_BAD_LENGTH || kind == LOG_BAD_FORMAT || kind == LOG_DEAD; }

SR_LOG_HD uint32_t log_dec_digits(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}

SR_LOG_HD uint32_t log_hex_digits(uint64_t v) {
    uint32_t n = 1;
    while (v >>= 4) ++n;
    return n;
}

SR_LOG_HD uint32_t log_put(uint8_t *dst, uint32_t at, const char *s, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) dst[at + i] = (uint8_t)s[i];
    return at + n;
}

SR_LOG_HD uint32_t log_put_dec(uint8_t *dst, uint32_t at, uint32_t v) {
    const uint32_t n = log_dec_digits(v);
    for (uint32_t i = n; i-- > 0;) {
        dst[at + i] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return at + n;
}

SR_LOG_HD uint32_t log_put_hex(uint8_t *dst, uint32_t at, uint64_t v) {
    const uint32_t n = log_hex_digits(v);
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t d = (uint32_t)(v & 15u);
        dst[at + i] = (uint8_t)(d < 10u ? '0' + d : 'a' + (d - 10u));
        v >>= 4;
    }
    return at + n;
}

// the header's length: what log_header writes
SR_LOG_HD uint32_t log_header_len(uint32_t kind, uint64_t hash, uint32_t len, uint32_t route) {
    switch (kind) {
    case LOG_GOT_PACKET: return 24u;
    case LOG_BAD_LENGTH: return 28u + log_dec_digits(len) + 11u;
    case LOG_BAD_FORMAT: return 34u;
    case LOG_HASH: return 24u + log_hex_digits(hash) + 11u + log_dec_digits(len) + 9u;
    case LOG_PUSH: return 39u + log_dec_digits(route);
    default: return 41u;
    }
}

// the header into dst (room kLogMaxHeader); returns its length
SR_LOG_HD uint32_t log_header(uint8_t *dst, uint32_t kind, uint64_t hash, uint32_t len, uint32_t route) {
    uint32_t at = 0;
    switch (kind) {
    case LOG_GOT_PACKET: return log_put(dst, at, "udp_read_cb: got packet ", 24u);
    case LOG_BAD_LENGTH:
        at = log_put(dst, at, "udp_read_cb: invalid length ", 28u);
        at = log_put_dec(dst, at, len);
        return log_put(dst, at, " of metric ", 11u);
    case LOG_BAD_FORMAT: return log_put(dst, at, "process_data_line: invalid metric ", 34u);
    case LOG_HASH:
        at = log_put(dst, at, "find_downstream: hash = ", 24u);
        at = log_put_hex(dst, at, hash);
        at = log_put(dst, at, ", length = ", 11u);
        at = log_put_dec(dst, at, len);
        return log_put(dst, at, ", line = ", 9u);
    case LOG_PUSH:
        at = log_put(dst, at, "find_downstream: pushing to downstream ", 39u);
        return log_put_dec(dst, at, route);
    default: return log_put(dst, at, "find_downstream: all downstreams are dead", 41u);
    }
}

// bytes of one message on the wire: prefix + header + span cut to max_msg (0: no cut), then '\n'
SR_LOG_HD uint32_t log_keep(uint32_t plen, uint32_t hlen, uint32_t slen, uint32_t max_msg) {
    const uint32_t full = plen + hlen + slen;
    return max_msg && full > max_msg ? max_msg : full;
}

}  // namespace srk
