// coalesce_host.hpp — the host part of the plain-counter coalescing (include/sr_route.h): the
// grammar of a plain counter, the decimal text of a sum and the configuration's limits. The kernels use the same
// functions (SRK_HD), so the device cannot disagree with sr_coalesce_parse / sr_coalesce_format. No HIP here: a
// host program can include this file alone (tools/coalesce_host_check.cpp).
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#include "stats_host.hpp"

namespace srk {

constexpr uint32_t kCoalesceMinLine = SR_MIN_LINE_LENGTH, kCoalesceMaxLine = SR_MAX_LINE_LENGTH;
constexpr uint32_t kCoalesceMaxDigits = 9;       // of a value: it fits an int32
constexpr uint32_t kCoalesceMaxTail = 24;        // ':' + '-' + 19 digits + "|c\n"
static_assert(SR_COALESCE_NAME_MAX + kCoalesceMaxTail == kCoalesceMaxLine, "the longest merged line is a valid line");

// The plain-counter test on one line of len bytes, '\n' included: <name>:-?[0-9]{1,9}|c\n with the ':' the
// line's first and 1 <= name bytes <= SR_COALESCE_NAME_MAX. Read from the end: the grammar behind the ':' holds
// no ':' itself, so the ':' in front of the number is the first one iff the name holds none. Only bytes of
// [line, line + len) are read.
SRK_HD bool coalesce_parse(const uint8_t *line, uint32_t len, uint32_t *name_len, int32_t *value) {
    if (len < kCoalesceMinLine || len > kCoalesceMaxLine) return false;
    if (line[len - 1u] != (uint8_t)'\n' || line[len - 2u] != (uint8_t)'c' || line[len - 3u] != (uint8_t)'|') return false;
    int p = (int)len - 4;   // >= 2
    uint32_t mag = 0, unit = 1, nd = 0;
    while (nd < kCoalesceMaxDigits && p >= 0) {
        const uint32_t d = (uint32_t)line[p] - (uint32_t)'0';
        if (d > 9u) break;
        mag += d * unit;
        unit *= 10u;
        ++nd;
        --p;
    }
    if (nd == 0 || p < 0) return false;
    const bool neg = line[p] == (uint8_t)'-';
    if (neg && --p < 0) return false;
    if (line[p] != (uint8_t)':') return false;   // a tenth digit, a '+', a '.', ... end here
    const uint32_t k = (uint32_t)p;
    if (k < 1u || k > SR_COALESCE_NAME_MAX) return false;
    for (uint32_t q = 0; q < k; ++q)
        if (line[q] == (uint8_t)':') return false;
    *name_len = k;
    *value = neg ? -(int32_t)mag : (int32_t)mag;
    return true;
}

// The bytes of dec(sum): 1..19 digits and a '-' for a negative sum (|sum| < 2^63).
SRK_HD uint32_t coalesce_dec_len(int64_t sum) {
    uint64_t mag = sum < 0 ? 0ull - (uint64_t)sum : (uint64_t)sum;
    uint32_t n = 1;
    while (mag >= 10ull) {
        mag /= 10ull;
        ++n;
    }
    return n + (sum < 0 ? 1u : 0u);
}

// The length of the merged line of a name of k bytes: name ':' dec(sum) "|c\n".
SRK_HD uint32_t coalesce_line_len(uint32_t k, int64_t sum) { return k + 1u + coalesce_dec_len(sum) + 3u; }

// What follows the name in a merged line, ':' dec(sum) "|c\n", to dst: of its bytes only those below `room` are
// written (the device stops at the caller's append_cap). No array, no table: a digit goes straight to its place.
SRK_HD uint32_t coalesce_put_tail(uint8_t *dst, uint64_t room, int64_t sum) {
    const uint32_t dl = coalesce_dec_len(sum);
    uint64_t mag = sum < 0 ? 0ull - (uint64_t)sum : (uint64_t)sum;
    if (0u < room) dst[0] = (uint8_t)':';
    if (sum < 0 && 1u < room) dst[1] = (uint8_t)'-';
    const uint32_t first = sum < 0 ? 2u : 1u;   // the first digit's place
    for (uint32_t at = dl; at >= first; --at) {   // dec(sum) is dst[1 .. dl]: the last digit first (first >= 1)
        if (at < room) dst[at] = (uint8_t)('0' + (uint32_t)(mag % 10ull));
        mag /= 10ull;
    }
    const uint32_t e = 1u + dl;
    if (e < room) dst[e] = (uint8_t)'|';
    if (e + 1u < room) dst[e + 1u] = (uint8_t)'c';
    if (e + 2u < room) dst[e + 2u] = (uint8_t)'\n';
    return e + 3u;
}

// 0 selects the default; else a power of two within the limits. Returns 0 or -EINVAL.
inline int coalesce_resolve(const sr_coalesce_config *in, uint32_t *slots) {
    const uint32_t s = (in && in->slots) ? in->slots : SR_COALESCE_DEFAULT_SLOTS;
    if (s < SR_COALESCE_MIN_SLOTS || s > SR_COALESCE_MAX_SLOTS || (s & (s - 1u))) return -EINVAL;
    *slots = s;
    return 0;
}

inline int coalesce_parse_line(const uint8_t *line, size_t len, uint32_t *name_len, int64_t *value) {
    uint32_t k = 0;
    int32_t v = 0;
    if (!line || len > kCoalesceMaxLine || !coalesce_parse(line, (uint32_t)len, &k, &v)) return 0;
    if (name_len) *name_len = k;
    if (value) *value = v;
    return 1;
}

inline size_t coalesce_format_line(uint8_t *dst, const uint8_t *name, uint32_t name_len, int64_t sum) {
    for (uint32_t q = 0; q < name_len; ++q) dst[q] = name[q];
    return (size_t)name_len + coalesce_put_tail(dst + name_len, ~0ull, sum);
}

}  // namespace srk
