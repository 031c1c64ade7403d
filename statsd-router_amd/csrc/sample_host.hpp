// sample_host.hpp — the host part of the sample-rate stage (include/sr_route.h): whether a line is
// sampleable and where the rate goes in, the ladder, the keep rule, the rate texts, the rewrite, the configuration's
// check and the SR_SAMPLE spec. The count and the sum kernels run the very same functions (SRK_HD) over the very same
// 16-byte steps, so the device cannot disagree with sr_sample_parse, sr_sample_step and sr_sample_keep. No HIP here:
// a host program can include this file alone (tools/sample_host_check.cpp).
//
// A line's content (its bytes without the final '\n') is taken in steps of 16 bytes, four little-endian dwords. Per
// step two 16-bit masks are built with SWAR on the dwords, ':' and '|'. The parse is a small machine over them:
//   COLON  up to the first ':' (p; p == 0 fails);
//   PIPE   up to the first '|' behind it (q; q == p + 1 fails: the value is empty);
//   TYPE   the bytes up to the next '|' (e) or the content's end, at most two of them, shifted into a code;
//   HASH   the one byte behind e must be '#' (it may be the first byte of the next step).
// A machine that is OK or FAIL ignores further steps; nothing behind e + 1 is ever looked at.
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "stats_host.hpp"

namespace srk {

constexpr uint32_t kSampleSteps = SR_SAMPLE_STEPS;
constexpr uint32_t kSampleTypesAll = SR_SAMPLE_TYPES_ALL;
constexpr uint32_t kSampleDefaultTypes = SR_VALID_TYPE_MS | SR_VALID_TYPE_H | SR_VALID_TYPE_D;
constexpr uint64_t kSampleGolden = 0x9E3779B97F4A7C15ull;

enum : uint32_t { kSpColon = 0, kSpPipe, kSpType, kSpHash, kSpOk, kSpFail };

struct SampleState {
    uint32_t phase;
    uint32_t p;       // PIPE: the index of the first ':'
    uint32_t tcode;   // TYPE: 1, then the type's bytes shifted in from the right; all ones once there are three
    uint32_t ins;     // HASH, OK: e
    uint32_t bit;     // HASH, OK: the type's bit
};

SRK_HD void sample_begin(SampleState &s) {
    s.phase = kSpColon;
    s.p = s.ins = s.bit = 0u;
    s.tcode = 1u;
}

// 0x80 in every byte of x that is zero (exact: no borrow crosses a byte)
SRK_HD uint32_t sample_zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// the four 0x80 flags of a dword as bits 0..3
SRK_HD uint32_t sample_gather(uint32_t m) { return ((m >> 7) * 0x00204081u >> 21) & 0xFu; }

// bit i: byte i of the step equals `b`, for the first v bytes
SRK_HD uint32_t sample_mask(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t b, uint32_t v) {
    const uint32_t rep = b * 0x01010101u;
    const uint32_t m = sample_gather(sample_zero_bytes(w0 ^ rep)) | sample_gather(sample_zero_bytes(w1 ^ rep)) << 4 |
                       sample_gather(sample_zero_bytes(w2 ^ rep)) << 8 | sample_gather(sample_zero_bytes(w3 ^ rep)) << 12;
    return m & (v >= 16u ? 0xFFFFu : (1u << v) - 1u);
}

// byte i (0..15) of the step, picked by comparisons (no array, so no scratch on the device)
SRK_HD uint32_t sample_byte(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) {
    const uint32_t d = i < 4u ? w0 : i < 8u ? w1 : i < 12u ? w2 : w3;
    return (d >> (8u * (i & 3u))) & 0xFFu;
}

// the type's bit for a code, 0 for a type that is not c, ms, h or d or that `types` leaves out
SRK_HD uint32_t sample_type_bit(uint32_t tcode, uint32_t types) {
    const uint32_t bit = tcode == 0x163u ? SR_VALID_TYPE_C : tcode == 0x168u ? SR_VALID_TYPE_H
                       : tcode == 0x164u ? SR_VALID_TYPE_D : tcode == 0x16D73u ? SR_VALID_TYPE_MS : 0u;
    return bit & types;
}

// One step: bytes [base, base + v) of the content as four little-endian dwords, 1 <= v <= 16; bytes of the dwords
// behind v are ignored. Not called for a machine that is OK or FAIL.
SRK_HD void sample_step_bytes(SampleState &s, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t base,
                              uint32_t v, uint32_t types) {
    if (s.phase == kSpHash) {   // e was the last byte of the step before
        s.phase = (w0 & 0xFFu) == 0x23u ? kSpOk : kSpFail;
        return;
    }
    const uint32_t pipes = sample_mask(w0, w1, w2, w3, 0x7Cu, v);
    uint32_t from = 0u;   // the step's first byte that the next phase takes
    if (s.phase == kSpColon) {
        const uint32_t i = (uint32_t)__builtin_ctz(sample_mask(w0, w1, w2, w3, 0x3Au, v) | 0x10000u);
        if (i == 16u) return;
        s.p = base + i;
        s.phase = s.p == 0u ? kSpFail : kSpPipe;
        from = i + 1u;
    }
    if (s.phase == kSpPipe) {
        const uint32_t i = (uint32_t)__builtin_ctz((pipes >> from << from) | 0x10000u);
        if (i == 16u) return;
        s.phase = base + i == s.p + 1u ? kSpFail : kSpType;
        from = i + 1u;
    }
    if (s.phase == kSpType) {
        const uint32_t rest = pipes >> from << from;
        const uint32_t end = (uint32_t)__builtin_ctz(rest | (1u << v));   // <= v; from <= v
        const uint32_t n = end - from;
        uint32_t t = s.tcode;
        if (n >= 1u) t = t < 0x10000u ? t << 8 | sample_byte(w0, w1, w2, w3, from) : 0xFFFFFFFFu;
        if (n >= 2u) t = t < 0x10000u ? t << 8 | sample_byte(w0, w1, w2, w3, from + 1u) : 0xFFFFFFFFu;
        if (n >= 3u) t = 0xFFFFFFFFu;
        s.tcode = t;
        if (t >= 0x1000000u) {   // three bytes or more: no type
            s.phase = kSpFail;
        } else if (rest) {       // e is in this step
            s.ins = base + end;
            s.bit = sample_type_bit(t, types);
            s.phase = !s.bit ? kSpFail
                    : end + 1u < v ? (sample_byte(w0, w1, w2, w3, end + 1u) == 0x23u ? kSpOk : kSpFail)
                                   : kSpHash;   // the next step's first byte, if the content has one
        }
    }
}

// The content of clen bytes has ended. 1: sampleable, and s.ins and s.bit hold.
SRK_HD uint32_t sample_finish(SampleState &s, uint32_t clen, uint32_t types) {
    if (s.phase == kSpType) {
        s.ins = clen;
        s.bit = sample_type_bit(s.tcode, types);
        s.phase = s.bit ? kSpOk : kSpFail;
    }
    return s.phase == kSpOk ? 1u : 0u;
}

// K[j], j < SR_SAMPLE_STEPS: 1, 2, 5 times a power of ten
SRK_HD uint32_t sample_k(uint32_t j) {
    const uint32_t d = j / 3u, r = j - 3u * d;
    const uint32_t ten = d == 0u ? 1u : d == 1u ? 10u : d == 2u ? 100u : d == 3u ? 1000u : 10000u;
    return (r == 0u ? 1u : r == 1u ? 2u : 5u) * ten;
}

// the smallest j with c <= limit * K[j], else the last step
SRK_HD uint32_t sample_step(uint32_t limit, uint64_t c) {
    uint32_t j = 0u;
    for (uint32_t k = 0u; k + 1u < kSampleSteps; ++k) j += c > (uint64_t)limit * sample_k(k) ? 1u : 0u;
    return j;   // K rises, so the number of steps that c exceeds is the first that it does not
}

SRK_HD uint32_t sample_keep(uint64_t hash, uint64_t seed, uint64_t index, uint32_t step) {
    const uint64_t u = stats_fmix64(hash ^ (seed + index * kSampleGolden));
    return step == 0u || (((u >> 32) * sample_k(step)) >> 32) == 0u ? 1u : 0u;
}

// "|@" + R[step] as up to eight little-endian bytes and its length, 1 <= step < SR_SAMPLE_STEPS: "0.", then z
// zeroes, then 5, 2 or 1, with step - 1 = 3 z + r.
SRK_HD uint64_t sample_insert(uint32_t step, uint32_t *len) {
    const uint32_t z = (step - 1u) / 3u, r = step - 1u - 3u * z;
    const uint64_t digit = r == 0u ? 0x35u : r == 1u ? 0x32u : 0x31u;
    const uint32_t at = 8u * (4u + z);   // the digit's byte: 4..7
    const uint64_t text = (0x303030302E30407Cull & ~(0xFFull << at)) | digit << at;
    *len = 5u + z;
    return z == 3u ? text : text & ((1ull << (at + 8u)) - 1ull);
}
SRK_HD uint32_t sample_insert_len(uint32_t step) { return step == 0u ? 0u : 5u + (step - 1u) / 3u; }

inline const char *sample_rate_text(uint32_t step) {
    static const char *const texts[SR_SAMPLE_STEPS] = {"", "0.5", "0.2", "0.1", "0.05", "0.02", "0.01", "0.005",
                                                       "0.002", "0.001", "0.0005", "0.0002", "0.0001"};
    return step < kSampleSteps ? texts[step] : nullptr;
}

inline uint32_t sample_resolve_slots(uint32_t slots) { return slots ? slots : SR_SAMPLE_DEFAULT_SLOTS; }

// 0 or -EINVAL, as sr_sample_open judges a configuration
inline int sample_check(const sr_sample_config *cfg) {
    if (!cfg) return -EINVAL;
    const uint32_t s = sample_resolve_slots(cfg->slots);
    if (s < SR_SAMPLE_MIN_SLOTS || s > SR_SAMPLE_MAX_SLOTS || (s & (s - 1u))) return -EINVAL;
    if (cfg->limit < 1u || cfg->reserved != 0u) return -EINVAL;
    if (cfg->types == 0u || (cfg->types & ~kSampleTypesAll)) return -EINVAL;
    return 0;
}

// 1 when the line of len bytes ('\n' included) is sampleable under `types`. Reads line[0 .. len) only.
inline int sample_parse(const uint8_t *line, size_t len, uint32_t types, uint32_t *ins, uint32_t *type_bit) {
    if (len < 6 || len > SR_SAMPLE_LINE_MAX || line[len - 1] != 0x0Au) return 0;
    const size_t clen = len - 1;
    SampleState s;
    sample_begin(s);
    for (size_t base = 0; base < clen && s.phase < kSpOk; base += 16) {
        const size_t v = clen - base < 16 ? clen - base : 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (size_t q = 0; q < v; ++q) w[q >> 2] |= (uint32_t)line[base + q] << (8u * (q & 3u));
        sample_step_bytes(s, w[0], w[1], w[2], w[3], (uint32_t)base, (uint32_t)v, types);
    }
    if (!sample_finish(s, (uint32_t)clen, types)) return 0;
    if (ins) *ins = s.ins;
    if (type_bit) *type_bit = s.bit;
    return 1;
}

// line[0:ins] + "|@" + R[step] + line[ins:len] into dst (len + SR_SAMPLE_EXTRA_MAX bytes of room); the new length
inline size_t sample_rewrite(uint8_t *dst, const uint8_t *line, size_t len, uint32_t ins, uint32_t step) {
    if (!dst || !line || step == 0u || step >= kSampleSteps || ins > len) return 0;
    uint32_t n = 0u;
    const uint64_t text = sample_insert(step, &n);
    memcpy(dst, line, ins);
    for (uint32_t k = 0; k < n; ++k) dst[ins + k] = (uint8_t)(text >> (8u * k));
    memcpy(dst + ins + n, line + ins, len - ins);
    return len + n;
}

// `<limit>` or `<limit>:<comma list of c, ms, h, d>`; the default types are ms, h, d
inline int sample_parse_spec(const char *text, sr_sample_config *out) {
    if (!text || !out) return -EINVAL;
    sr_sample_config cfg = {0u, 0u, kSampleDefaultTypes, 0u, 0ull};
    const char *p = text;
    uint64_t limit = 0;
    if (*p < '0' || *p > '9') return -EINVAL;
    for (; *p >= '0' && *p <= '9'; ++p) {
        limit = limit * 10u + (uint64_t)(*p - '0');
        if (limit > 0xFFFFFFFFull) return -EINVAL;
    }
    if (limit < 1u) return -EINVAL;
    cfg.limit = (uint32_t)limit;
    if (*p == ':') {
        cfg.types = 0u;
        ++p;
        for (;;) {
            const char *e = strchr(p, ',');
            const size_t n = e ? (size_t)(e - p) : strlen(p);
            const uint32_t bit = n == 1 && *p == 'c' ? SR_VALID_TYPE_C : n == 1 && *p == 'h' ? SR_VALID_TYPE_H
                               : n == 1 && *p == 'd' ? SR_VALID_TYPE_D
                               : n == 2 && p[0] == 'm' && p[1] == 's' ? SR_VALID_TYPE_MS : 0u;
            if (!bit) return -EINVAL;
            cfg.types |= bit;
            if (!e) break;
            p = e + 1;
        }
    } else if (*p) {
        return -EINVAL;
    }
    *out = cfg;
    return 0;
}

}  // namespace srk
