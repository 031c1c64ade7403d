// validate_host.hpp — the host part of the line grammar (include/sr_route.h): the judgement of one
// line, the configuration's check, the reasons' names and the SR_VALIDATE spec. The check kernel runs the very same
// judgement (validate_step, validate_finish: SRK_HD) over the very same 16-byte steps, so the device cannot disagree
// with sr_validate_line. No HIP here: a host program can include this file alone (tools/validate_host_check.cpp).
//
// A line is taken in steps of 16 bytes, four little-endian dwords. Per step three 16-bit masks are built with SWAR on
// the dwords: bytes outside 0x21..0x7E, ':' and '|' (digits are told apart in the middle, byte by byte). The
// judgement is a small machine over those steps:
//   NAME   up to the first ':' — by masks alone: the colon's place, and whether a byte before it is outside NB;
//   VALUE, TYPE, SECTION START, RATE — the middle of the line, byte by byte out of the four dwords (no array): f0
//          is classified for every type at once (a number's shape, its sign, its length as a set value), because
//          the type that decides follows it and TYPE comes before VALUE;
//   TAGS   from '#' on — by masks alone: a byte outside TB before the next '|' is TAGS, a further field is SECTION.
// A machine that has its reason is DONE and ignores further steps.
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "stats_host.hpp"

// loops of the shared judgement stay loops on the device
#ifndef SRK_ROLLED
#if defined(__HIPCC__)
#define SRK_ROLLED _Pragma("unroll 1")
#else
#define SRK_ROLLED
#endif
#endif

namespace srk {

constexpr uint32_t kValidTypesAll = SR_VALID_TYPES_ALL;
constexpr uint32_t kValidDropAll = ((1u << SR_VALID_REASONS) - 1u) & ~1u;
constexpr uint32_t kValidNumDigits = 20u, kValidSetMax = 64u;

enum : uint32_t { kVpName = 0, kVpValue, kVpType, kVpSection, kVpRate, kVpTags, kVpDone };
// a number's shape: nothing yet (a sign may come), a digit must come, integer digits, behind the point, fraction
// digits, no number
enum : uint32_t { kVnStart = 0, kVnFirst, kVnInt, kVnPoint, kVnFrac, kVnBad };

// The machine's state, six registers on the device. A machine that is DONE holds kVpDone + its reason in phase.
enum : uint32_t {
    kVfNameBad = 1u,      // NAME: a byte outside NB was seen
    kVfNotTb = 2u,        // VALUE: a byte of f0 is outside TB
    kVfTagged = 4u,       // TAGS: the field has a byte
    kVfAt = 8u,           // an '@' field was seen
    kVfMinus = 16u,       // VALUE: f0 begins with '-'
    kVfPlus = 32u,        // VALUE: f0 begins with '+'
    kVfTypeShift = 8u,    // the type's bit (SR_VALID_TYPE_*) once f1 has passed
};

struct ValidateState {
    uint32_t phase;
    uint32_t flags;
    uint32_t num, digits;   // VALUE, RATE: the number's shape and the digits of its current run
    uint32_t vlen;          // VALUE: f0's bytes, capped at kValidSetMax + 1
    uint32_t tcode;         // TYPE: 1, then f1's bytes shifted in from the right; all ones once there are three
};

SRK_HD void validate_begin(ValidateState &s) {
    s.phase = kVpName;
    s.flags = s.num = s.digits = s.vlen = 0u;
    s.tcode = 1u;
}

SRK_HD void validate_fail(ValidateState &s, uint32_t reason) { s.phase = kVpDone + reason; }

// 0x80 in every byte of x that is zero (exact: no borrow crosses a byte)
SRK_HD uint32_t validate_zero_bytes(uint32_t x) {
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// 0x80 in every byte b of x with lo <= b < lo + span, for lo + span <= 0x80 (bytes of 0x80 and above never match)
SRK_HD uint32_t validate_range_bytes(uint32_t x, uint32_t lo, uint32_t span) {
    const uint32_t l = x & 0x7F7F7F7Fu;
    const uint32_t ge = l + (0x80u - lo) * 0x01010101u;          // bit 7: b7 >= lo
    const uint32_t lt = ~(l + (0x80u - lo - span) * 0x01010101u);  // bit 7: b7 < lo + span
    return ge & lt & ~x & 0x80808080u;
}
// the four 0x80 flags of a dword as bits 0..3
SRK_HD uint32_t validate_gather(uint32_t m) { return ((m >> 7) * 0x00204081u >> 21) & 0xFu; }

struct ValidateMasks {
    uint32_t bad, colon, pipe;   // bit i: byte i of the step
};

SRK_HD ValidateMasks validate_masks(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t v) {
    const uint32_t w[4] = {w0, w1, w2, w3};
    ValidateMasks m = {0u, 0u, 0u};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 4u; ++k) {
        m.bad |= validate_gather(~validate_range_bytes(w[k], 0x21u, 0x5Eu) & 0x80808080u) << (4u * k);
        m.colon |= validate_gather(validate_zero_bytes(w[k] ^ 0x3A3A3A3Au)) << (4u * k);
        m.pipe |= validate_gather(validate_zero_bytes(w[k] ^ 0x7C7C7C7Cu)) << (4u * k);
    }
    const uint32_t valid = v >= 16u ? 0xFFFFu : (1u << v) - 1u;
    m.bad &= valid;
    m.colon &= valid;
    m.pipe &= valid;
    return m;
}

// one byte of a number; written as selects, so that the device needs no branch for it
SRK_HD void validate_number_byte(ValidateState &s, uint32_t b) {
    const uint32_t n = s.num;
    const bool digit = b - 0x30u < 10u, run = n == kVnInt || n == kVnFrac;
    const bool sign = (b == 0x2Du || b == 0x2Bu) && n == kVnStart;
    const uint32_t digits = digit ? (run ? s.digits + 1u : 1u) : s.digits;
    uint32_t to = digit  ? (run ? n : n == kVnBad ? kVnBad : n == kVnPoint ? kVnFrac : kVnInt)
                : b == 0x2Eu ? (n == kVnInt ? kVnPoint : kVnBad)
                : sign   ? kVnFirst
                         : kVnBad;
    if (digits > kValidNumDigits) to = kVnBad;
    s.num = to;
    s.digits = digits;
    s.flags |= sign ? (b == 0x2Du ? kVfMinus : kVfPlus) : 0u;
}

SRK_HD bool validate_number_ok(const ValidateState &s) { return s.num == kVnInt || s.num == kVnFrac; }

// f1 has ended: the phase that follows (TYPE, then VALUE, else `next`); *bit receives the type's bit
SRK_HD uint32_t validate_end_type(const ValidateState &s, uint32_t accept, uint32_t next, uint32_t *bit_out) {
    const uint32_t c = s.tcode;
    const uint32_t bit = c == 0x163u ? SR_VALID_TYPE_C : c == 0x167u ? SR_VALID_TYPE_G : c == 0x168u ? SR_VALID_TYPE_H
                       : c == 0x173u ? SR_VALID_TYPE_S : c == 0x164u ? SR_VALID_TYPE_D
                       : c == 0x16D73u ? SR_VALID_TYPE_MS : 0u;
    const bool num = validate_number_ok(s);
    const bool set = s.vlen >= 1u && s.vlen <= kValidSetMax && !(s.flags & kVfNotTb);
    const uint32_t signs = bit == SR_VALID_TYPE_G ? 0u : bit == SR_VALID_TYPE_C ? kVfPlus : kVfPlus | kVfMinus;
    const bool ok = bit == SR_VALID_TYPE_S ? set : num && !(s.flags & signs);
    *bit_out = bit;
    return !(bit & accept) ? kVpDone + SR_VALID_TYPE : !ok ? kVpDone + SR_VALID_VALUE : next;
}

// an '@' field has ended: the phase that follows
SRK_HD uint32_t validate_end_rate(const ValidateState &s, uint32_t next) {
    const uint32_t rated = (SR_VALID_TYPE_C | SR_VALID_TYPE_MS | SR_VALID_TYPE_H | SR_VALID_TYPE_D) << kVfTypeShift;
    return validate_number_ok(s) && (s.flags & rated) ? next : kVpDone + SR_VALID_RATE;
}

// One byte of the middle of the line (the phase is VALUE, TYPE, SECTION or RATE). Every phase's answer is worked
// out and the phase picks: selects, no branches, so the device keeps the machine in its six registers.
SRK_HD void validate_middle_byte(ValidateState &s, uint32_t b, uint32_t accept) {
    const uint32_t ph = s.phase;
    const bool pipe = b == 0x7Cu;
    const bool in_value = ph == kVpValue, in_type = ph == kVpType, in_rate = ph == kVpRate, in_section = ph == kVpSection;
    uint32_t bit = 0u;
    const uint32_t after_type = validate_end_type(s, accept, kVpSection, &bit);
    const uint32_t after_rate = validate_end_rate(s, kVpSection);
    const bool at = in_section && b == 0x40u && !(s.flags & kVfAt);   // (no field behind '#' comes here: TAGS ends it)
    const uint32_t after_section = at ? kVpRate : b == 0x23u ? kVpTags : kVpDone + SR_VALID_SECTION;
    ValidateState n = s;
    validate_number_byte(n, b);
    const bool number = (in_value || in_rate) && !pipe;
    uint32_t flags = number ? n.flags : s.flags;
    if (in_value && !pipe && b - 0x21u >= 0x5Eu) flags |= kVfNotTb;
    if (in_type && pipe && after_type == kVpSection) flags |= bit << kVfTypeShift;
    if (at) flags |= kVfAt;
    s.flags = flags;
    s.num = at ? kVnFirst : number ? n.num : s.num;   // behind '@': no sign
    s.digits = at ? 0u : number ? n.digits : s.digits;
    s.vlen += in_value && !pipe && s.vlen <= kValidSetMax ? 1u : 0u;
    s.tcode = in_type && !pipe ? (s.tcode < 0x10000u ? s.tcode << 8 | b : 0xFFFFFFFFu) : s.tcode;
    s.phase = in_section ? after_section
            : !pipe      ? ph
            : in_value   ? kVpType
            : in_type    ? after_type
                         : after_rate;
}

// One step: bytes [base, base + v) of the line's L bytes as four little-endian dwords, 1 <= v <= 16; bytes of the
// dwords behind v are ignored. `last` marks the step that holds the line's last byte: a '\n' there is not content.
// Not called for a machine that is DONE.
SRK_HD void validate_step(ValidateState &s, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t base,
                          uint32_t v, bool last, uint32_t accept) {
    {   // a '\n' as the line's last byte is not content (v may become 0: then every mask is empty)
        const uint32_t q = v - 1u;
        const uint32_t d = q < 4u ? w0 : q < 8u ? w1 : q < 12u ? w2 : w3;
        v -= last && ((d >> (8u * (q & 3u))) & 0xFFu) == 0x0Au ? 1u : 0u;
    }
    const ValidateMasks m = validate_masks(w0, w1, w2, w3, v);
    uint32_t from = 0u;   // the step's first byte that the next phase takes
    {   // NAME, as selects: the first ':' of the step, and whether a byte before it is outside NB
        const bool in_name = s.phase == kVpName;
        const uint32_t nb = m.bad | m.pipe;
        const uint32_t p = (uint32_t)__builtin_ctz(m.colon | 0x10000u);   // 16: none
        const bool bad = ((s.flags & kVfNameBad) | (nb & ((1u << p) - 1u))) != 0u;
        const uint32_t to = p == 16u ? kVpName : base + p == 0u ? kVpDone + SR_VALID_EMPTY_NAME
                          : bad ? kVpDone + SR_VALID_NAME_BYTE : kVpValue;
        s.flags |= in_name && nb ? kVfNameBad : 0u;   // (only read while the phase is NAME)
        s.phase = in_name ? to : s.phase;
        from = in_name ? p + 1u : 0u;                 // 17 when there is no ':': nothing below looks at the step
    }
    // the middle: one byte per turn, picked out of the four dwords by comparisons (no array, so no scratch on the
    // device); the loop stays a loop there, as unrolled it costs the kernel its register budget
    SRK_ROLLED
    for (; from < v && s.phase >= kVpValue && s.phase <= kVpRate; ++from) {
        const uint32_t d = from < 4u ? w0 : from < 8u ? w1 : from < 12u ? w2 : w3;
        validate_middle_byte(s, (d >> (8u * (from & 3u))) & 0xFFu, accept);
    }
    if (s.phase == kVpTags && from <= v) {   // TAGS, from byte `from` of the step (from may be v)
        const uint32_t pipes = m.pipe >> from << from;
        const uint32_t end = (uint32_t)__builtin_ctz(pipes | (1u << v));
        const uint32_t span = ((1u << end) - 1u) >> from << from;
        if (end > from) s.flags |= kVfTagged;
        if (m.bad & span) s.phase = kVpDone + SR_VALID_TAGS;
        else if (pipes) s.phase = kVpDone + ((s.flags & kVfTagged) ? SR_VALID_SECTION : SR_VALID_TAGS);
    }
}

// The content has ended.
SRK_HD uint32_t validate_finish(const ValidateState &s, uint32_t accept) {
    uint32_t bit = 0u;
    const uint32_t ph = s.phase == kVpType ? validate_end_type(s, accept, kVpDone + SR_VALID_OK, &bit)
                      : s.phase == kVpRate ? validate_end_rate(s, kVpDone + SR_VALID_OK)
                                           : s.phase;
    if (ph >= kVpDone) return ph - kVpDone;
    return ph == kVpName ? SR_VALID_NO_COLON : ph == kVpValue ? SR_VALID_NO_TYPE : ph == kVpSection ? SR_VALID_SECTION
         : !(s.flags & kVfTagged) ? SR_VALID_TAGS : SR_VALID_OK;
}

// 0 or -EINVAL, as sr_validate_open judges a configuration
inline int validate_check(const sr_validate_config *cfg) {
    if (!cfg) return -EINVAL;
    if ((cfg->drop_mask & 1u) || (cfg->drop_mask >> SR_VALID_REASONS)) return -EINVAL;
    if (cfg->accept_types == 0u || (cfg->accept_types & ~kValidTypesAll)) return -EINVAL;
    return 0;
}

// The reason of one line of len >= 1 bytes ('\n' included when it has one). Reads line[0 .. len) only.
inline uint32_t validate_line(const uint8_t *line, size_t len, uint32_t accept) {
    ValidateState s;
    validate_begin(s);
    for (size_t base = 0; base < len && s.phase < kVpDone; base += 16) {
        const size_t v = len - base < 16 ? len - base : 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (size_t q = 0; q < v; ++q) w[q >> 2] |= (uint32_t)line[base + q] << (8u * (q & 3u));
        validate_step(s, w[0], w[1], w[2], w[3], (uint32_t)(base > 0xFFFFFFF0u ? 0xFFFFFFF0u : base), (uint32_t)v,
                      base + 16 >= len, accept);
    }
    return validate_finish(s, accept);
}

inline const char *validate_reason_name(uint32_t reason) {
    static const char *const names[SR_VALID_REASONS] = {"ok", "no_colon", "empty_name", "name_byte", "no_type",
                                                       "type", "value", "section", "rate", "tags"};
    return reason < SR_VALID_REASONS ? names[reason] : nullptr;
}

// `count`, `drop`, or a comma list of reason names to drop; every type is accepted
inline int validate_parse_spec(const char *text, sr_validate_config *out) {
    if (!text || !out) return -EINVAL;
    sr_validate_config cfg = {0u, kValidTypesAll};
    if (strcmp(text, "count") == 0) {
        *out = cfg;
        return 0;
    }
    if (strcmp(text, "drop") == 0) {
        cfg.drop_mask = kValidDropAll;
        *out = cfg;
        return 0;
    }
    const char *p = text;
    for (;;) {
        const char *e = strchr(p, ',');
        const size_t n = e ? (size_t)(e - p) : strlen(p);
        uint32_t r = 0u;
        for (uint32_t q = 1u; q < SR_VALID_REASONS; ++q) {
            const char *name = validate_reason_name(q);
            if (strlen(name) == n && memcmp(name, p, n) == 0) r = q;
        }
        if (r == 0u) return -EINVAL;
        cfg.drop_mask |= 1u << r;
        if (!e) break;
        p = e + 1;
    }
    *out = cfg;
    return 0;
}

}  // namespace srk
