// rules_host.hpp — the host part of the name rules (include/sr_route.h): validation of a rule
// set, its compiled table, the search of that table for a line's head, and the rule file's text format. The match
// kernel runs the very same search (rules_search, SRK_HD) over the very same table, copied into LDS, so the device
// cannot disagree with sr_rules_match. No HIP here: a host program can include this file alone
// (tools/rules_host_check.cpp).
//
// The compiled form: the distinct pattern texts sorted as byte strings (a shorter text before its extensions),
// one entry per text with the PREFIX rule and the EXACT rule of that text, and per entry its parent: the longest
// other text that is a proper prefix of it. The patterns that are prefixes of a head H form a chain P1 < ... < P*
// under "is a prefix of"; every text between P* and H in sorted order begins with P*. So the largest text <= H
// (one binary search, compared by 8-byte big-endian words) has P* among its ancestors, and P* is the first
// ancestor-or-self no longer than the bytes that text shares with H. From there the chain is walked up until an
// entry has a rule that applies: EXACT when the byte behind the text is ':', else PREFIX.
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "stats_host.hpp"

// loops of the shared search stay loops on the device: unrolled they cost the match kernel its register budget
#if defined(__HIPCC__)
#define SRK_ROLLED _Pragma("unroll 1")
#else
#define SRK_ROLLED
#endif

namespace srk {

constexpr uint32_t kRulesMax = SR_RULES_MAX, kRulesPatternMax = SR_RULES_PATTERN_MAX, kRulesTextMax = SR_RULES_TEXT_MAX;
constexpr uint32_t kRulesNone = 0xFFFFu;                         // no such rule, no parent
constexpr uint32_t kRulesHeadMax = kRulesPatternMax + 1u;        // the longest text and the byte behind it
constexpr uint32_t kRulesHeadWords = (kRulesHeadMax + 7u) / 8u;  // 9 big-endian words

struct RulesEntry {
    uint16_t off, len;                 // the text in RulesTable::text
    uint16_t parent;                   // the longest entry whose text is a proper prefix of this one, or none
    uint16_t prefix_rule, exact_rule;  // the caller's rule indices, or none
    uint16_t pad;
};
static_assert(sizeof(RulesEntry) == 12, "table entry layout");

// What sr_rules_open uploads and rules_match_kernel copies into LDS, 16 bytes at a time.
struct RulesTable {
    uint32_t n_rules, n_entries, default_action, pad;
    uint64_t key[kRulesMax];             // an entry's first 8 bytes, big endian, zero filled
    RulesEntry ent[kRulesMax];
    uint8_t action[kRulesMax + 16];      // per rule, then the default's at n_rules
    uint8_t first_max[256];              // by a text's first byte: the longest such text (0: none begins so)
    uint8_t text[kRulesTextMax];
};
static_assert(sizeof(RulesTable) % 16 == 0 && sizeof(RulesTable) <= 10 * 1024, "the table is copied as uint4 and fits LDS eight times over");

// Validation alone: 0 or -EINVAL. Duplicates are found by the compiler below (it sorts).
inline int rules_check_shape(const sr_rules_config *cfg) {
    if (!cfg || cfg->n_rules > kRulesMax || (cfg->n_rules && !cfg->rules)) return -EINVAL;
    if (cfg->default_action != SR_RULE_DROP && cfg->default_action != SR_RULE_KEEP) return -EINVAL;
    size_t text = 0;
    for (uint32_t i = 0; i < cfg->n_rules; ++i) {
        const sr_rule &r = cfg->rules[i];
        if (!r.pattern || r.len < 1u || r.len > kRulesPatternMax) return -EINVAL;
        if (r.kind != SR_RULE_PREFIX && r.kind != SR_RULE_EXACT) return -EINVAL;
        if (r.action != SR_RULE_DROP && r.action != SR_RULE_KEEP) return -EINVAL;
        for (uint32_t q = 0; q < r.len; ++q)
            if (r.pattern[q] == (uint8_t)':' || r.pattern[q] == (uint8_t)'\n') return -EINVAL;
        text += r.len;
    }
    return text > kRulesTextMax ? -EINVAL : 0;
}

inline int rules_text_cmp(const sr_rule &a, const sr_rule &b) {
    const uint32_t m = a.len < b.len ? a.len : b.len;
    const int c = memcmp(a.pattern, b.pattern, m);
    return c ? c : (a.len < b.len ? -1 : a.len > b.len ? 1 : 0);
}

// cfg into *t. 0, or -EINVAL for a bad set (two rules of one kind and text included).
inline int rules_compile(const sr_rules_config *cfg, RulesTable *t) {
    if (rules_check_shape(cfg) != 0) return -EINVAL;
    memset(t, 0, sizeof(*t));
    const uint32_t n = cfg->n_rules;
    t->n_rules = n;
    t->default_action = cfg->default_action;
    for (uint32_t i = 0; i < n; ++i) t->action[i] = cfg->rules[i].action;
    t->action[n] = (uint8_t)cfg->default_action;
    uint16_t order[kRulesMax];
    for (uint32_t i = 0; i < n; ++i) order[i] = (uint16_t)i;
    const sr_rule *rules = cfg->rules;
    std::sort(order, order + n, [rules](uint16_t x, uint16_t y) {
        const int c = rules_text_cmp(rules[x], rules[y]);
        return c ? c < 0 : (rules[x].kind != rules[y].kind ? rules[x].kind < rules[y].kind : x < y);
    });
    uint32_t ne = 0, at = 0;
    uint16_t chain[kRulesPatternMax + 1];   // the entries that are prefixes of the current text, shortest first
    uint32_t depth = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const sr_rule &r = rules[order[k]];
        if (k && rules_text_cmp(rules[order[k - 1]], r) == 0) {   // the same text: the other kind, or a duplicate
            if (rules[order[k - 1]].kind == r.kind) return -EINVAL;
        } else {
            RulesEntry &e = t->ent[ne];
            e.off = (uint16_t)at;
            e.len = (uint16_t)r.len;
            e.prefix_rule = e.exact_rule = (uint16_t)kRulesNone;
            memcpy(t->text + at, r.pattern, r.len);
            at += r.len;
            uint64_t key = 0;
            for (uint32_t q = 0; q < 8u; ++q) key = key << 8 | (q < r.len ? r.pattern[q] : 0u);
            t->key[ne] = key;
            while (depth) {   // sorted order: an entry's prefixes are the latest texts that are prefixes at all
                const RulesEntry &p = t->ent[chain[depth - 1]];
                if (p.len < r.len && memcmp(t->text + p.off, r.pattern, p.len) == 0) break;
                --depth;
            }
            e.parent = depth ? chain[depth - 1] : (uint16_t)kRulesNone;
            chain[depth++] = (uint16_t)ne;
            if (t->first_max[r.pattern[0]] < r.len) t->first_max[r.pattern[0]] = (uint8_t)r.len;
            ++ne;
        }
        RulesEntry &e = t->ent[ne - 1];
        (r.kind == SR_RULE_EXACT ? e.exact_rule : e.prefix_rule) = order[k];
    }
    t->n_entries = ne;
    return 0;
}

// Word w of entry e's text, big endian, zero filled behind its end.
SRK_HD uint64_t rules_text_word(const RulesTable &t, uint32_t e, uint32_t w) {
    if (w == 0u) return t.key[e];
    const uint32_t off = t.ent[e].off, len = t.ent[e].len;
    uint64_t v = 0;
    SRK_ROLLED
    for (uint32_t q = 8u * w; q < 8u * w + 8u; ++q) v = v << 8 | (q < len ? (uint64_t)t.text[off + q] : 0ull);
    return v;
}

// The rule that wins for a head: `have` bytes of the line's start (have = min(L - 1, need), where need >
// first_max[first byte] suffices) given as big-endian words, zero filled behind `have`: head.word(w), w <
// kRulesHeadWords. `have` >= 1. Returns the rule's index, or n_rules for none.
// A text compares with the head by words and then by length (the zero fill makes a text and its extension by NUL
// bytes equal word for word; the shorter one is the smaller): that is the order of the byte strings.
template <class Head>
SRK_HD uint32_t rules_search(const RulesTable &t, const Head &head, uint32_t have) {
    const uint32_t hwords = (have + 7u) / 8u;
    uint32_t lo = 0, hi = t.n_entries;
    SRK_ROLLED
    while (lo < hi) {   // lo = the entries <= head
        const uint32_t mid = (lo + hi) >> 1, len = t.ent[mid].len, words = (len + 7u) / 8u;
        bool le = len <= have;
        SRK_ROLLED
        for (uint32_t w = 0; w < words || w < hwords; ++w) {
            const uint64_t a = rules_text_word(t, mid, w), b = head.word(w);
            if (a != b) {
                le = a < b;
                break;
            }
        }
        if (le) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == 0u) return t.n_rules;
    uint32_t e = lo - 1u;
    uint32_t lcp = t.ent[e].len < have ? t.ent[e].len : have;   // both sides are zero behind their ends
    SRK_ROLLED
    for (uint32_t w = 0; 8u * w < lcp; ++w) {
        const uint64_t x = rules_text_word(t, e, w) ^ head.word(w);
        if (x) {
            const uint32_t same = 8u * w + ((uint32_t)__builtin_clzll(x) >> 3);
            lcp = same < lcp ? same : lcp;
            break;
        }
    }
    SRK_ROLLED
    while (e != kRulesNone) {
        const RulesEntry &en = t.ent[e];
        const uint32_t p = en.len;
        if (p <= lcp) {   // the text is a prefix of the head
            if (en.exact_rule != kRulesNone && p < have &&
                (uint8_t)(head.word(p >> 3) >> (56u - 8u * (p & 7u))) == (uint8_t)':')
                return en.exact_rule;
            if (en.prefix_rule != kRulesNone) return en.prefix_rule;
        }
        e = en.parent;
    }
    return t.n_rules;
}

// The bytes of a line that the search needs: min(L - 1, the longest text of its first byte + 1).
SRK_HD uint32_t rules_head_need(const RulesTable &t, uint8_t first, uint32_t len) {
    const uint32_t fm = t.first_max[first], head = len - 1u;
    return fm == 0u ? 0u : (head < fm + 1u ? head : fm + 1u);
}

struct RulesHostHead {
    const uint8_t *p;
    uint32_t have;
    uint64_t word(uint32_t w) const {
        uint64_t v = 0;
        for (uint32_t q = 8u * w; q < 8u * w + 8u; ++q) v = v << 8 | (q < have ? (uint64_t)p[q] : 0ull);
        return v;
    }
};

// The scalar matcher: the winning rule's index for a line of len bytes (its last byte, the '\n' of a routed line,
// is never part of a match), n_rules for none. Reads bytes of [line, line + len) only.
inline uint32_t rules_match(const RulesTable &t, const uint8_t *line, size_t len) {
    if (len < 2u) return t.n_rules;
    const uint32_t have = rules_head_need(t, line[0], (uint32_t)(len > 0xFFFFu ? 0xFFFFu : len));
    if (have == 0u) return t.n_rules;
    const RulesHostHead h{line, have};
    return rules_search(t, h, have);
}

// ---- the rule file ------------------------------------------------------------------------------------------
// One allocation: the config, its rules, the pattern bytes. Freed with free().
struct RulesParsed {
    sr_rules_config cfg;
    sr_rule rules[kRulesMax];
    uint8_t text[kRulesTextMax];
};

inline bool rules_word_is(const char *p, size_t n, const char *w) { return strlen(w) == n && memcmp(p, w, n) == 0; }

// 0 and *out, or -EINVAL / -ENOMEM with *err_line = the 1-based line at fault (0: not a line's fault).
inline int rules_parse_text(const char *text, size_t len, sr_rules_config **out, size_t *err_line) {
    if (err_line) *err_line = 0;
    if (!out || (len && !text)) return -EINVAL;
    *out = nullptr;
    RulesParsed *P = (RulesParsed *)calloc(1, sizeof(RulesParsed));
    if (!P) return -ENOMEM;
    P->cfg.rules = P->rules;
    P->cfg.default_action = SR_RULE_KEEP;
    RulesTable *scratch = (RulesTable *)malloc(sizeof(RulesTable));
    if (!scratch) {
        free(P);
        return -ENOMEM;
    }
    size_t at = 0, line_no = 0, used = 0;
    bool have_default = false, bad = false;
    while (at < len && !bad) {
        ++line_no;
        size_t end = at;
        while (end < len && text[end] != '\n') ++end;
        const char *l = text + at;
        const size_t n = end - at;
        at = end + 1;
        if (n == 0 || l[0] == '#') continue;
        size_t sp = 0;
        while (sp < n && l[sp] != ' ') ++sp;
        const size_t an = sp < n ? n - sp - 1 : 0;
        const char *arg = sp < n ? l + sp + 1 : l + n;   /* never past the text's end */
        if (rules_word_is(l, sp, "default")) {
            const bool drop = rules_word_is(arg, an, "drop"), keep = rules_word_is(arg, an, "keep");
            bad = have_default || sp == n || !(drop || keep);
            P->cfg.default_action = drop ? SR_RULE_DROP : SR_RULE_KEEP;
            have_default = true;
            continue;
        }
        const bool drop = rules_word_is(l, sp, "drop"), keep = rules_word_is(l, sp, "keep");
        const bool prefix = an && arg[an - 1] == '*';
        const size_t pn = prefix ? an - 1 : an;
        if (!(drop || keep) || sp == n || pn < 1 || pn > kRulesPatternMax || P->cfg.n_rules == kRulesMax ||
            used + pn > kRulesTextMax) {
            bad = true;
            break;
        }
        sr_rule &r = P->rules[P->cfg.n_rules];
        memcpy(P->text + used, arg, pn);
        r.pattern = P->text + used;
        r.len = (uint32_t)pn;
        r.kind = prefix ? SR_RULE_PREFIX : SR_RULE_EXACT;
        r.action = drop ? SR_RULE_DROP : SR_RULE_KEEP;
        used += pn;
        ++P->cfg.n_rules;
        bad = rules_compile(&P->cfg, scratch) != 0;   // a ':' in the pattern, or a duplicate: this line's fault
    }
    free(scratch);
    if (bad) {
        if (err_line) *err_line = line_no;
        free(P);
        return -EINVAL;
    }
    *out = &P->cfg;
    return 0;
}

}  // namespace srk
