// stats_host.hpp — the host part of the name statistics (include/sr_route.h): the
// configuration's defaults and limits, the hash mixing both sides share, and everything that works on a
// snapshot (estimate, cardinality, merge, the ordering of the hot entries). No HIP here: a host program can
// include this file alone (tools/stats_host_check.cpp).
#pragma once

#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/sr_route.h"

#ifndef SRK_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRK_HD __host__ __device__ __forceinline__
#else
#define SRK_HD inline
#endif
#endif

namespace srk {

// The MurmurHash3 finaliser: sdbm alone mixes too weakly for a sketch. A bijection; fmix64(0) = 0.
SRK_HD uint64_t stats_fmix64(uint64_t m) {
    m ^= m >> 33;
    m *= 0xff51afd7ed558ccdull;
    m ^= m >> 33;
    m *= 0xc4ceb9fe1a85ec53ull;
    m ^= m >> 33;
    return m;
}

// Row r's cell of the count-min sketch for the mixed hash m (32-bit wrapping arithmetic; wmask = W - 1).
SRK_HD uint32_t stats_cell(uint64_t m, uint32_t r, uint32_t wmask) {
    const uint32_t a = (uint32_t)m, b = (uint32_t)(m >> 32) | 1u;
    return (a + r * b) & wmask;
}

// The defaults filled in and the limits checked. Returns 0 or -EINVAL.
inline int stats_resolve(const sr_stats_config *in, uint32_t nds, sr_stats_config *out) {
    sr_stats_config c;
    memset(&c, 0, sizeof(c));
    if (in) c = *in;
    if (!c.hll_p && !c.cms_rows && !c.cms_width && !c.hot_slots && !c.hot_div && !c.hot_min_lines) {
        c.hll_p = SR_STATS_DEFAULT_P;
        c.cms_rows = SR_STATS_DEFAULT_ROWS;
        c.cms_width = SR_STATS_DEFAULT_WIDTH;
        c.hot_slots = SR_STATS_DEFAULT_SLOTS;
        c.hot_div = SR_STATS_DEFAULT_HOT_DIV;
        c.hot_min_lines = SR_STATS_DEFAULT_HOT_MIN;
    }
    if (c.hll_p < SR_STATS_MIN_P || c.hll_p > SR_STATS_MAX_P) return -EINVAL;
    if (((uint64_t)nds << c.hll_p) > SR_STATS_MAX_REGS) return -EINVAL;
    if (c.cms_rows < 1 || c.cms_rows > SR_STATS_MAX_ROWS) return -EINVAL;
    if (c.cms_width < SR_STATS_MIN_WIDTH || (c.cms_width & (c.cms_width - 1u))) return -EINVAL;
    if ((uint64_t)c.cms_rows * c.cms_width > SR_STATS_MAX_CELLS) return -EINVAL;
    if (c.hot_slots < SR_STATS_MIN_SLOTS || c.hot_slots > SR_STATS_MAX_SLOTS || (c.hot_slots & (c.hot_slots - 1u)))
        return -EINVAL;
    if (c.hot_div < 1) return -EINVAL;
    *out = c;
    return 0;
}

inline bool stats_cfg_equal(const sr_stats_config &a, const sr_stats_config &b) {
    return a.hll_p == b.hll_p && a.cms_rows == b.cms_rows && a.cms_width == b.cms_width && a.hot_slots == b.hot_slots &&
           a.hot_div == b.hot_div && a.hot_min_lines == b.hot_min_lines;
}

// A snapshot's configuration as its own arrays need it (snapshots may come from a caller).
inline bool stats_snap_ok(const sr_stats_snapshot *s) {
    sr_stats_config c;
    if (!s || stats_resolve(&s->cfg, s->n_downstreams, &c) != 0 || !stats_cfg_equal(c, s->cfg)) return false;
    if (!s->cells || (s->n_downstreams && (!s->regs || !s->shard_lines || !s->shard_bytes))) return false;
    return s->n_hot <= s->cfg.hot_slots && (s->hot || !s->n_hot);
}

// One allocation: the structure, then its arrays (8-byte ones first). Freed with free().
inline sr_stats_snapshot *stats_snap_alloc(const sr_stats_config &cfg, uint32_t nds) {
    const size_t cells = (size_t)cfg.cms_rows * cfg.cms_width, regs = (size_t)nds << cfg.hll_p;
    const size_t head = (sizeof(sr_stats_snapshot) + 15u) & ~(size_t)15u;
    const size_t bytes = head + 2 * (size_t)nds * 8u + cells * 8u + (size_t)cfg.hot_slots * sizeof(sr_stats_hot) + regs;
    uint8_t *p = (uint8_t *)calloc(1, bytes ? bytes : 1);
    if (!p) return nullptr;
    sr_stats_snapshot *s = (sr_stats_snapshot *)p;
    s->cfg = cfg;
    s->n_downstreams = nds;
    p += head;
    s->shard_lines = (uint64_t *)p;
    p += (size_t)nds * 8u;
    s->shard_bytes = (uint64_t *)p;
    p += (size_t)nds * 8u;
    s->cells = (uint64_t *)p;
    p += cells * 8u;
    s->hot = (sr_stats_hot *)p;
    p += (size_t)cfg.hot_slots * sizeof(sr_stats_hot);
    s->regs = p;
    return s;
}

inline uint64_t stats_estimate(const sr_stats_snapshot *s, uint64_t hash) {
    const uint64_t m = stats_fmix64(hash);
    const uint32_t wmask = s->cfg.cms_width - 1u;
    uint64_t est = ~0ull;
    for (uint32_t r = 0; r < s->cfg.cms_rows; ++r)
        est = std::min(est, s->cells[(size_t)r * s->cfg.cms_width + stats_cell(m, r, wmask)]);
    return est;
}

// lines = est(hash) from this snapshot; by lines descending, then hash ascending
inline void stats_sort_hot(sr_stats_snapshot *s) {
    for (uint32_t i = 0; i < s->n_hot; ++i) s->hot[i].lines = stats_estimate(s, s->hot[i].hash);
    std::sort(s->hot, s->hot + s->n_hot, [](const sr_stats_hot &a, const sr_stats_hot &b) {
        return a.lines != b.lines ? a.lines > b.lines : a.hash < b.hash;
    });
}

inline double stats_cardinality(const sr_stats_snapshot *s, uint32_t shard) {
    const uint32_t m = 1u << s->cfg.hll_p;
    double sum = 0.0;
    uint32_t zeros = 0;
    for (uint32_t i = 0; i < m; ++i) {
        uint8_t reg = 0;
        if (shard == SR_STATS_ALL) {
            for (uint32_t k = 0; k < s->n_downstreams; ++k) reg = std::max(reg, s->regs[((size_t)k << s->cfg.hll_p) + i]);
        } else {
            reg = s->regs[((size_t)shard << s->cfg.hll_p) + i];
        }
        sum += ldexp(1.0, -(int)reg);
        zeros += reg == 0;
    }
    const double alpha = m == 16 ? 0.673 : m == 32 ? 0.697 : m == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / (double)m);
    const double e = alpha * (double)m * (double)m / sum;
    if (e <= 2.5 * (double)m && zeros) return (double)m * log((double)m / (double)zeros);
    return e;
}

inline int stats_merge(sr_stats_snapshot *into, const sr_stats_snapshot *from) {
    if (!stats_snap_ok(into) || !stats_snap_ok(from)) return -EINVAL;
    if (!stats_cfg_equal(into->cfg, from->cfg) || into->n_downstreams != from->n_downstreams) return -EINVAL;
    const uint32_t nds = into->n_downstreams;
    for (int v = 0; v < 4; ++v) {
        into->lines[v] += from->lines[v];
        into->bytes[v] += from->bytes[v];
    }
    into->ignored += from->ignored;
    for (uint32_t k = 0; k < nds; ++k) {
        into->shard_lines[k] += from->shard_lines[k];
        into->shard_bytes[k] += from->shard_bytes[k];
    }
    const size_t regs = (size_t)nds << into->cfg.hll_p, cells = (size_t)into->cfg.cms_rows * into->cfg.cms_width;
    for (size_t i = 0; i < regs; ++i) into->regs[i] = std::max(into->regs[i], from->regs[i]);
    for (size_t i = 0; i < cells; ++i) into->cells[i] += from->cells[i];
    into->hot_overflow = (into->hot_overflow || from->hot_overflow) ? 1u : 0u;
    for (uint32_t j = 0; j < from->n_hot; ++j) {
        bool have = false;
        for (uint32_t i = 0; i < into->n_hot && !have; ++i) have = into->hot[i].hash == from->hot[j].hash;
        if (have) continue;
        if (into->n_hot >= into->cfg.hot_slots) {
            into->hot_overflow = 1u;
            continue;
        }
        into->hot[into->n_hot++] = from->hot[j];
    }
    stats_sort_hot(into);
    return 0;
}

// sr-main.c:120-134: sdbm with the reference's signed `char` (bytes >= 0x80 subtract)
inline uint64_t stats_name_hash(const uint8_t *s, size_t len) {
    uint64_t h = 0;
    for (size_t i = 0; i < len; ++i) h = (h << 6) + (h << 16) - h + (uint64_t)(int64_t)(int8_t)s[i];
    return h;
}

}  // namespace srk
