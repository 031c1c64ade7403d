// rules_kernel.hpp — name rules on the device (include/sr_route.h).
//
// Behind a route launch the input-order records are on the device. Three launches turn them into the list of the
// records that the rule set keeps. All ordering is by kernel boundaries: no workgroup waits for another, no atomic
// returns a value that a wait depends on.
//
//   rules_match_kernel  one record per thread, tiles of kRulesTile records numbered by the device's record counts
//                       (coalesce_kernel.hpp's scheme). The workgroup copies the compiled table (rules_host.hpp,
//                       under 10 KiB) into LDS. A thread fetches its line's first 16 bytes with aligned 16-byte
//                       loads (one, or two when the line straddles a block; the halves are put together with
//                       v_alignbyte), looks its first byte up in the table's first-byte array, and ends there with
//                       the default when no pattern begins so: most lines do. Else it fetches further 16-byte
//                       steps only up to the longest pattern of that first byte plus one, and runs rules_search,
//                       the function sr_rules_match runs, over the LDS table. No loop reads global memory byte
//                       by byte, except for a 16-byte block that is not wholly inside the batch (its first and
//                       its last one at most), whose bytes inside it are read one by one.
//                       It writes the match index (u16) per record, the tile's {kept, dropped, dropped bytes,
//                       subject} and the hits: per-workgroup u64 LDS cells; a wave first settles runs of one rule
//                       (up to kRulesPeel times the first undecided lane's rule is matched against the wave, and
//                       that lane adds for all of them), and the non-zero cells go to the global cells once per
//                       workgroup.
//   rules_scan_kernel   one workgroup per batch turns the tiles' kept counts into exclusive bases (DPP wave
//                       scans, as coalesce_scan_kernel) and writes the batch's four counts.
//   rules_emit_kernel   reads the match indices, ranks the kept records in the workgroup and writes them, and
//                       their hashes when given, in input order.
//   rules_out_kernel    the host-memory path only: the counts, and for the trace the input records, into the
//                       slot's page-locked memory.
// Vector stores only; no scratch memory: the head lives in 18 registers that are only ever indexed statically.
#pragma once

#include <hip/hip_runtime.h>

#include "route_kernel.hpp"
#include "rules_host.hpp"
#include "stats_kernel.hpp"

namespace srk {

constexpr int kRulesBlock = 256;             // threads per workgroup: four waves
constexpr int kRulesTile = kRulesBlock;      // records per tile (R of the tests), one per thread
constexpr int kRulesWaves = kRulesBlock / 64;
constexpr int kRulesGroups = 2048;           // most workgroups of a launch (eight per CU)
constexpr int kRulesMaxBatches = 32;
constexpr int kRulesPeel = 2;                // rounds of settling equal rules in a wave
constexpr int kRulesScanBlock = 1024;        // rules_scan_kernel: tiles per step
// The grid is sized by the records a batch can hold: max_records, but no more than one per this many bytes
// (§5.9). A grid smaller than the tiles only means more tiles per workgroup.
constexpr uint32_t kRulesGridLineBytes = 16;
constexpr uint32_t kRulesHitCells = 2u * (kRulesMax + 1u);   // {lines, bytes} per rule and for the default

struct RulesBatchArg {
    const uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;     // with hashes_out, or both null
    sr_record *out;
    uint64_t *hashes_out;
    uint16_t *match;            // the caller's d_match, or the stage's scratch
    uint64_t *counts;
    uint32_t nbytes, max_records;
};

struct RulesArgs {
    RulesBatchArg b[kRulesMaxBatches];
    const RulesTable *table;
    unsigned long long *hits;   // kRulesHitCells
    uint4 *tiles;               // per tile {kept, dropped, dropped bytes, subject}; after the scan x = kept base
    uint32_t nb, nds;
};

// The launch's real tiles, as coalesce_tiles numbers them.
__device__ __forceinline__ uint32_t rules_tiles(const RulesArgs &a, uint32_t *s_n, uint32_t *s_t0) {
    if (threadIdx.x < kRulesMaxBatches) {
        uint32_t n = 0;
        if (threadIdx.x < a.nb) {
            const RulesBatchArg &b = a.b[threadIdx.x];
            const uint64_t nrec = *b.n_records;
            n = (uint32_t)(nrec < b.max_records ? nrec : b.max_records);
        }
        s_n[threadIdx.x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int j = 0; j < kRulesMaxBatches; ++j) {
            s_t0[j] = t;
            t += (s_n[j] + (uint32_t)kRulesTile - 1u) / (uint32_t)kRulesTile;
        }
        s_t0[kRulesMaxBatches] = t;
    }
    __syncthreads();
    return s_t0[kRulesMaxBatches];
}

// The 16-byte block at byte `rel` of the batch (rel + the batch's address is a multiple of 16; rel is negative
// for the block that begins in front of the batch). A block wholly inside [0, nbytes) is one load; of any other
// only the bytes inside are read, one by one (the rest are zero): nothing outside the batch is touched.
__device__ __forceinline__ uint4 rules_block(const uint8_t *bytes, int64_t rel, uint32_t nbytes) {
    if (rel >= 0 && rel + 16 <= (int64_t)nbytes) return *reinterpret_cast<const uint4 *>(bytes + rel);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        uint32_t v = 0u;
#pragma unroll 1
        for (uint32_t q = 0; q < 4u; ++q) {
            const int64_t p = rel + 4 * k + q;
            if (p >= 0 && p < (int64_t)nbytes) v |= (uint32_t)bytes[p] << (8u * q);
        }
        w[0] = k == 0u ? v : w[0];
        w[1] = k == 1u ? v : w[1];
        w[2] = k == 2u ? v : w[2];
        w[3] = k == 3u ? v : w[3];
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 bytes from byte `sh` (0..15) of the 32 bytes b0 | b1.
__device__ __forceinline__ uint4 rules_shift(const uint4 &b0, const uint4 &b1, uint32_t sh) {
    const uint32_t q[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const uint32_t ds = sh >> 2, bs = sh & 3u;
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = ds == 0u ? q[i] : ds == 1u ? q[i + 1] : ds == 2u ? q[i + 2] : q[i + 3];
    return make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], bs), __builtin_amdgcn_alignbyte(w[2], w[1], bs),
                      __builtin_amdgcn_alignbyte(w[3], w[2], bs), __builtin_amdgcn_alignbyte(w[4], w[3], bs));
}

// dword i of a 16-byte step of which the first v bytes count: the others become zero
__device__ __forceinline__ uint32_t rules_clip(uint32_t x, uint32_t v, uint32_t i) {
    const uint32_t n = v > 4u * i ? v - 4u * i : 0u;
    return n >= 4u ? x : x & ((1u << (8u * n)) - 1u);
}

// A line's head in registers, little-endian dwords, zero behind the bytes that count.
struct RulesDevHead {
    uint32_t d[2 * kRulesHeadWords];
    __device__ __forceinline__ uint64_t word(uint32_t w) const {
        uint32_t a = 0u, b = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kRulesHeadWords; ++k)
            if (w == k) {
                a = d[2 * k];
                b = d[2 * k + 1];
            }
        return (uint64_t)__builtin_bswap32(a) << 32 | __builtin_bswap32(b);
    }
};

// The winning rule of the subject record (o, len), len >= 2: n_rules for none.
__device__ __forceinline__ uint32_t rules_match_line(const RulesTable &t, const uint8_t *bytes, uint32_t nbytes,
                                                     uint32_t o, uint32_t len) {
    const uint32_t sh = (uint32_t)(((uintptr_t)bytes + o) & 15u);
    const int64_t blk = (int64_t)o - (int64_t)sh;   // the line's first block, relative to the batch
    const uint32_t head = len - 1u < kRulesHeadMax ? len - 1u : kRulesHeadMax;   // >= 1
    RulesDevHead h;
#pragma unroll
    for (uint32_t k = 0; k < 2u * kRulesHeadWords; ++k) h.d[k] = 0u;
    // the first step: up to 16 bytes, and with them the first byte
    const uint32_t v0 = head < 16u ? head : 16u;
    uint4 b0 = rules_block(bytes, blk, nbytes);
    uint4 b1 = make_uint4(0u, 0u, 0u, 0u);
    if (sh + v0 > 16u) b1 = rules_block(bytes, blk + 16, nbytes);
    uint4 c = rules_shift(b0, b1, sh);
    const uint32_t need = rules_head_need(t, (uint8_t)c.x, len);   // <= head
    if (need == 0u) return t.n_rules;   // no pattern begins with this byte
    h.d[0] = rules_clip(c.x, need, 0u);
    h.d[1] = rules_clip(c.y, need, 1u);
    h.d[2] = rules_clip(c.z, need, 2u);
    h.d[3] = rules_clip(c.w, need, 3u);
    // further steps only while a pattern of this first byte can still reach them. Step s is bytes 16 s .. of the
    // head: blocks s and, for a line that is not 16-byte aligned, s + 1; the block behind a step is the next
    // step's first, so a step loads one block.
#pragma unroll
    for (uint32_t s = 1; s < (kRulesHeadMax + 15u) / 16u; ++s) {
        if (16u * s < need) {
            const uint32_t v = need - 16u * s;   // of this step's bytes the first v count (all when v >= 16)
            b0 = sh ? b1 : rules_block(bytes, blk + 16 * (int64_t)s, nbytes);
            b1 = make_uint4(0u, 0u, 0u, 0u);
            if (sh + (v < 16u ? v : 16u) > 16u) b1 = rules_block(bytes, blk + 16 * (int64_t)(s + 1u), nbytes);
            c = rules_shift(b0, b1, sh);
            h.d[4 * s] = rules_clip(c.x, v, 0u);
            h.d[4 * s + 1] = rules_clip(c.y, v, 1u);
            if (4 * s + 2 < 2u * kRulesHeadWords) {
                h.d[4 * s + 2] = rules_clip(c.z, v, 2u);
                h.d[4 * s + 3] = rules_clip(c.w, v, 3u);
            }
        }
    }
    return rules_search(t, h, need);
}

__global__ __launch_bounds__(kRulesBlock, 8) void rules_match_kernel(RulesArgs a) {
    __shared__ __attribute__((aligned(16))) RulesTable s_t;
    __shared__ unsigned long long s_hits[kRulesHitCells];
    __shared__ uint32_t s_n[kRulesMaxBatches], s_t0[kRulesMaxBatches + 1];
    __shared__ uint32_t s_wave[kRulesWaves][4];
    const uint32_t ntiles = rules_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    {   // the table into LDS; of an empty set only the header and the actions are read, so only they are copied
        const uint4 *src = reinterpret_cast<const uint4 *>(a.table);
        uint4 *dst = reinterpret_cast<uint4 *>(&s_t);
        const uint32_t all = sizeof(RulesTable) / 16u, a0 = offsetof(RulesTable, action) / 16u,
                       a1 = offsetof(RulesTable, first_max) / 16u;
        static_assert(offsetof(RulesTable, action) % 16 == 0 && offsetof(RulesTable, first_max) % 16 == 0, "copied as uint4");
        if (a.table->n_entries) {
            for (uint32_t q = threadIdx.x; q < all; q += kRulesBlock) dst[q] = src[q];
        } else {
            if (threadIdx.x == 0) dst[0] = src[0];
            for (uint32_t q = a0 + threadIdx.x; q < a1; q += kRulesBlock) dst[q] = src[q];
        }
        const uint32_t cells = 2u * (a.table->n_rules + 1u);
        for (uint32_t q = threadIdx.x; q < cells; q += kRulesBlock) s_hits[q] = 0ull;
    }
    __syncthreads();
    const RulesTable &t = s_t;
    const uint32_t nr = t.n_rules;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;   // tile < ntiles = s_t0[32]: j stays below the batch count
        const RulesBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kRulesTile + threadIdx.x;
        uint32_t idx = SR_RULES_NOT_SUBJECT, len = 0;
        if (i < n) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(b.recs + i);   // sr_record is 4-byte aligned
            const uint32_t o = w[0], ly = w[1];
            len = ly & 0xFFFFu;
            if ((ly >> 16) < a.nds && len >= 1u && (uint64_t)o + len <= b.nbytes) {
                idx = nr;
                if (len >= 2u && t.n_entries) idx = rules_match_line(t, b.bytes, b.nbytes, o, len);
            }
            b.match[i] = (uint16_t)idx;
        }
        const bool subject = idx != SR_RULES_NOT_SUBJECT;
        const bool dropped = subject && t.action[idx] == SR_RULE_DROP;
        const uint32_t kept = (uint32_t)__builtin_popcountll(__ballot(i < n && !dropped));
        const uint64_t dm = __ballot(dropped);
        const uint32_t dbytes = dm ? stats_wave_sum(dropped ? len : 0u) : 0u;
        uint64_t rem = __ballot(subject);
        if (lane == 0u) {
            s_wave[wave][0] = kept;
            s_wave[wave][1] = (uint32_t)__builtin_popcountll(dm);
            s_wave[wave][2] = dbytes;
            s_wave[wave][3] = (uint32_t)__builtin_popcountll(rem);
        }
        // hits: runs of one rule are settled in the wave, the first undecided lane adds for all of them
        bool act = subject;
        uint32_t cnt = 1u, bsum = len;
        for (int round = 0; round < kRulesPeel && rem; ++round) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t li = __shfl(idx, lead);
            const bool mine = subject && ((rem >> lane) & 1ull) && idx == li;
            const uint64_t same = __ballot(mine);
            rem &= ~same;
            if (__builtin_popcountll(same) > 1) {
                const uint32_t s = stats_wave_sum(mine ? len : 0u);
                if (mine) {
                    act = lane == (uint32_t)lead;
                    cnt = (uint32_t)__builtin_popcountll(same);
                    bsum = s;
                }
            }
        }
        if (act) {
            atomicAdd(&s_hits[2u * idx], (unsigned long long)cnt);
            atomicAdd(&s_hits[2u * idx + 1u], (unsigned long long)bsum);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = 0, d = 0, m = 0, s = 0;
            for (int w = 0; w < kRulesWaves; ++w) {
                k += s_wave[w][0];
                d += s_wave[w][1];
                m += s_wave[w][2];
                s += s_wave[w][3];
            }
            a.tiles[tile] = make_uint4(k, d, m, s);
        }
        __syncthreads();
    }
    // the workgroup's hits into the context's: the non-zero cells only (the barrier above ordered the LDS adds)
    for (uint32_t q = threadIdx.x; q < 2u * (nr + 1u); q += kRulesBlock) {
        const unsigned long long v = s_hits[q];
        if (v) atomicAdd(&a.hits[q], v);
    }
}

// One workgroup per batch: its tiles' kept counts into exclusive bases, and the batch's counts. A tile's dropped
// bytes stay below 2^24 (256 lines of at most 65535), so they are summed in 64 bits.
__global__ __launch_bounds__(kRulesScanBlock) void rules_scan_kernel(RulesArgs a) {
    __shared__ uint32_t s_n[kRulesMaxBatches], s_t0[kRulesMaxBatches + 1];
    __shared__ uint32_t s_wave[kRulesScanBlock / 64][3];
    __shared__ unsigned long long s_bytes[kRulesScanBlock / 64];
    (void)rules_tiles(a, s_n, s_t0);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x;   // < nb
    const uint32_t t0 = s_t0[j], nt = s_t0[j + 1] - t0;
    uint64_t run_k = 0, run_d = 0, run_b = 0, run_s = 0;
    for (uint32_t g0 = 0; g0 < nt; g0 += (uint32_t)kRulesScanBlock) {
        const uint32_t g = g0 + tid;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (g < nt) e = a.tiles[t0 + g];
        const uint32_t ik = wave_incl_add32(e.x), sd = stats_wave_sum(e.y), ss = stats_wave_sum(e.w);
        const uint64_t sb = stats_wave_sum64((uint64_t)e.z);
        if (lane == 63u) {
            s_wave[wave][0] = ik;
            s_wave[wave][1] = sd;
            s_wave[wave][2] = ss;
            s_bytes[wave] = sb;
        }
        __syncthreads();
        uint32_t before_k = 0, all_k = 0, all_d = 0, all_s = 0;
        uint64_t all_b = 0;
        for (uint32_t w = 0; w < (uint32_t)kRulesScanBlock / 64u; ++w) {
            before_k += w < wave ? s_wave[w][0] : 0u;
            all_k += s_wave[w][0];
            all_d += s_wave[w][1];
            all_s += s_wave[w][2];
            all_b += s_bytes[w];
        }
        if (g < nt) a.tiles[t0 + g] = make_uint4((uint32_t)(run_k + before_k + (ik - e.x)), 0u, 0u, 0u);
        run_k += all_k;
        run_d += all_d;
        run_b += all_b;
        run_s += all_s;
        __syncthreads();
    }
    if (tid == 0) {
        uint64_t *const c = a.b[j].counts;
        c[0] = run_k;
        c[1] = run_d;
        c[2] = run_b;
        c[3] = run_s;
    }
}

__global__ __launch_bounds__(kRulesBlock) void rules_emit_kernel(RulesArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_action[sizeof(RulesTable::action)];
    __shared__ uint32_t s_n[kRulesMaxBatches], s_t0[kRulesMaxBatches + 1];
    __shared__ uint32_t s_wave[kRulesWaves];
    const uint32_t ntiles = rules_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    if (threadIdx.x < sizeof(s_action) / 16u)
        reinterpret_cast<uint4 *>(s_action)[threadIdx.x] = reinterpret_cast<const uint4 *>(a.table->action)[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;
        const RulesBatchArg &b = a.b[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kRulesTile + threadIdx.x;
        bool kept = false;
        uint2 w = make_uint2(0u, 0u);
        if (i < s_n[j]) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(b.recs + i);
            w = make_uint2(r[0], r[1]);
            const uint32_t idx = b.match[i];
            kept = idx == SR_RULES_NOT_SUBJECT || s_action[idx] != SR_RULE_DROP;   // idx <= n_rules <= 256
        }
        const uint64_t km = __ballot(kept);
        const uint32_t rank = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
        if (lane == 0u) s_wave[wave] = (uint32_t)__builtin_popcountll(km);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t q = 0; q < (uint32_t)kRulesWaves; ++q) before += q < wave ? s_wave[q] : 0u;
        if (kept) {   // kept ranks stay below the batch's records, so below max_records
            const uint32_t at = a.tiles[tile].x + before + rank;
            uint32_t *const o = reinterpret_cast<uint32_t *>(b.out + at);
            o[0] = w.x;
            o[1] = w.y;
            if (b.hashes_out) b.hashes_out[at] = b.hashes[i];
        }
        __syncthreads();
    }
}

// The host-memory path (sr_set_name_rules): the stage's four counts and the batch's input record count into the
// slot's page-locked memory (device-mapped); with sr_set_trace and without the coalescing (whose own out kernel
// does it then) also the input-order records and the hashes, which pack_out_kernel would cut at the kept count.
struct RulesOut {
    const uint64_t *counts;      // the stage's four
    const uint64_t *n_records;   // the route launch's count
    uint64_t rec_cap;
    uint64_t *h_counts;          // device-mapped: 4 counts, then the input records
    const sr_record *recs;       // sr_set_trace (else null)
    const uint64_t *hashes;
    sr_record *h_recs;
    uint64_t *h_hashes;
};

__global__ __launch_bounds__(kRulesBlock) void rules_out_kernel(RulesOut o) {
    const uint64_t tid = (uint64_t)blockIdx.x * kRulesBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kRulesBlock;
    const uint64_t nr = min(*o.n_records, o.rec_cap);
    if (tid < 4) o.h_counts[tid] = o.counts[tid];
    if (tid == 4) o.h_counts[4] = *o.n_records;
    if (o.recs) {
        for (uint64_t i = tid; i < nr; i += stride) {
            o.h_recs[i] = o.recs[i];
            o.h_hashes[i] = o.hashes[i];
        }
    }
}

// The stage's device state on the host side (sr_rules_open, sr_rules).
struct RulesState {
    int open;
    uint32_t n_rules;
    RulesTable *d_table;
    unsigned long long *d_hits;   // kRulesHitCells
    uint16_t *d_match;            // per record of a call, for batches without d_match
    size_t match_cap;
    uint4 *d_tiles;               // per tile of a call
    size_t tiles_cap;
};

}  // namespace srk
