// coalesce_kernel.hpp — plain counters coalesced on the device (include/sr_route.h).
//
// Behind a route launch the input-order records and the 64-bit name hashes are on the device. Six launches turn
// them into a shorter record list and the merged lines' text behind the batch. All ordering is by kernel
// boundaries: no workgroup waits for another, no atomic returns a value that a wait depends on.
//
//   coalesce_clear_kernel  the launch's tables (one of `slots` entries per batch): owner = none, members = 0,
//                          sum = 0, one 16-byte store per entry.
//   coalesce_claim_kernel  one record per thread, tiles of kCoalesceTile records numbered by the device's record
//                          counts (stats_kernel.hpp's scheme: the grid is sized by what a batch plausibly holds,
//                          the tiles stride). The line is parsed once (coalesce_host.hpp's grammar, the very
//                          function sr_coalesce_parse runs); k, the value and a flag go to the record's scratch
//                          word pair; then atomicMin(index) on the slot's owner. Before the atomic a wave
//                          settles runs of one slot: up to kCoalescePeel times the first undecided lane's slot
//                          is matched against the wave, and that lane (the lowest index) acts alone for all of
//                          them, so a launch of one name costs one atomic per wave, not 64 on one address.
//   coalesce_join_kernel   a plain counter reads its slot's owner and joins it iff hash, route, k and the name
//                          bytes are equal (the owner joins itself without a compare). Joined lanes of one slot
//                          are one group: they are settled in the wave the same way, then one 64-bit add on
//                          the slot's sum and one 32-bit add on its member count per run.
//   coalesce_sum_kernel    per tile: records kept, groups merged (owners of two or more members) and the bytes
//                          of their merged lines.
//   coalesce_scan_kernel   one workgroup per batch turns the tile sums into exclusive bases (DPP wave scans, as
//                          log_scan_kernel) and writes the batch's four counts.
//   coalesce_emit_kernel   computes a tile's verdicts again (8 bytes of scratch per record are kept, the
//                          verdicts are not), ranks them in the workgroup and writes the kept records in input
//                          order. A merged line's name is copied by the whole wave, 64 bytes per step; the
//                          owner's lane writes ':' dec(sum) "|c\n" behind it. Every byte store checks the
//                          caller's append_cap.
// Vector stores only; no scratch memory: the decimal digits go straight to their places, no array holds them.
#pragma once

#include <hip/hip_runtime.h>

#include "coalesce_host.hpp"
#include "route_kernel.hpp"
#include "stats_kernel.hpp"

namespace srk {

constexpr int kCoalesceBlock = 256;              // threads per workgroup: four waves
constexpr int kCoalesceTile = kCoalesceBlock;    // records per tile (R of the tests), one per thread
constexpr int kCoalesceWaves = kCoalesceBlock / 64;
constexpr int kCoalesceGroups = 2048;            // most workgroups of a launch (eight per CU)
constexpr int kCoalesceMaxBatches = 32;
constexpr int kCoalescePeel = 2;                 // rounds of settling equal slots in a wave
constexpr int kCoalesceScanBlock = 1024;         // coalesce_scan_kernel: tiles per step
// The grid is sized by the records a batch can hold: max_records, but no more than one per this many bytes
// (§5.9). A grid smaller than the tiles only means more tiles per workgroup.
constexpr uint32_t kCoalesceGridLineBytes = 16;
constexpr uint32_t kCoalesceNoOwner = 0xFFFFFFFFu;   // record indices stay below 0xFFFFFFF0
// a record's scratch: x = k | flags, y = the value (an int32)
constexpr uint32_t kCoalescePlain = 1u << 16, kCoalesceJoined = 1u << 17, kCoalesceKMask = 0xFFFFu;

struct CoalesceSlot {
    uint32_t owner, members;
    unsigned long long sum;   // the group's values, two's complement
};
static_assert(sizeof(CoalesceSlot) == 16, "table entry layout");

struct CoalesceBatchArg {
    uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;
    sr_record *out;
    uint64_t *counts;
    uint2 *scratch;           // [max_records]
    uint64_t append_cap;
    uint32_t nbytes, max_records;
};

struct CoalesceArgs {
    CoalesceBatchArg b[kCoalesceMaxBatches];
    CoalesceSlot *table;      // [nb][slots]
    uint4 *tiles;             // per tile {kept, groups, bytes, -}, after the scan {kept base, -, byte base lo, hi}
    uint32_t nb, nds, slots;
};

// The launch's real tiles, as stats_tiles numbers them: batch j has ceil(min(*n_records, max_records) /
// kCoalesceTile) tiles, back to back. s_n[j] = the batch's records, s_t0[j] = its first tile, s_t0[32] = the
// total, which is returned.
__device__ __forceinline__ uint32_t coalesce_tiles(const CoalesceArgs &a, uint32_t *s_n, uint32_t *s_t0) {
    if (threadIdx.x < kCoalesceMaxBatches) {
        uint32_t n = 0;
        if (threadIdx.x < a.nb) {
            const CoalesceBatchArg &b = a.b[threadIdx.x];
            const uint64_t nrec = *b.n_records;
            n = (uint32_t)(nrec < b.max_records ? nrec : b.max_records);
        }
        s_n[threadIdx.x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int j = 0; j < kCoalesceMaxBatches; ++j) {
            s_t0[j] = t;
            t += (s_n[j] + (uint32_t)kCoalesceTile - 1u) / (uint32_t)kCoalesceTile;
        }
        s_t0[kCoalesceMaxBatches] = t;
    }
    __syncthreads();
    return s_t0[kCoalesceMaxBatches];
}

// a record as two words (sr_record is 4-byte aligned): offset, length | route << 16
__device__ __forceinline__ uint2 coalesce_load_rec(const sr_record *r) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(r);
    return make_uint2(w[0], w[1]);
}

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_clear_kernel(CoalesceSlot *table, uint32_t entries) {
    for (uint32_t e = blockIdx.x * (uint32_t)kCoalesceBlock + threadIdx.x; e < entries;
         e += gridDim.x * (uint32_t)kCoalesceBlock)
        *reinterpret_cast<uint4 *>(table + e) = make_uint4(kCoalesceNoOwner, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_claim_kernel(CoalesceArgs a) {
    __shared__ uint32_t s_n[kCoalesceMaxBatches], s_t0[kCoalesceMaxBatches + 1];
    const uint32_t ntiles = coalesce_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;   // t < ntiles = s_t0[32]: j stays below the batch count
        const CoalesceBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (t - s_t0[j]) * (uint32_t)kCoalesceTile + threadIdx.x;
        bool plain = false;
        uint32_t slot = 0;
        if (i < n) {
            const uint2 w = coalesce_load_rec(b.recs + i);
            const uint64_t h = b.hashes[i];   // with the record, not behind its verdict
            const uint32_t len = w.y & 0xFFFFu, route = w.y >> 16;
            uint32_t k = 0;
            int32_t v = 0;
            if (route < a.nds && len >= kCoalesceMinLine && len <= kCoalesceMaxLine && (uint64_t)w.x + len <= b.nbytes)
                plain = coalesce_parse(b.bytes + w.x, len, &k, &v);
            b.scratch[i] = make_uint2(plain ? (k | kCoalescePlain) : 0u, (uint32_t)v);
            slot = (uint32_t)stats_fmix64(h) & smask;
        }
        uint64_t rem = __ballot(plain);
        if (!rem) continue;
        // runs of one slot: the first undecided lane has the lowest index of them and claims for all
        bool act = plain;
        for (int round = 0; round < kCoalescePeel && rem; ++round) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t ls = __shfl(slot, lead);
            const bool mine = plain && ((rem >> lane) & 1ull) && slot == ls;
            rem &= ~__ballot(mine);
            if (mine) act = lane == lead;
        }
        if (act) atomicMin(&a.table[(size_t)j * a.slots + slot].owner, i);
    }
}

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_join_kernel(CoalesceArgs a) {
    __shared__ uint32_t s_n[kCoalesceMaxBatches], s_t0[kCoalesceMaxBatches + 1];
    const uint32_t ntiles = coalesce_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;
        const CoalesceBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (t - s_t0[j]) * (uint32_t)kCoalesceTile + threadIdx.x;
        CoalesceSlot *const table = a.table + (size_t)j * a.slots;
        bool join = false;
        uint32_t slot = 0;
        int32_t val = 0;
        if (i < n) {
            const uint2 s = b.scratch[i];
            if (s.x & kCoalescePlain) {
                const uint2 w = coalesce_load_rec(b.recs + i);
                const uint64_t h = b.hashes[i];
                slot = (uint32_t)stats_fmix64(h) & smask;
                const uint32_t o = table[slot].owner;   // a plain counter of this slot, at most i
                join = o == i;
                if (!join && o < n) {
                    const uint2 so = b.scratch[o], wo = coalesce_load_rec(b.recs + o);
                    const uint32_t k = s.x & kCoalesceKMask;
                    if (b.hashes[o] == h && (wo.y >> 16) == (w.y >> 16) && (so.x & kCoalesceKMask) == k) {
                        const uint8_t *p = b.bytes + w.x, *q = b.bytes + wo.x;   // both names lie inside the batch
                        uint32_t x = 0;
                        while (x < k && p[x] == q[x]) ++x;
                        join = x == k;
                    }
                }
                if (join) {
                    b.scratch[i] = make_uint2(s.x | kCoalesceJoined, s.y);
                    val = (int32_t)s.y;
                }
            }
        }
        uint64_t rem = __ballot(join);
        if (!rem) continue;
        // joined lanes of one slot joined one owner: one lane adds for the run
        bool act = join;
        uint32_t cnt = 1u;
        uint64_t vs = (uint64_t)(int64_t)val;
        for (int round = 0; round < kCoalescePeel && rem; ++round) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t ls = __shfl(slot, lead);
            const bool mine = join && ((rem >> lane) & 1ull) && slot == ls;
            const uint64_t same = __ballot(mine);
            rem &= ~same;
            if (__builtin_popcountll(same) > 1) {
                const uint64_t sum = stats_wave_sum64(mine ? (uint64_t)(int64_t)val : 0ull);
                if (mine) {
                    act = lane == lead;
                    cnt = (uint32_t)__builtin_popcountll(same);
                    vs = sum;
                }
            }
        }
        if (act) {
            atomicAdd(&table[slot].sum, (unsigned long long)vs);
            atomicAdd(&table[slot].members, cnt);
        }
    }
}

// What becomes of record i of its batch: kept or dropped, and for the owner of a group of two or more the
// merged line's length and sum.
struct CoalesceVerdict {
    uint2 w;          // the record
    bool kept, merged;
    uint32_t k, mlen;
    int64_t sum;
};

__device__ __forceinline__ CoalesceVerdict coalesce_verdict(const CoalesceBatchArg &b, const CoalesceSlot *table,
                                                            uint32_t smask, uint32_t i, uint32_t n) {
    CoalesceVerdict v;
    v.w = make_uint2(0u, 0u);
    v.kept = i < n;
    v.merged = false;
    v.k = v.mlen = 0u;
    v.sum = 0;
    if (i < n) {
        v.w = coalesce_load_rec(b.recs + i);
        const uint2 s = b.scratch[i];
        if (s.x & kCoalesceJoined) {
            const uint4 e = *reinterpret_cast<const uint4 *>(table + ((uint32_t)stats_fmix64(b.hashes[i]) & smask));
            if (e.y >= 2u) {
                if (e.x == i) {
                    v.merged = true;
                    v.k = s.x & kCoalesceKMask;
                    v.sum = (int64_t)((uint64_t)e.w << 32 | e.z);
                    v.mlen = coalesce_line_len(v.k, v.sum);
                } else {
                    v.kept = false;
                }
            }
        }
    }
    return v;
}

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_sum_kernel(CoalesceArgs a) {
    __shared__ uint32_t s_n[kCoalesceMaxBatches], s_t0[kCoalesceMaxBatches + 1];
    __shared__ uint32_t s_wave[kCoalesceWaves][3];
    const uint32_t ntiles = coalesce_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;
        const uint32_t i = (t - s_t0[j]) * (uint32_t)kCoalesceTile + threadIdx.x;
        const CoalesceVerdict v = coalesce_verdict(a.b[j], a.table + (size_t)j * a.slots, smask, i, s_n[j]);
        const uint32_t kept = (uint32_t)__builtin_popcountll(__ballot(v.kept));
        const uint32_t groups = (uint32_t)__builtin_popcountll(__ballot(v.merged));
        const uint32_t bytes = stats_wave_sum(v.mlen);
        if (lane == 0u) {
            s_wave[wave][0] = kept;
            s_wave[wave][1] = groups;
            s_wave[wave][2] = bytes;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = 0, g = 0, m = 0;
            for (int w = 0; w < kCoalesceWaves; ++w) {
                k += s_wave[w][0];
                g += s_wave[w][1];
                m += s_wave[w][2];
            }
            a.tiles[t] = make_uint4(k, g, m, 0u);
        }
        __syncthreads();
    }
}

// One workgroup per batch: its tiles' sums into exclusive bases, and the batch's counts. A tile's bytes stay
// below 2^19 (256 lines of at most 1449), 1024 of them below 2^29; the running totals are 64 bits.
__global__ __launch_bounds__(kCoalesceScanBlock) void coalesce_scan_kernel(CoalesceArgs a) {
    __shared__ uint32_t s_n[kCoalesceMaxBatches], s_t0[kCoalesceMaxBatches + 1];
    __shared__ uint32_t s_wave[kCoalesceScanBlock / 64][3];
    (void)coalesce_tiles(a, s_n, s_t0);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x;   // < nb
    const uint32_t t0 = s_t0[j], nt = s_t0[j + 1] - t0;
    uint64_t run_k = 0, run_g = 0, run_b = 0;
    for (uint32_t g0 = 0; g0 < nt; g0 += (uint32_t)kCoalesceScanBlock) {
        const uint32_t g = g0 + tid;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (g < nt) e = a.tiles[t0 + g];
        const uint32_t ik = wave_incl_add32(e.x), ig = wave_incl_add32(e.y), ib = wave_incl_add32(e.z);
        if (lane == 63u) {
            s_wave[wave][0] = ik;
            s_wave[wave][1] = ig;
            s_wave[wave][2] = ib;
        }
        __syncthreads();
        uint32_t before_k = 0, before_b = 0, all_k = 0, all_g = 0, all_b = 0;
        for (uint32_t w = 0; w < (uint32_t)kCoalesceScanBlock / 64u; ++w) {
            before_k += w < wave ? s_wave[w][0] : 0u;
            before_b += w < wave ? s_wave[w][2] : 0u;
            all_k += s_wave[w][0];
            all_g += s_wave[w][1];
            all_b += s_wave[w][2];
        }
        if (g < nt) {
            const uint64_t kb = run_k + before_k + (ik - e.x), bb = run_b + before_b + (ib - e.z);
            a.tiles[t0 + g] = make_uint4((uint32_t)kb, 0u, (uint32_t)bb, (uint32_t)(bb >> 32));
        }
        run_k += all_k;
        run_g += all_g;
        run_b += all_b;
        __syncthreads();
    }
    if (tid == 0) {
        uint64_t *const c = a.b[j].counts;
        c[0] = run_k;
        c[1] = (uint64_t)s_n[j] - run_k;
        c[2] = run_g;
        c[3] = run_b;
    }
}

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_emit_kernel(CoalesceArgs a) {
    __shared__ uint32_t s_n[kCoalesceMaxBatches], s_t0[kCoalesceMaxBatches + 1];
    __shared__ uint32_t s_wave[kCoalesceWaves][2];
    const uint32_t ntiles = coalesce_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;
        const CoalesceBatchArg &b = a.b[j];
        const uint32_t i = (t - s_t0[j]) * (uint32_t)kCoalesceTile + threadIdx.x;
        const CoalesceVerdict v = coalesce_verdict(b, a.table + (size_t)j * a.slots, smask, i, s_n[j]);
        const uint64_t km = __ballot(v.kept);
        const uint32_t rank = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
        const uint32_t ib = wave_incl_add32(v.mlen);
        if (lane == 63u) {
            s_wave[wave][0] = (uint32_t)__builtin_popcountll(km);
            s_wave[wave][1] = ib;
        }
        __syncthreads();
        uint32_t before_k = 0, before_b = 0;
        for (uint32_t w = 0; w < (uint32_t)kCoalesceWaves; ++w) {
            before_k += w < wave ? s_wave[w][0] : 0u;
            before_b += w < wave ? s_wave[w][1] : 0u;
        }
        const uint4 base = a.tiles[t];
        // the merged line's place in the appended text (64 bits: made-up records may overlap and pass 2^32)
        const uint64_t at = ((uint64_t)base.w << 32 | base.z) + before_b + (ib - v.mlen);
        if (v.kept) {   // kept ranks stay below the batch's records, so below max_records
            uint32_t *const o = reinterpret_cast<uint32_t *>(b.out + (base.x + before_k + rank));
            o[0] = v.merged ? (uint32_t)(b.nbytes + at) : v.w.x;
            o[1] = v.merged ? (v.mlen | (v.w.y & 0xFFFF0000u)) : v.w.y;
        }
        uint8_t *const text = b.bytes + b.nbytes;
        uint64_t mm = __ballot(v.merged);
        while (mm) {   // the wave copies one merged name at a time
            const int lead = __builtin_ctzll(mm);
            mm &= mm - 1ull;
            const uint32_t src = __shfl(v.w.x, lead), k = __shfl(v.k, lead);
            const uint64_t dst = stats_shfl64(at, lead);
            for (uint32_t q = lane; q < k; q += 64u)
                if (dst + q < b.append_cap) text[dst + q] = b.bytes[src + q];
        }
        if (v.merged) {
            const uint64_t tail = at + v.k;
            (void)coalesce_put_tail(text + tail, tail < b.append_cap ? b.append_cap - tail : 0ull, v.sum);
        }
        __syncthreads();
    }
}

// The host-memory path (sr_set_coalesce): the merged text, the four counts and the batch's input record count
// copied into the slot's page-locked memory (device-mapped), sized by the device's own counts as pack_out_kernel
// sizes its copies; with sr_set_trace also the input-order records and the hashes, which pack_out_kernel would
// cut at the coalesced count. The text's source has any alignment, its destination is aligned: a thread composes
// 16 bytes and stores them once.
struct CoalesceOut {
    const uint8_t *text;         // d_bytes + nbytes
    const uint64_t *counts;      // the stage's four
    const uint64_t *n_records;   // the route launch's count
    uint64_t text_cap, rec_cap;
    uint8_t *h_text;             // device-mapped host pointers
    uint64_t *h_counts;          // 4 counts, then the input records
    const sr_record *recs;       // sr_set_trace (else null)
    const uint64_t *hashes;
    sr_record *h_recs;
    uint64_t *h_hashes;
};

__global__ __launch_bounds__(kCoalesceBlock) void coalesce_out_kernel(CoalesceOut o) {
    const uint64_t tid = (uint64_t)blockIdx.x * kCoalesceBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kCoalesceBlock;
    const uint64_t nb = min(o.counts[3], o.text_cap), nr = min(*o.n_records, o.rec_cap);
    for (uint64_t p = tid; p < nb / 16u; p += stride) {
        const uint8_t *s = o.text + p * 16u;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = (uint32_t)s[4 * q] | (uint32_t)s[4 * q + 1] << 8 | (uint32_t)s[4 * q + 2] << 16 | (uint32_t)s[4 * q + 3] << 24;
        reinterpret_cast<uint4 *>(o.h_text)[p] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (uint64_t x = (nb & ~15ull) + tid; x < nb; x += stride) o.h_text[x] = o.text[x];
    if (tid < 4) o.h_counts[tid] = o.counts[tid];
    if (tid == 4) o.h_counts[4] = *o.n_records;
    if (o.recs) {
        for (uint64_t i = tid; i < nr; i += stride) {
            o.h_recs[i] = o.recs[i];
            o.h_hashes[i] = o.hashes[i];
        }
    }
}

// The stage's device state on the host side (sr_coalesce_open, sr_coalesce).
struct CoalesceState {
    int open;
    uint32_t slots;
    CoalesceSlot *d_table;    // [SR_MAX_BATCHES_PER_LAUNCH][slots]
    uint2 *d_scratch;         // per record of a call
    size_t scratch_cap;
    uint4 *d_tiles;           // per tile of a call
    size_t tiles_cap;
};

}  // namespace srk
