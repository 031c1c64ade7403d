// stats_kernel.hpp — name statistics on the device (include/sr_route.h).
//
// Behind a route launch the input-order records and the 64-bit name hashes are on the device. Two kernels
// turn them into the context's statistics; all ordering is by kernel boundaries, no workgroup waits for
// another, no atomic returns a value that a wait depends on.
//
//   stats_count_kernel  At most kStatsGroups workgroups (a constant, not read from the machine; fewer for few
//                       records) walk the launch's tiles of kStatsTile records; the tiles are numbered by the
//                       device's record counts, so room in max_records that holds no record costs nothing and
//                       a workgroup without a tile ends at once. A workgroup keeps a private
//                       copy of the whole count-min sketch in LDS as u32 cells (LDS atomics) and adds it into
//                       the global u64 cells once, at its end: the non-zero cells only, which are contiguous
//                       when the sketch is dense and few when the launch is small. Per-shard lines and bytes
//                       go the same way up to kStatsLdsShards shards; above that each wave aggregates equal
//                       shards before any global atomic. Per-verdict sums stay in registers until the end.
//                       Before the updates a wave settles runs of one name: up to kStatsPeel times the first
//                       undecided lane's name (and shard) is matched against the wave, and its lane acts for all of them
//                       with their count and bytes (a launch of one name costs one LDS atomic per row and
//                       wave, not 64 on one address). HyperLogLog registers are monotone: a plain load, and an
//                       atomic max only when rho is larger (a stale read costs an extra atomic, never a wrong
//                       value).
//   stats_hot_kernel    The same tiling. It ends at once while total < hot_min_lines. Else the workgroup
//                       first reduces the merged sketch to one bit per cell (cell >= T) in LDS, so a record's
//                       test is cms_rows LDS reads. Hot records of one name are settled in the wave (one lane
//                       per distinct name) and then in the workgroup (a direct-mapped LDS cache of names
//                       already inserted) before anything touches the global table.
//
// The hot table: open addressing over hot_slots slots. A slot's key is two write-once 64-bit words, A = the
// hash's high half and B = its low half, each shifted up with bit 0 set (0 = empty), claimed with a
// compare-and-swap each. An inserter walks the slots from the name's start slot; at a slot it takes or
// reads A, goes on to the next slot if A is another name's, then does the same with B. Both words settle once
// and every inserter of a name sees the same settled words in the same order, so all stop at the same slot:
// no duplicates and no waiting, and a slot always ends up holding one whole candidate (when two names that
// share their high half race for a slot, the one that loses B walks on). Whoever sets B writes the name's
// bytes; nothing reads names inside the kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "stats_host.hpp"

namespace srk {

// 16 waves share one LDS sketch: a record costs two global loads (record, hash), and with one workgroup per
// CU the waves in flight are what hides them
constexpr int kStatsBlock = 1024;           // threads per workgroup
constexpr int kStatsPerThread = 1;
constexpr int kStatsTile = kStatsBlock * kStatsPerThread;   // records per tile (R of the tests)
constexpr int kStatsGroups = 256;           // most workgroups of a launch
constexpr int kStatsTilesPerGroup = 4;      // a smaller launch gets fewer workgroups: ceil(tiles / this)
constexpr int kStatsLdsShards = 512;        // per-shard sums in LDS up to this many shards
constexpr int kStatsPeel = 2;               // rounds of settling equal names in a wave
constexpr int kStatsMaxBatches = 32;
constexpr int kStatsHotCache = 256;         // names a workgroup remembers having inserted
// The grid is sized by the records a batch can hold: max_records, but no more than one per this many bytes.
// A grid smaller than the tiles only means more tiles per workgroup (they stride), so shorter lines stay correct.
constexpr uint32_t kStatsGridLineBytes = 16;
// A workgroup adds at most kStatsTile to an LDS cell per tile and flushes after this many tiles: a cell never
// passes 2^30.
constexpr uint32_t kStatsFlushTiles = 1u << 20;

struct StatsHotName {
    uint32_t name_len;
    uint8_t name[SR_STATS_NAME_MAX];
};
static_assert(sizeof(StatsHotName) == 112 && sizeof(sr_stats_hot) == 128, "hot entry layout");

enum : int { kStatsCtrLines = 0, kStatsCtrBytes = 4, kStatsCtrIgnored = 8, kStatsCtrOverflow = 9, kStatsCtrs = 16 };

struct StatsBatchArg {
    const uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;
    uint32_t nbytes, max_records;
};

struct StatsArgs {
    StatsBatchArg b[kStatsMaxBatches];
    unsigned long long *ctr;      // kStatsCtrs
    unsigned long long *shard;    // [2][nds]: lines, bytes
    unsigned long long *cells;    // [rows * width]
    uint32_t *regs;               // [nds << p], one register per word
    unsigned long long *key_a, *key_b;   // [slots]
    StatsHotName *names;          // [slots]
    uint32_t nb, nds, p, rows, width, slots, hot_div, hot_min;
};

__device__ __forceinline__ uint32_t stats_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ uint64_t stats_shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t stats_wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

// The launch's real tiles. The host sizes the grid by max_records; the device knows the counts: batch j has
// ceil(min(*n_records, max_records) / kStatsTile) tiles, numbered back to back. One load per batch and
// workgroup, all in flight together: s_n[j] = the batch's records, s_t0[j] = its first tile, s_t0[32] = the
// total, which is returned. A workgroup without a tile ends before it touches anything else.
__device__ __forceinline__ uint32_t stats_tiles(const StatsArgs &a, uint32_t *s_n, uint32_t *s_t0) {
    if (threadIdx.x < kStatsMaxBatches) {
        uint32_t n = 0;
        if (threadIdx.x < a.nb) {
            const StatsBatchArg &b = a.b[threadIdx.x];
            const uint64_t nrec = *b.n_records;
            n = (uint32_t)(nrec < b.max_records ? nrec : b.max_records);
        }
        s_n[threadIdx.x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int j = 0; j < kStatsMaxBatches; ++j) {
            s_t0[j] = t;
            t += (s_n[j] + (uint32_t)kStatsTile - 1u) / (uint32_t)kStatsTile;
        }
        s_t0[kStatsMaxBatches] = t;
    }
    __syncthreads();
    return s_t0[kStatsMaxBatches];
}

// The LDS copies into the global sums: the non-zero entries only, which are then zero again.
__device__ __forceinline__ void stats_flush(const StatsArgs &a, uint32_t *s_cells, unsigned long long *s_shard,
                                            bool lds_shards) {
    const uint32_t ncells = a.rows * a.width;
    for (uint32_t c = threadIdx.x; c < ncells; c += kStatsBlock) {
        const uint32_t v = s_cells[c];
        if (v) {
            atomicAdd(&a.cells[c], (unsigned long long)v);
            s_cells[c] = 0u;
        }
    }
    if (lds_shards)
        for (uint32_t k = threadIdx.x; k < 2u * a.nds; k += kStatsBlock) {
            const unsigned long long v = s_shard[k];
            if (v) {
                atomicAdd(&a.shard[k], v);
                s_shard[k] = 0ull;
            }
        }
}

template <bool kLdsShards>
__global__ __launch_bounds__(kStatsBlock) void stats_count_kernel(StatsArgs a) {
    extern __shared__ uint32_t s_cells[];   // rows * width
    __shared__ unsigned long long s_shard[kLdsShards ? 2 * kStatsLdsShards : 2];
    __shared__ unsigned long long s_ctr[9];
    __shared__ uint32_t s_n[kStatsMaxBatches], s_t0[kStatsMaxBatches + 1];
    const uint32_t ncells = a.rows * a.width, wmask = a.width - 1u;
    const int lane = threadIdx.x & 63;
    const uint32_t ntiles = stats_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    for (uint32_t c = threadIdx.x; c < ncells; c += kStatsBlock) s_cells[c] = 0u;
    if (kLdsShards)
        for (uint32_t k = threadIdx.x; k < 2u * a.nds; k += kStatsBlock) s_shard[k] = 0ull;
    if (threadIdx.x < 9) s_ctr[threadIdx.x] = 0ull;
    __syncthreads();

    uint64_t c_lines[4] = {0, 0, 0, 0}, c_bytes[4] = {0, 0, 0, 0}, c_ignored = 0;
    uint32_t since = 0;
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;   // t < ntiles = s_t0[32]: j stays below the batch count
        const StatsBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t base = (t - s_t0[j]) * (uint32_t)kStatsTile;
#pragma unroll 1
        for (int k = 0; k < kStatsPerThread; ++k) {
            const uint32_t i = base + (uint32_t)k * kStatsBlock + threadIdx.x;
            uint32_t len = 0, route = 0xFFFCu;   // out of range: treated as neither valid nor counted
            const bool in = i < n;
            uint64_t h = 0;
            if (in) {   // both loads leave together: the hash does not wait for the record's verdict
                const uint2 w = *reinterpret_cast<const uint2 *>(b.recs + i);
                h = b.hashes[i];
                len = w.y & 0xFFFFu;
                route = w.y >> 16;
            }
            const bool valid = in && route < a.nds;
            if (in) {
                const uint32_t v = route < a.nds ? 0u : route >= SR_ROUTE_INVALID_LENGTH ? route - 0xFFFCu : 4u;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    c_lines[q] += v == q ? 1u : 0u;
                    c_bytes[q] += v == q ? len : 0u;
                }
                c_ignored += v == 4u ? 1u : 0u;
            }
            const uint64_t vmask = __ballot(valid);
            if (!vmask) continue;
            const uint64_t m = valid ? stats_fmix64(h) : 0ull;
            // runs of one name: the first undecided lane acts for every lane with its name
            bool act = valid;
            uint32_t cnt = 1u, bsum = len;
            uint64_t rem = vmask;
            for (int round = 0; round < kStatsPeel && rem; ++round) {
                const int lead = __builtin_ctzll(rem);
                const uint64_t lm = stats_shfl64(m, lead);
                const uint32_t lr = __shfl(route, lead);
                // equal hash AND equal shard: the route kernel gives equal names one shard, a caller's own
                // records need not, and every record counts under its own route
                const bool mine = valid && ((rem >> lane) & 1ull) && m == lm && route == lr;
                const uint64_t same = __ballot(mine);
                rem &= ~same;
                if (__builtin_popcountll(same) > 1) {
                    const uint32_t s = stats_wave_sum(mine ? len : 0u);
                    if (mine) {
                        act = lane == lead;
                        cnt = (uint32_t)__builtin_popcountll(same);
                        bsum = s;
                    }
                }
            }
            if (act) {
                for (uint32_t r = 0; r < a.rows; ++r) atomicAdd(&s_cells[r * a.width + stats_cell(m, r, wmask)], cnt);
                const uint32_t idx = (uint32_t)(m >> (64u - a.p));
                const uint64_t w = m << a.p;
                const uint32_t rho = w ? (uint32_t)__builtin_clzll(w) + 1u : 64u - a.p + 1u;
                uint32_t *reg = a.regs + (((size_t)route << a.p) + idx);
                if (*reg < rho) (void)__hip_atomic_fetch_max(reg, rho, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (kLdsShards) {
                    atomicAdd(&s_shard[route], (unsigned long long)cnt);
                    atomicAdd(&s_shard[a.nds + route], (unsigned long long)bsum);
                }
            }
            if (!kLdsShards) {   // equal shards aggregated in the wave, then one pair of global atomics each
                uint64_t left = __ballot(act);
                while (left) {
                    const int lead = __builtin_ctzll(left);
                    const uint32_t ls = __shfl(route, lead);
                    const bool mine = act && route == ls;
                    left &= ~__ballot(mine);
                    const uint32_t c = stats_wave_sum(mine ? cnt : 0u), s = stats_wave_sum(mine ? bsum : 0u);
                    if (lane == lead) {
                        atomicAdd(&a.shard[ls], (unsigned long long)c);
                        atomicAdd(&a.shard[a.nds + ls], (unsigned long long)s);
                    }
                }
            }
        }
        if (++since == kStatsFlushTiles) {
            __syncthreads();
            stats_flush(a, s_cells, s_shard, kLdsShards);
            __syncthreads();
            since = 0;
        }
    }
    // the per-verdict sums: registers -> wave -> LDS -> one global atomic each
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t l = stats_wave_sum64(c_lines[q]), s = stats_wave_sum64(c_bytes[q]);
        if (lane == 0 && l) {
            atomicAdd(&s_ctr[q], (unsigned long long)l);
            atomicAdd(&s_ctr[4 + q], (unsigned long long)s);
        }
    }
    {
        const uint64_t g = stats_wave_sum64(c_ignored);
        if (lane == 0 && g) atomicAdd(&s_ctr[8], (unsigned long long)g);
    }
    __syncthreads();
    stats_flush(a, s_cells, s_shard, kLdsShards);
    if (threadIdx.x < 9 && s_ctr[threadIdx.x]) atomicAdd(&a.ctr[threadIdx.x], s_ctr[threadIdx.x]);
}

// The name of record (off, len) of batch b into slot s: the bytes before the first ':' inside the line
// clipped to [0, nbytes). The slot's name bytes are zero since the last reset and written once.
__device__ __forceinline__ void stats_write_name(const StatsArgs &a, const StatsBatchArg &b, uint32_t off, uint32_t len,
                                                 uint32_t s) {
    const uint32_t start = off < b.nbytes ? off : b.nbytes;
    const uint64_t e64 = (uint64_t)off + len;
    const uint32_t end = e64 < b.nbytes ? (uint32_t)e64 : b.nbytes;
    uint32_t k = start;
    while (k < end && b.bytes[k] != (uint8_t)':') ++k;
    const uint32_t name_len = k - start;
    StatsHotName &o = a.names[s];
    const uint32_t keep = name_len < SR_STATS_NAME_MAX ? name_len : SR_STATS_NAME_MAX;
    for (uint32_t q = 0; q < keep; ++q) o.name[q] = b.bytes[start + q];
    o.name_len = name_len;
}

// One name into the global table (see the head of this file). Returns nothing: a full table sets the flag.
__device__ __forceinline__ void stats_hot_insert(const StatsArgs &a, const StatsBatchArg &b, uint64_t h, uint64_t m,
                                                 uint32_t off, uint32_t len) {
    const unsigned long long ka = (h >> 32) << 32 | 1ull, kb = (h & 0xFFFFFFFFull) << 32 | 1ull;
    const uint32_t mask = a.slots - 1u, start = (uint32_t)(m >> 40) & mask;
    for (uint32_t probe = 0; probe < a.slots; ++probe) {
        const uint32_t s = (start + probe) & mask;
        unsigned long long oa = __hip_atomic_load(&a.key_a[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (oa == 0ull) oa = atomicCAS(&a.key_a[s], 0ull, ka);
        if (oa != 0ull && oa != ka) continue;
        unsigned long long ob = __hip_atomic_load(&a.key_b[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ob == 0ull) ob = atomicCAS(&a.key_b[s], 0ull, kb);
        if (ob == 0ull) {
            stats_write_name(a, b, off, len, s);
            return;
        }
        if (ob == kb) return;
    }
    atomicOr(&a.ctr[kStatsCtrOverflow], 1ull);
}

__global__ __launch_bounds__(kStatsBlock) void stats_hot_kernel(StatsArgs a) {
    __shared__ uint32_t s_bits[SR_STATS_MAX_CELLS / 32];
    __shared__ unsigned long long s_seen[kStatsHotCache];
    __shared__ uint32_t s_seen_ok[kStatsHotCache];
    __shared__ uint32_t s_n[kStatsMaxBatches], s_t0[kStatsMaxBatches + 1];
    const unsigned long long total = a.ctr[kStatsCtrLines];
    if (total < a.hot_min) return;
    const uint32_t ntiles = stats_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const unsigned long long per = (total + a.hot_div - 1ull) / a.hot_div;
    const unsigned long long T = per > a.hot_min ? per : (unsigned long long)a.hot_min;
    const uint32_t ncells = a.rows * a.width, wmask = a.width - 1u;   // ncells is a multiple of 256
    const int lane = threadIdx.x & 63;
    // a wave turns 64 consecutive cells into two words; eight such loads are in flight per lane
    for (uint32_t c0 = (threadIdx.x >> 6) * 64u; c0 < ncells; c0 += kStatsBlock * 8u) {
        unsigned long long v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t c = c0 + u * kStatsBlock + lane;
            v[u] = c < ncells ? a.cells[c] : 0ull;
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t c = c0 + u * kStatsBlock;
            const uint64_t bal = __ballot(v[u] >= T);
            if (lane == 0 && c < ncells) {
                s_bits[c >> 5] = (uint32_t)bal;
                s_bits[(c >> 5) + 1u] = (uint32_t)(bal >> 32);
            }
        }
    }
    for (uint32_t k = threadIdx.x; k < kStatsHotCache; k += kStatsBlock) s_seen_ok[k] = 0u;
    __syncthreads();
    int j = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        while (s_t0[j + 1] <= t) ++j;
        const StatsBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t base = (t - s_t0[j]) * (uint32_t)kStatsTile;
#pragma unroll 1
        for (int k = 0; k < kStatsPerThread; ++k) {
            const uint32_t i = base + (uint32_t)k * kStatsBlock + threadIdx.x;
            bool hot = false;
            uint32_t off = 0, len = 0;
            uint64_t h = 0, m = 0;
            if (i < n) {
                const uint2 w = *reinterpret_cast<const uint2 *>(b.recs + i);
                h = b.hashes[i];   // with the record, not behind its verdict
                off = w.x;
                len = w.y & 0xFFFFu;
                if ((w.y >> 16) < a.nds) {
                    m = stats_fmix64(h);
                    hot = true;
                    for (uint32_t r = 0; r < a.rows; ++r) {
                        const uint32_t c = r * a.width + stats_cell(m, r, wmask);
                        hot = hot && ((s_bits[c >> 5] >> (c & 31u)) & 1u);
                    }
                }
            }
            // one lane per distinct hot name of the wave
            uint64_t rem = __ballot(hot);
            bool leader = false;
            while (rem) {
                const int lead = __builtin_ctzll(rem);
                const uint64_t lh = stats_shfl64(h, lead);
                rem &= ~__ballot(hot && h == lh);
                leader = leader || lane == lead;
            }
            if (leader) {
                const uint32_t ci = (uint32_t)(m >> 20) & (kStatsHotCache - 1);
                // Waves share the cache without a barrier. An entry is one 64-bit LDS atomic store and load, so a
                // reader sees a whole hash that some wave stored, never halves of two; and a wave stores a hash
                // only when its own insert of it is issued, which completes before the kernel ends whoever
                // skips meanwhile. The flag only says that the entry was ever written.
                const bool known = s_seen_ok[ci] &&
                                   __hip_atomic_load(&s_seen[ci], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == h;
                if (!known) {
                    stats_hot_insert(a, b, h, m, off, len);
                    __hip_atomic_store(&s_seen[ci], (unsigned long long)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    s_seen_ok[ci] = 1u;
                }
            }
        }
    }
}

// The stage's device state on the host side (sr_stats_open): one allocation and the offsets of its parts.
struct StatsState {
    int open;
    sr_stats_config cfg;   // effective values
    uint8_t *d_base;
    size_t bytes, o_shard, o_cells, o_ka, o_kb, o_names, o_regs;
};

}  // namespace srk
