// validate_kernel.hpp — the line grammar on the device (include/sr_route.h).
//
// Behind a route launch the input-order records are on the device. Three launches turn them into the list of the
// records whose lines the grammar keeps, in the shape of rules_kernel.hpp. All ordering is by kernel boundaries: no
// workgroup waits for another, no atomic returns a value that a wait depends on.
//
//   validate_check_kernel  one record per thread, tiles of kValidTile records numbered by the device's record
//                          counts (rules_kernel.hpp's scheme). A thread takes its line in 16-byte steps: aligned
//                          uint4 loads (rules_block: a block that is not wholly inside the batch is read byte by
//                          byte, its bytes inside the batch only), two neighbouring blocks put together with
//                          v_alignbyte (rules_shift). The loads do not depend on the judgement: the block two
//                          ahead is requested before the current step is judged. A step is judged by
//                          validate_step (validate_host.hpp), the function sr_validate_line runs: SWAR masks over
//                          the four dwords settle the name and the tags; only the bytes from the first ':' to the
//                          end of the '@' field go through the byte machine, out of the registers with static
//                          shifts. A line whose reason is known stops loading.
//                          It writes the reason (u8) per record, the tile's {kept, dropped, dropped bytes,
//                          subject} and the hits: per-workgroup u64 LDS cells; a wave first settles runs of one
//                          reason (up to kValidPeel times the first undecided lane's reason is matched against the
//                          wave, and that lane adds for all of them), so a wave of OK lines costs one pair of LDS
//                          atomics per tile; the non-zero cells go to the global cells once per workgroup.
//   validate_scan_kernel   one workgroup per batch turns the tiles' kept counts into exclusive bases and writes the
//                          batch's four counts (rules_scan_kernel's code over this stage's arguments).
//   validate_emit_kernel   reads the reasons, ranks the kept records in the workgroup and writes them, and their
//                          hashes when given, in input order.
//   validate_out_kernel    the host-memory path only: the counts, and for the trace the input records, into the
//                          slot's page-locked memory.
// Vector stores only; no scratch memory.
#pragma once

#include <hip/hip_runtime.h>

#include "route_kernel.hpp"
#include "rules_kernel.hpp"
#include "stats_kernel.hpp"
#include "validate_host.hpp"

namespace srk {

constexpr int kValidBlock = 256;             // threads per workgroup: four waves
constexpr int kValidTile = kValidBlock;      // records per tile, one per thread
constexpr int kValidWaves = kValidBlock / 64;
constexpr int kValidGroups = 2048;           // most workgroups of a launch (eight per CU)
constexpr int kValidMaxBatches = 32;
constexpr int kValidPeel = 2;                // rounds of settling equal reasons in a wave
constexpr int kValidScanBlock = 1024;        // validate_scan_kernel: tiles per step
constexpr uint32_t kValidGridLineBytes = 16; // the grid's bound: no more than one record per this many bytes
constexpr uint32_t kValidHitCells = 2u * SR_VALID_REASONS;   // {lines, bytes} per reason

struct ValidateBatchArg {
    const uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;     // with hashes_out, or both null
    sr_record *out;
    uint64_t *hashes_out;
    uint8_t *reason;            // the caller's d_reason, or the stage's scratch
    uint64_t *counts;
    uint32_t nbytes, max_records;
};

struct ValidateArgs {
    ValidateBatchArg b[kValidMaxBatches];
    unsigned long long *hits;   // kValidHitCells
    uint4 *tiles;               // per tile {kept, dropped, dropped bytes, subject}; after the scan x = kept base
    uint32_t nb, nds;
    uint32_t drop_mask, accept_types;
};

// The launch's real tiles, as rules_tiles numbers them.
__device__ __forceinline__ uint32_t validate_tiles(const ValidateArgs &a, uint32_t *s_n, uint32_t *s_t0) {
    if (threadIdx.x < kValidMaxBatches) {
        uint32_t n = 0;
        if (threadIdx.x < a.nb) {
            const ValidateBatchArg &b = a.b[threadIdx.x];
            const uint64_t nrec = *b.n_records;
            n = (uint32_t)(nrec < b.max_records ? nrec : b.max_records);
        }
        s_n[threadIdx.x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int j = 0; j < kValidMaxBatches; ++j) {
            s_t0[j] = t;
            t += (s_n[j] + (uint32_t)kValidTile - 1u) / (uint32_t)kValidTile;
        }
        s_t0[kValidMaxBatches] = t;
    }
    __syncthreads();
    return s_t0[kValidMaxBatches];
}

// The reason of the subject record (o, len), len >= 1. Step s is bytes [16 s, 16 s + 16) of the line: blocks s and,
// for a line that is not 16-byte aligned, s + 1 of the line's blocks; block k is requested only when a byte of the
// line lies in it.
__device__ __forceinline__ uint32_t validate_line_dev(const uint8_t *bytes, uint32_t nbytes, uint32_t o, uint32_t len,
                                                      uint32_t accept) {
    const uint32_t sh = (uint32_t)(((uintptr_t)bytes + o) & 15u);
    const int64_t blk = (int64_t)o - (int64_t)sh;   // the line's first block, relative to the batch
    const uint32_t nblk = (sh + len + 15u) >> 4;    // the blocks that hold a byte of the line, >= 1
    const uint32_t steps = (len + 15u) >> 4;        // <= nblk
    uint4 cur = make_uint4(0u, 0u, 0u, 0u), nxt = cur;
    ValidateState st;
    validate_begin(st);
    // Turn t requests block t and judges step t - 2 from blocks t - 2 and t - 1, which turns before it requested:
    // one load site, and a load is two turns old when its bytes are first looked at.
#pragma unroll 1
    for (uint32_t t = 0; t < steps + 2u; ++t) {
        uint4 ld = make_uint4(0u, 0u, 0u, 0u);
        if (t < nblk) ld = rules_block(bytes, blk + 16 * (int64_t)t, nbytes);
        if (t >= 2u) {
            const uint4 c = rules_shift(cur, nxt, sh);
            const uint32_t left = len - 16u * (t - 2u);
            validate_step(st, c.x, c.y, c.z, c.w, 16u * (t - 2u), left < 16u ? left : 16u, left <= 16u, accept);
            if (st.phase >= kVpDone) break;
        }
        cur = nxt;
        nxt = ld;
    }
    return validate_finish(st, accept);
}

// Six workgroups per CU are promised to the compiler, not eight: under eight it caps the scalar registers at 80 and
// spills six of them into vector lanes. With six it takes 96 scalar and 64 vector registers and spills nothing,
// which by the vector registers still lets eight workgroups be resident.
__global__ __launch_bounds__(kValidBlock, 6) void validate_check_kernel(ValidateArgs a) {
    __shared__ unsigned long long s_hits[kValidHitCells];
    __shared__ uint32_t s_n[kValidMaxBatches], s_t0[kValidMaxBatches + 1];
    __shared__ uint32_t s_wave[kValidWaves][4];
    const uint32_t ntiles = validate_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    if (threadIdx.x < kValidHitCells) s_hits[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;   // tile < ntiles = s_t0[32]: j stays below the batch count
        const ValidateBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kValidTile + threadIdx.x;
        uint32_t reason = SR_VALID_NOT_SUBJECT, len = 0;
        if (i < n) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(b.recs + i);   // sr_record is 4-byte aligned
            const uint32_t o = w[0], ly = w[1];
            len = ly & 0xFFFFu;
            if ((ly >> 16) < a.nds && len >= 1u && (uint64_t)o + len <= b.nbytes)
                reason = validate_line_dev(b.bytes, b.nbytes, o, len, a.accept_types);
            b.reason[i] = (uint8_t)reason;
        }
        const bool subject = reason != SR_VALID_NOT_SUBJECT;
        const bool dropped = subject && ((a.drop_mask >> reason) & 1u);
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
        // hits: runs of one reason are settled in the wave, the first undecided lane adds for all of them
        bool act = subject;
        uint32_t cnt = 1u, bsum = len;
        for (int round = 0; round < kValidPeel && rem; ++round) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t lr = __shfl(reason, lead);
            const bool mine = subject && ((rem >> lane) & 1ull) && reason == lr;
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
        if (act) {   // subject: reason < SR_VALID_REASONS
            atomicAdd(&s_hits[2u * reason], (unsigned long long)cnt);
            atomicAdd(&s_hits[2u * reason + 1u], (unsigned long long)bsum);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = 0, d = 0, m = 0, s = 0;
            for (int w = 0; w < kValidWaves; ++w) {
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
    if (threadIdx.x < kValidHitCells) {
        const unsigned long long v = s_hits[threadIdx.x];
        if (v) atomicAdd(&a.hits[threadIdx.x], v);
    }
}

// One workgroup per batch: its tiles' kept counts into exclusive bases, and the batch's counts. A tile's dropped
// bytes stay below 2^24 (256 lines of at most 65535), so they are summed in 64 bits.
__global__ __launch_bounds__(kValidScanBlock) void validate_scan_kernel(ValidateArgs a) {
    __shared__ uint32_t s_n[kValidMaxBatches], s_t0[kValidMaxBatches + 1];
    __shared__ uint32_t s_wave[kValidScanBlock / 64][3];
    __shared__ unsigned long long s_bytes[kValidScanBlock / 64];
    (void)validate_tiles(a, s_n, s_t0);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x;   // < nb
    const uint32_t t0 = s_t0[j], nt = s_t0[j + 1] - t0;
    uint64_t run_k = 0, run_d = 0, run_b = 0, run_s = 0;
    for (uint32_t g0 = 0; g0 < nt; g0 += (uint32_t)kValidScanBlock) {
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
        for (uint32_t w = 0; w < (uint32_t)kValidScanBlock / 64u; ++w) {
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

__global__ __launch_bounds__(kValidBlock) void validate_emit_kernel(ValidateArgs a) {
    __shared__ uint32_t s_n[kValidMaxBatches], s_t0[kValidMaxBatches + 1];
    __shared__ uint32_t s_wave[kValidWaves];
    const uint32_t ntiles = validate_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;
        const ValidateBatchArg &b = a.b[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kValidTile + threadIdx.x;
        bool kept = false;
        uint2 w = make_uint2(0u, 0u);
        if (i < s_n[j]) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(b.recs + i);
            w = make_uint2(r[0], r[1]);
            const uint32_t reason = b.reason[i];
            kept = reason >= SR_VALID_REASONS || !((a.drop_mask >> reason) & 1u);
        }
        const uint64_t km = __ballot(kept);
        const uint32_t rank = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
        if (lane == 0u) s_wave[wave] = (uint32_t)__builtin_popcountll(km);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t q = 0; q < (uint32_t)kValidWaves; ++q) before += q < wave ? s_wave[q] : 0u;
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

// The host-memory path (sr_set_validate): the stage's four counts and the batch's input record count into the
// slot's page-locked memory (device-mapped); with sr_set_trace, and when no later stage's out kernel does it,
// also the input-order records and the hashes, which pack_out_kernel would cut at the kept count.
struct ValidateOut {
    const uint64_t *counts;      // the stage's four
    const uint64_t *n_records;   // the route launch's count
    uint64_t rec_cap;
    uint64_t *h_counts;          // device-mapped: 4 counts, then the input's record count
    const sr_record *recs;       // sr_set_trace (else null)
    const uint64_t *hashes;
    sr_record *h_recs;
    uint64_t *h_hashes;
};

__global__ __launch_bounds__(kValidBlock) void validate_out_kernel(ValidateOut o) {
    const uint64_t tid = (uint64_t)blockIdx.x * kValidBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kValidBlock;
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

// The stage's device state on the host side (sr_validate_open, sr_validate).
struct ValidateStage {
    int open;
    sr_validate_config cfg;
    unsigned long long *d_hits;   // kValidHitCells
    uint8_t *d_reason;            // per record of a call, for batches without d_reason
    size_t reason_cap;
    uint4 *d_tiles;               // per tile of a call
    size_t tiles_cap;
};

}  // namespace srk
