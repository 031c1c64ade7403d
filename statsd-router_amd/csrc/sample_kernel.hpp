// sample_kernel.hpp — sample rates on the device (include/sr_route.h).
//
// Behind a route launch the input-order records, their 64-bit name hashes and the bytes are on the device. Five
// launches count the sampleable lines per slot, thin the slots over the limit and write the kept lines with the
// rate inserted. All ordering is by kernel boundaries: no workgroup waits for another, no atomic returns a value
// that anything depends on. The table holds counts only: no owner, no compare of names (a shared slot is a shared
// budget, and every kept line still carries the rate by which it was thinned).
//
//   sample_clear_kernel  the launch's slot counts (u32, `slots` per batch) to zero, 16 bytes per store.
//   sample_count_kernel  one record per thread, tiles of kSampleTile records numbered by the device's record
//                        counts (rules_kernel.hpp's scheme). A thread takes its line's content in 16-byte steps:
//                        aligned uint4 loads (rules_block), two neighbouring blocks put together with v_alignbyte
//                        (rules_shift), the block two ahead requested before the current step is looked at. A step
//                        is judged by sample_step_bytes (sample_host.hpp), the function sr_sample_parse runs: SWAR
//                        masks for ':' and '|'. It stops at the step that holds e; behind the type only the byte
//                        at e + 1 is looked at. {ins, type, sampleable} goes to the per-record scratch word. The
//                        slot's count is a 32-bit atomic add without return; before it a wave settles runs of one
//                        slot (up to kSamplePeel times the first undecided lane's slot is matched against the
//                        wave, and that lane adds for all of them), so a wave of one hot name costs one atomic.
//   sample_sum_kernel    per tile, from the final counts: the step, the keep verdict (both into the scratch word),
//                        the tile's {records kept, lines rewritten, rewritten bytes, records dropped}, and the hits
//                        {seen, kept} per step: the wave settles each step it holds in one pair of LDS adds, and
//                        the non-zero cells go to the global cells once per workgroup. (Its own kernel, not fused
//                        into the scan: the scan is one workgroup per batch.)
//   sample_scan_kernel   one workgroup of 1024 per batch turns the tiles' kept records and rewritten bytes into
//                        exclusive bases (the bytes' in 64 bits) and writes the batch's four counts.
//   sample_emit_kernel   records and hashes out in input order, d_step, and the rewritten text. A rewritten line is
//                        copied by its whole wave: the wave walks the ballot of its lanes' rewritten lines, takes
//                        (o, L, ins, step, destination) by lane reads and copies 64 bytes per turn, lane k the
//                        line's byte 64 t + k to its place in front of or behind the insert; bytes, because the
//                        insert of 5..8 bytes moves the source against the destination by any phase. The insert
//                        is written by lane 0. Every byte store checks append_cap against a 64-bit position.
//   sample_out_kernel    the host-memory path only: the text, the counts and, for the trace, the input records into
//                        the slot's page-locked memory.
// Vector stores only; no scratch memory.
#pragma once

#include <hip/hip_runtime.h>

#include "route_kernel.hpp"
#include "rules_kernel.hpp"
#include "stats_kernel.hpp"
#include "sample_host.hpp"

namespace srk {

constexpr int kSampleBlock = 256;             // threads per workgroup: four waves
constexpr int kSampleTile = kSampleBlock;     // records per tile, one per thread
constexpr int kSampleWaves = kSampleBlock / 64;
constexpr int kSampleGroups = 2048;           // most workgroups of a launch (eight per CU)
constexpr int kSampleMaxBatches = 32;
constexpr int kSamplePeel = 2;                // rounds of settling equal slots in a wave
constexpr int kSampleScanBlock = 1024;        // sample_scan_kernel: tiles per step
constexpr uint32_t kSampleGridLineBytes = 16; // the grid's bound: no more than one record per this many bytes
constexpr uint32_t kSampleHitCells = 2u * SR_SAMPLE_STEPS;   // {seen, kept} per step

// the per-record scratch word
constexpr uint32_t kSwInsMask = 0x7FFu;       // ins <= 1440
constexpr uint32_t kSwTypeShift = 16u;        // the type's bit, 6 bits
constexpr uint32_t kSwStepShift = 24u;        // the step, 4 bits (sample_sum_kernel)
constexpr uint32_t kSwDropped = 1u << 30;     // (sample_sum_kernel)
constexpr uint32_t kSwSampleable = 1u << 31;

struct SampleBatchArg {
    uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;
    sr_record *out;
    uint64_t *hashes_out;       // or null
    uint8_t *step;              // the caller's d_step, or null
    uint64_t *counts;
    uint32_t *scratch;          // one word per record
    uint32_t *table;            // the batch's `slots` counts
    uint64_t append_cap;
    uint64_t seed;              // cfg.seed + seed_add
    uint32_t nbytes, max_records;
};

struct SampleArgs {
    SampleBatchArg b[kSampleMaxBatches];
    unsigned long long *hits;   // kSampleHitCells
    uint4 *tiles;               // per tile {kept, rewritten, bytes, dropped}; after the scan {kept base, byte base lo, hi}
    uint32_t nb, nds;
    uint32_t slots, limit, types;
};

// The launch's real tiles, as rules_tiles numbers them.
__device__ __forceinline__ uint32_t sample_tiles(const SampleArgs &a, uint32_t *s_n, uint32_t *s_t0) {
    if (threadIdx.x < kSampleMaxBatches) {
        uint32_t n = 0;
        if (threadIdx.x < a.nb) {
            const SampleBatchArg &b = a.b[threadIdx.x];
            const uint64_t nrec = *b.n_records;
            n = (uint32_t)(nrec < b.max_records ? nrec : b.max_records);
        }
        s_n[threadIdx.x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int j = 0; j < kSampleMaxBatches; ++j) {
            s_t0[j] = t;
            t += (s_n[j] + (uint32_t)kSampleTile - 1u) / (uint32_t)kSampleTile;
        }
        s_t0[kSampleMaxBatches] = t;
    }
    __syncthreads();
    return s_t0[kSampleMaxBatches];
}

// The table is a.b[0].table .. + nb * slots words, back to back (sr_sample lays the batches' tables out so).
__global__ __launch_bounds__(kSampleBlock) void sample_clear_kernel(SampleArgs a) {
    uint4 *const t = reinterpret_cast<uint4 *>(a.b[0].table);
    const uint64_t n = (uint64_t)a.nb * a.slots / 4u;   // slots is a multiple of 16
    for (uint64_t i = (uint64_t)blockIdx.x * kSampleBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSampleBlock)
        t[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The scratch word of the subject record (o, len): whether it is sampleable, and then ins and the type's bit.
// Step s is bytes [16 s, 16 s + 16) of the content; block k is requested only when a byte of the content lies in it.
__device__ __forceinline__ uint32_t sample_line_dev(const uint8_t *bytes, uint32_t nbytes, uint32_t o, uint32_t len,
                                                    uint32_t types) {
    if (len < 6u || len > SR_SAMPLE_LINE_MAX || bytes[o + len - 1u] != 0x0Au) return 0u;
    const uint32_t clen = len - 1u;                 // >= 5
    const uint32_t sh = (uint32_t)(((uintptr_t)bytes + o) & 15u);
    const int64_t blk = (int64_t)o - (int64_t)sh;   // the line's first block, relative to the batch
    const uint32_t nblk = (sh + clen + 15u) >> 4;   // the blocks that hold a byte of the content, >= 1
    const uint32_t steps = (clen + 15u) >> 4;       // <= nblk
    uint4 cur = make_uint4(0u, 0u, 0u, 0u), nxt = cur;
    SampleState st;
    sample_begin(st);
    // Turn t requests block t and judges step t - 2 from blocks t - 2 and t - 1 (validate_line_dev's loop).
#pragma unroll 1
    for (uint32_t t = 0; t < steps + 2u; ++t) {
        uint4 ld = make_uint4(0u, 0u, 0u, 0u);
        if (t < nblk) ld = rules_block(bytes, blk + 16 * (int64_t)t, nbytes);
        if (t >= 2u) {
            const uint4 c = rules_shift(cur, nxt, sh);
            const uint32_t left = clen - 16u * (t - 2u);
            sample_step_bytes(st, c.x, c.y, c.z, c.w, 16u * (t - 2u), left < 16u ? left : 16u, types);
            if (st.phase >= kSpOk) break;
        }
        cur = nxt;
        nxt = ld;
    }
    if (!sample_finish(st, clen, types)) return 0u;
    return kSwSampleable | st.bit << kSwTypeShift | st.ins;
}

__global__ __launch_bounds__(kSampleBlock) void sample_count_kernel(SampleArgs a) {
    __shared__ uint32_t s_n[kSampleMaxBatches], s_t0[kSampleMaxBatches + 1];
    const uint32_t ntiles = sample_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;   // tile < ntiles = s_t0[32]: j stays below the batch count
        const SampleBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kSampleTile + threadIdx.x;
        uint32_t word = 0u, slot = 0u;
        if (i < n) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(b.recs + i);   // sr_record is 4-byte aligned
            const uint32_t o = w[0], ly = w[1], len = ly & 0xFFFFu;
            if ((ly >> 16) < a.nds && len >= 1u && (uint64_t)o + len <= b.nbytes)
                word = sample_line_dev(b.bytes, b.nbytes, o, len, a.types);
            b.scratch[i] = word;
            if (word) slot = (uint32_t)stats_fmix64(b.hashes[i]) & smask;
        }
        // runs of one slot are settled in the wave: the first undecided lane adds for all of them
        const bool samp = word != 0u;
        uint64_t rem = __ballot(samp);
        bool act = samp;
        uint32_t cnt = 1u;
        for (int round = 0; round < kSamplePeel && rem; ++round) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t ls = __shfl(slot, lead);
            const bool mine = samp && ((rem >> lane) & 1ull) && slot == ls;
            const uint64_t same = __ballot(mine);
            rem &= ~same;
            if (mine) {
                act = lane == (uint32_t)lead;
                cnt = (uint32_t)__builtin_popcountll(same);
            }
        }
        if (act) atomicAdd(&b.table[slot], cnt);   // slot < slots; the result is not used
    }
}

__global__ __launch_bounds__(kSampleBlock) void sample_sum_kernel(SampleArgs a) {
    __shared__ unsigned long long s_hits[kSampleHitCells];
    __shared__ uint32_t s_n[kSampleMaxBatches], s_t0[kSampleMaxBatches + 1];
    __shared__ uint32_t s_wave[kSampleWaves][4];
    const uint32_t ntiles = sample_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    if (threadIdx.x < kSampleHitCells) s_hits[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t smask = a.slots - 1u;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;
        const SampleBatchArg &b = a.b[j];
        const uint32_t n = s_n[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kSampleTile + threadIdx.x;
        bool samp = false, keep = true;
        uint32_t step = 0u, newlen = 0u;
        if (i < n) {
            const uint32_t word = b.scratch[i];
            if (word & kSwSampleable) {
                samp = true;
                const uint64_t h = b.hashes[i];
                step = sample_step(a.limit, (uint64_t)b.table[(uint32_t)stats_fmix64(h) & smask]);
                keep = sample_keep(h, b.seed, (uint64_t)i, step) != 0u;
                if (keep && step) newlen = (reinterpret_cast<const uint32_t *>(b.recs + i)[1] & 0xFFFFu) + sample_insert_len(step);
                b.scratch[i] = word | step << kSwStepShift | (keep ? 0u : kSwDropped);
            }
        }
        const uint64_t km = __ballot(i < n && keep), rm = __ballot(newlen != 0u);
        const uint32_t rbytes = rm ? stats_wave_sum(newlen) : 0u;
        uint64_t rem = __ballot(samp);
        if (lane == 0u) {
            s_wave[wave][0] = (uint32_t)__builtin_popcountll(km);
            s_wave[wave][1] = (uint32_t)__builtin_popcountll(rm);
            s_wave[wave][2] = rbytes;
            s_wave[wave][3] = (uint32_t)__builtin_popcountll(rem & ~km);
        }
        // hits: every step the wave holds is settled by its first lane (at most SR_SAMPLE_STEPS turns, mostly one)
        while (rem) {
            const int lead = __builtin_ctzll(rem);
            const uint32_t ls = __shfl(step, lead);
            const uint64_t same = __ballot(samp && step == ls) & rem;
            rem &= ~same;
            if (lane == (uint32_t)lead) {   // ls < SR_SAMPLE_STEPS
                atomicAdd(&s_hits[2u * ls], (unsigned long long)__builtin_popcountll(same));
                const uint32_t k = (uint32_t)__builtin_popcountll(same & km);
                if (k) atomicAdd(&s_hits[2u * ls + 1u], (unsigned long long)k);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t k = 0, r = 0, m = 0, d = 0;
            for (int w = 0; w < kSampleWaves; ++w) {
                k += s_wave[w][0];
                r += s_wave[w][1];
                m += s_wave[w][2];
                d += s_wave[w][3];
            }
            a.tiles[tile] = make_uint4(k, r, m, d);
        }
        __syncthreads();
    }
    // the workgroup's hits into the context's: the non-zero cells only (the barrier above ordered the LDS adds)
    if (threadIdx.x < kSampleHitCells) {
        const unsigned long long v = s_hits[threadIdx.x];
        if (v) atomicAdd(&a.hits[threadIdx.x], v);
    }
}

// One workgroup per batch: its tiles' kept records and rewritten bytes into exclusive bases, and the batch's counts.
// A tile's rewritten bytes stay below 2^19 (256 lines of at most 1449), 1024 tiles' below 2^29: a turn's scan is in
// 32 bits, the running base in 64.
__global__ __launch_bounds__(kSampleScanBlock) void sample_scan_kernel(SampleArgs a) {
    __shared__ uint32_t s_n[kSampleMaxBatches], s_t0[kSampleMaxBatches + 1];
    __shared__ uint32_t s_wave[kSampleScanBlock / 64][4];
    (void)sample_tiles(a, s_n, s_t0);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x;   // < nb
    const uint32_t t0 = s_t0[j], nt = s_t0[j + 1] - t0;
    uint64_t run_k = 0, run_r = 0, run_b = 0, run_d = 0;
    for (uint32_t g0 = 0; g0 < nt; g0 += (uint32_t)kSampleScanBlock) {
        const uint32_t g = g0 + tid;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (g < nt) e = a.tiles[t0 + g];
        const uint32_t ik = wave_incl_add32(e.x), ib = wave_incl_add32(e.z);
        const uint32_t sr = stats_wave_sum(e.y), sd = stats_wave_sum(e.w);
        if (lane == 63u) {
            s_wave[wave][0] = ik;
            s_wave[wave][1] = sr;
            s_wave[wave][2] = ib;
            s_wave[wave][3] = sd;
        }
        __syncthreads();
        uint32_t before_k = 0, before_b = 0, all_k = 0, all_r = 0, all_b = 0, all_d = 0;
        for (uint32_t w = 0; w < (uint32_t)kSampleScanBlock / 64u; ++w) {
            before_k += w < wave ? s_wave[w][0] : 0u;
            before_b += w < wave ? s_wave[w][2] : 0u;
            all_k += s_wave[w][0];
            all_r += s_wave[w][1];
            all_b += s_wave[w][2];
            all_d += s_wave[w][3];
        }
        if (g < nt) {
            const uint64_t bb = run_b + before_b + (ib - e.z);
            a.tiles[t0 + g] = make_uint4((uint32_t)(run_k + before_k + (ik - e.x)), (uint32_t)bb, (uint32_t)(bb >> 32), 0u);
        }
        run_k += all_k;
        run_r += all_r;
        run_b += all_b;
        run_d += all_d;
        __syncthreads();
    }
    if (tid == 0) {
        uint64_t *const c = a.b[j].counts;
        c[0] = run_k;
        c[1] = run_d;
        c[2] = run_r;
        c[3] = run_b;
    }
}

__global__ __launch_bounds__(kSampleBlock) void sample_emit_kernel(SampleArgs a) {
    __shared__ uint32_t s_n[kSampleMaxBatches], s_t0[kSampleMaxBatches + 1];
    __shared__ uint32_t s_wave[kSampleWaves][2];
    const uint32_t ntiles = sample_tiles(a, s_n, s_t0);
    if (blockIdx.x >= ntiles) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int j = 0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        while (s_t0[j + 1] <= tile) ++j;
        const SampleBatchArg &b = a.b[j];
        const uint32_t i = (tile - s_t0[j]) * (uint32_t)kSampleTile + threadIdx.x;
        bool kept = false;
        uint2 w = make_uint2(0u, 0u);
        uint32_t word = 0u, step = 0u, newlen = 0u;
        if (i < s_n[j]) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(b.recs + i);
            w = make_uint2(r[0], r[1]);
            word = b.scratch[i];
            kept = !(word & kSwDropped);
            if (word & kSwSampleable) step = (word >> kSwStepShift) & 15u;
            if (kept && step) newlen = (w.y & 0xFFFFu) + sample_insert_len(step);
            if (b.step)
                b.step[i] = (uint8_t)(!(word & kSwSampleable) ? SR_SAMPLE_NOT_SAMPLEABLE : step | (kept ? 0u : SR_SAMPLE_DROPPED));
        }
        const uint64_t km = __ballot(kept);
        const uint32_t rank = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
        const uint32_t ib = wave_incl_add32(newlen);   // < 2^17 in a wave
        if (lane == 63u) {
            s_wave[wave][0] = (uint32_t)__builtin_popcountll(km);
            s_wave[wave][1] = ib;
        }
        __syncthreads();
        uint32_t before = 0, before_b = 0;
        for (uint32_t q = 0; q < (uint32_t)kSampleWaves; ++q) {
            before += q < wave ? s_wave[q][0] : 0u;
            before_b += q < wave ? s_wave[q][1] : 0u;
        }
        const uint4 t = a.tiles[tile];
        const uint64_t dst = ((uint64_t)t.z << 32 | t.y) + before_b + (ib - newlen);   // this lane's text, if it has one
        if (kept) {   // kept ranks stay below the batch's records, so below max_records
            const uint32_t at = t.x + before + rank;
            uint32_t *const o = reinterpret_cast<uint32_t *>(b.out + at);
            o[0] = newlen ? b.nbytes + (uint32_t)dst : w.x;
            o[1] = newlen ? (w.y & 0xFFFF0000u) | newlen : w.y;
            if (b.hashes_out) b.hashes_out[at] = b.hashes[i];
        }
        // the rewritten lines of the wave, one after the other, each copied by all 64 lanes
        uint64_t todo = __ballot(newlen != 0u);
        uint8_t *const text = b.bytes + b.nbytes;
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t lo = __shfl(w.x, src), ll = __shfl(w.y, src) & 0xFFFFu;   // o + L <= nbytes: subject
            const uint32_t lins = __shfl(word, src) & kSwInsMask, lstep = __shfl(step, src);
            const uint64_t ld = stats_shfl64(dst, src);
            uint32_t xl = 0u;
            const uint64_t ins_text = sample_insert(lstep, &xl);
            const uint8_t *const from = b.bytes + lo;
            for (uint32_t k = lane; k < ll; k += 64u) {
                const uint64_t at = ld + (k < lins ? k : k + xl);
                const uint8_t v = from[k];
                if (at < b.append_cap) text[at] = v;
            }
            if (lane == 0u) {
                for (uint32_t k = 0; k < xl; ++k) {
                    const uint64_t at = ld + lins + k;
                    if (at < b.append_cap) text[at] = (uint8_t)(ins_text >> (8u * k));
                }
            }
        }
        __syncthreads();
    }
}

// The host-memory path (sr_set_sample): the rewritten text (by the device's count), the stage's four counts and the
// batch's input record count into the slot's page-locked memory (device-mapped); with sr_set_trace, and when no
// other stage's out kernel does it, also the input-order records and the hashes, which pack_out_kernel would cut
// at the kept count. The text's address has the alignment of the batch's end, so it is read byte by byte and
// written 16 bytes at a time (coalesce_out_kernel's copy).
struct SampleOut {
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

__global__ __launch_bounds__(kSampleBlock) void sample_out_kernel(SampleOut o) {
    const uint64_t tid = (uint64_t)blockIdx.x * kSampleBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kSampleBlock;
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

// The stage's device state on the host side (sr_sample_open, sr_sample).
struct SampleStage {
    int open;
    sr_sample_config cfg;
    uint32_t slots;
    uint32_t *d_table;            // kSampleMaxBatches * slots
    unsigned long long *d_hits;   // kSampleHitCells
    uint32_t *d_scratch;          // per record of a call
    size_t scratch_cap;
    uint4 *d_tiles;               // per tile of a call
    size_t tiles_cap;
};

}  // namespace srk
