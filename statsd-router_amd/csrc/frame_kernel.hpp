// frame_kernel.hpp — datagrams framed on the device, straight from their recvmmsg slots.
//
// udp_read_cb caps a datagram at 4095 bytes and appends '\n' unless its last byte is one
// (sr-main.c:163-173); the batch the route kernel reads is those framed datagrams back to back
// (sr_frame_datagrams). Here the input is what recvmmsg leaves: datagram j in bytes
// [j * stride, j * stride + lens[j]) of `slots`, and the output is that same batch plus ends[j], the framed
// end offset after datagram j.
//
// Three launches; no workgroup waits for another (no look-back, no spin, no returning atomic):
//   frame_lens_kernel    one datagram per thread: the capped length, one load of the last kept byte for the
//                        framed length, a DPP wave scan and an LDS scan over the workgroup's 16 waves:
//                        workgroup-local inclusive ends and one sum per workgroup (kFrameSpan datagrams);
//   frame_scan_kernel    one wave turns the (at most kFrameMaxGroups) sums into exclusive bases and writes
//                        the total;
//   frame_gather_kernel  a wave owns kFrameRun consecutive datagrams, i.e. one contiguous destination range.
//                        Every lane owns aligned 16-byte destination pieces of it (payload_kernel.hpp's
//                        discipline): a piece inside one datagram is one unaligned dwordx4 buffer load and
//                        one aligned dwordx4 store; a piece that spans datagrams (they can be 1 byte long,
//                        so it may span 16 of them) is composed from one masked fetch per datagram; the
//                        pieces a run shares with its neighbours are byte stores of the run's own bytes, so
//                        no two waves write the same byte and nothing is read back. An appended '\n' is
//                        written by the lane that owns its piece.
// Source addresses are 64-bit: the buffer resource is rebased to the run's first slot, and offsets inside a
// run (kFrameRun * stride) stay below 2^31 (sr_frame_slots bounds the stride).
#pragma once

#include "payload_kernel.hpp"

namespace srk {

constexpr uint32_t kFrameSpan = 1024;        // datagrams per workgroup of frame_lens_kernel
constexpr uint32_t kFrameMaxGroups = 64;     // SR_MAX_SLOTS / kFrameSpan: one wave scans the sums
constexpr int kFrameBlock = 256;             // gather: four waves, each on a run of its own
constexpr int kFrameWaves = kFrameBlock / 64;
constexpr int kFrameRun = 16;                // consecutive datagrams a wave gathers
constexpr uint64_t kFrameMaxStride = (1ull << 31) / kFrameRun;   // offsets inside a run fit 31 bits

struct FrameArgs {
    const uint8_t *slots;
    uint64_t stride;
    const uint16_t *lens;
    uint8_t *bytes;
    uint64_t cap;
    uint32_t *ends;      // null or [count]
    uint64_t *total;
    uint32_t *loc;       // [count] workgroup-local inclusive ends (scratch)
    uint32_t *sums;      // [kFrameMaxGroups] workgroup sums, then their exclusive bases (scratch)
    uint32_t count;
};

__device__ __forceinline__ uint32_t frame_cap_len(uint32_t len) { return min(len, (uint32_t)SR_MAX_DATAGRAM); }

__global__ __launch_bounds__(1024) void frame_lens_kernel(FrameArgs a) {
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t j = blockIdx.x * kFrameSpan + tid;
    uint32_t v = 0;
    if (j < a.count) {
        const uint32_t n = frame_cap_len(a.lens[j]);
        if (n) v = n + (a.slots[(uint64_t)j * a.stride + (n - 1u)] != (uint8_t)'\n' ? 1u : 0u);
    }
    const uint32_t incl = wave_incl_add32(v);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 16u; ++w) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    if (j < a.count) a.loc[j] = before + incl;
    if (tid == 0) a.sums[blockIdx.x] = all;
}

__global__ __launch_bounds__(64) void frame_scan_kernel(FrameArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t groups = (a.count + kFrameSpan - 1u) / kFrameSpan;   // <= 64
    const uint32_t s = lane < groups ? a.sums[lane] : 0u;
    const uint32_t incl = wave_incl_add32(s);
    if (lane < groups) a.sums[lane] = incl - s;
    if (lane == 63u) *a.total = incl;
}

// 16 bytes at byte `at` of the run's buffer; bytes outside [lo, hi) (one datagram's kept bytes) read as 0.
__device__ __forceinline__ uint4 frame_fetch16(__amdgpu_buffer_rsrc_t rsrc, int64_t at, int64_t lo, int64_t hi) {
    if (at >= lo && at + 16 <= hi) return pay_fetch16(rsrc, at, (uint32_t)hi);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t x = at + i;
        if (x >= lo && x < hi)
            w[i >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rsrc, (uint32_t)x, 0, 0) << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kFrameBlock) void frame_gather_kernel(FrameArgs a) {
    __shared__ uint32_t s_start[kFrameWaves][kFrameRun + 1];
    __shared__ uint32_t s_len[kFrameWaves][kFrameRun];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t j0 = (blockIdx.x * (uint32_t)kFrameWaves + (uint32_t)wave) * (uint32_t)kFrameRun;
    if (j0 >= a.count) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const int nrun = (int)min((uint32_t)kFrameRun, a.count - j0);
    uint32_t *const lstart = s_start[wave], *const llen = s_len[wave];
    // the run's first framed byte: the end of the datagram before it
    const uint32_t S = j0 ? a.loc[j0 - 1u] + a.sums[(j0 - 1u) / kFrameSpan] : 0u;
    if (lane < nrun) {
        const uint32_t j = j0 + (uint32_t)lane;
        const uint32_t e = a.loc[j] + a.sums[j / kFrameSpan];
        lstart[lane + 1] = e - S;
        llen[lane] = frame_cap_len(a.lens[j]);
        if (a.ends) a.ends[j] = e;
    }
    if (lane == 0) lstart[0] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // LDS hand-off between the lanes of one wave
    __builtin_amdgcn_wave_barrier();
    // bytes [S, S + w1) of the batch are this run's, cut at the capacity
    const int w1 = S >= a.cap ? 0 : (int)min((uint64_t)lstart[nrun], a.cap - S);
    if (w1 <= 0) return;
    uint8_t *const dst = a.bytes + S;
    const int mis = (int)((uintptr_t)dst & 15u);
    uint8_t *const base = dst - mis;            // 16-byte aligned; piece c covers base + 16 c
    const int x1 = mis + w1;                    // the written range in piece coordinates: [mis, x1)
    const int npieces = (x1 + 15) >> 4;
    const int64_t stride = (int64_t)a.stride;
    const uint32_t range = (uint32_t)((uint64_t)(nrun - 1) * a.stride + SR_MAX_DATAGRAM);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.slots + (uint64_t)j0 * a.stride), (short)0, (int)range, 0x00020000);
    for (int c = lane; c < npieces; c += 64) {
        const int A = 16 * c;
        const int s0 = max(A, mis), s1 = min(A + 16, x1);       // this piece's bytes of the run
        const int q0 = s0 - mis, q1 = s1 - mis, qa = A - mis;   // as run positions (qa may be < 0)
        // the last datagram that starts at or before q0 (the one that holds q0: empty ones before it share
        // its start)
        int lo = 0, hi = nrun - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int)lstart[mid] <= q0) lo = mid;
            else hi = mid - 1;
        }
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
        for (int i = lo; i < nrun; ++i) {
            const int ls = (int)lstart[i], le = (int)lstart[i + 1];
            if (ls >= q1) break;
            if (le == ls) continue;
            const int n = (int)llen[i];
            const int64_t slot0 = (int64_t)i * stride;
            uint4 v = frame_fetch16(rsrc, slot0 + (qa - ls), slot0, slot0 + n);
            if (le - ls > n) {   // the appended '\n' is the datagram's last framed byte
                const int p = le - 1 - qa;
                v.x |= pay_mask(p, p + 1, 0) & 0x0A0A0A0Au;
                v.y |= pay_mask(p, p + 1, 1) & 0x0A0A0A0Au;
                v.z |= pay_mask(p, p + 1, 2) & 0x0A0A0A0Au;
                v.w |= pay_mask(p, p + 1, 3) & 0x0A0A0A0Au;
            }
            if (ls <= qa && le >= qa + 16) {   // the datagram covers the whole piece (most pieces)
                acc = v;
                break;
            }
            pay_or(acc, v, max(ls, q0) - qa, min(le, q1) - qa);
        }
        uint8_t *const o = base + A;
        if (s1 - s0 == 16) {
            *reinterpret_cast<uint4 *>(o) = acc;
        } else {   // a piece shared with a neighbouring run (or an end of the batch): this run's bytes only
            const uint32_t w[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i >= s0 - A && i < s1 - A) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace srk
