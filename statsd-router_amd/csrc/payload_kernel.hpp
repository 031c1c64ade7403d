// payload_kernel.hpp — the packets' bytes in wire format, gathered on the device.
//
// sr_pack_packets writes, per batch, the sorted records and one 16-byte sr_packet descriptor per
// packet (mtu_kernel.hpp). These kernels turn the descriptors into what ds_flush_cb sends
// (sr-main.c:21-46): per descriptor the `carry` bytes pending before the batch followed by its
// `nlines` lines, laid end to end with no padding, the packets back to back in one arena.
//   offsets : off[i] = exclusive prefix of carry + length over the batch's descriptors, off[n] = total;
//   payload : bytes [off[i], off[i+1]) = pend_in[shard][:carry] + lines (pend_in null: the carry's
//             room is left unwritten, for a host that holds the pending bytes itself);
//   pend_out: slot s (SR_PENDING_STRIDE bytes apart) = the bytes of s's open packet, or, for a
//             downstream without a descriptor, the first fill_out[s] bytes of pend_in[s].
//
// Three launches over all batches of a call:
//   payload_offsets_kernel  one workgroup per batch scans carry + length (DPP wave scans);
//   payload_copy_kernel     a wave takes kPayPerWave consecutive packets, one after another (a wave per
//                           packet spent more time starting than copying: DESIGN.md §5.6). Per packet
//                           the wave scans the line lengths (at most
//                           241 lines of at least 6 bytes fit 1450: four per lane) into LDS, then
//                           every lane owns aligned 16-byte pieces of the destination, finds the
//                           lines that cover its piece in the packet's length prefix and fetches each
//                           with one unaligned dwordx4 buffer load at the matching source byte (byte
//                           loads only where a load would cross the input's ends). A piece that lies
//                           whole inside the packet is one aligned dwordx4 store; the pieces a packet
//                           shares with its neighbours (its first and last) are byte stores of the
//                           packet's own bytes, so no two waves write the same byte and nothing is
//                           read back. The open packet is composed a second time into its pending slot;
//   payload_pending_kernel  one wave per downstream: a binary search over the descriptors (they are
//                           in downstream order) and, where there is none, the pass-through copy.
#pragma once

#include "route_kernel.hpp"

namespace srk {

constexpr int kPayMaxBatches = 32;
constexpr int kPayBlock = 256;                     // four waves, each on packets of its own
constexpr int kPayWaves = kPayBlock / 64;
#ifndef SR_PAY_PER_WAVE
#define SR_PAY_PER_WAVE 8
#endif
constexpr int kPayPerWave = SR_PAY_PER_WAVE;        // consecutive packets a wave gathers, one after another
constexpr uint32_t kPayMaxLines = 256;             // lines of a packet held in LDS (four per lane)
constexpr uint32_t kPendStride = 1456;             // SR_PENDING_STRIDE

struct PayBatchArg {
    const uint8_t *bytes;
    const sr_record *sorted;
    const sr_packet *packets;
    const uint64_t *counts;        // [0] descriptors
    const uint16_t *fill_out;      // [nds] pending bytes after the batch
    const uint8_t *pend_in;        // null: room left for the carry
    uint8_t *pend_out;             // null: none
    uint8_t *payload;
    uint32_t *offsets;             // [max_packets + 1]
    uint64_t *total;
    uint64_t payload_cap;
    uint32_t nbytes;
    uint32_t max_records;
    uint32_t max_packets;
    uint32_t tile0;                // first copy workgroup of the batch in the launch
};

struct PayLaunch {
    uint32_t nb, nds;
    uint32_t tiles, pad;
    PayBatchArg b[kPayMaxBatches];
};
static_assert(sizeof(PayLaunch) < 3584, "kernel argument size");

// descriptors of a batch that were written
__device__ __forceinline__ uint32_t pay_count(const PayBatchArg &b) {
    const uint64_t n = b.counts[0];
    return (uint32_t)(n < b.max_packets ? n : b.max_packets);
}

static_assert(offsetof(sr_packet, length) == 8 && offsetof(sr_packet, carry) == 10, "{length, carry} word");

__global__ __launch_bounds__(1024) void payload_offsets_kernel(PayLaunch L) {
    __shared__ uint32_t s_wave[16];
    const PayBatchArg &b = L.b[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = pay_count(b);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(b.packets);
    uint64_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 1024u) {
        const uint32_t i = i0 + tid;
        uint32_t v = 0;
        if (i < n) {
            const uint32_t lc = words[4 * (size_t)i + 2];
            v = (lc & 0xFFFFu) + (lc >> 16);
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
        if (i < n) b.offsets[i] = (uint32_t)run + before + incl - v;
        run += all;
        __syncthreads();
    }
    if (tid == 0) {
        b.offsets[n] = (uint32_t)run;
        *b.total = run;
    }
}

// 16 bytes at byte `a` of a buffer of n bytes (a may be negative); bytes outside [0, n) read as 0.
// One dwordx4 load unless the piece crosses an end of the buffer.
__device__ __forceinline__ uint4 pay_fetch16(__amdgpu_buffer_rsrc_t rsrc, int64_t a, uint32_t n) {
    if (a >= 0 && a + 16 <= (int64_t)n) return as_uint4(__builtin_amdgcn_raw_buffer_load_b128(rsrc, (uint32_t)a, 0, 0));
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i) {
        const int64_t x = a + i;
        if (x >= 0 && x < (int64_t)n)
            w[i >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rsrc, (uint32_t)x, 0, 0) << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// dword d of the 16-byte mask whose bytes [b0, b1) are set (0 <= b0 <= b1 <= 16)
__device__ __forceinline__ uint32_t pay_mask(int b0, int b1, int d) {
    const int lo = max(b0 - 4 * d, 0), hi = min(b1 - 4 * d, 4);
    if (hi <= lo) return 0u;
    const uint32_t upto_hi = hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u);
    return upto_hi & ~((1u << (8 * lo)) - 1u);   // lo <= 3 here
}

__device__ __forceinline__ void pay_or(uint4 &acc, const uint4 &v, int b0, int b1) {
    acc.x |= v.x & pay_mask(b0, b1, 0);
    acc.y |= v.y & pay_mask(b0, b1, 1);
    acc.z |= v.z & pay_mask(b0, b1, 2);
    acc.w |= v.w & pay_mask(b0, b1, 3);
}

// One packet's view for the composing wave. Positions q count from the packet's first byte (the
// carry first, then the lines): line j covers [lstart[j], lstart[j + 1]), lstart[0] = carry.
struct PayPacket {
    __amdgpu_buffer_rsrc_t rs_in, rs_pend;
    uint32_t nbytes, pend_bytes;
    int64_t pend_at;           // byte of the downstream's slot in pend_in
    int carry, nl, end;        // carried bytes (0: none to fetch), lines, carry + the lines' bytes
    const uint32_t *lstart;    // LDS [nl + 1]
    const uint32_t *lsrc;      // LDS [nl] byte offset of each line in the batch
};

// Bytes [w0, w1) of the packet to dst (dst[q] = the packet's byte q), as aligned 16-byte pieces.
__device__ __forceinline__ void pay_compose(const PayPacket &k, uint8_t *dst, int w0, int w1, int lane) {
    if (w1 <= w0) return;
    const int mis = (int)(((uintptr_t)dst + (uint32_t)w0) & 15u);
    uint8_t *const base = dst + w0 - mis;          // 16-byte aligned; piece c covers base + 16 c
    const int x0 = mis, x1 = mis + (w1 - w0);      // the written range in piece coordinates
    const int qb = w0 - mis;                       // packet position of piece coordinate 0 (may be < 0)
    const int npieces = (x1 + 15) >> 4;
    for (int c = lane; c < npieces; c += 64) {
        const int A = 16 * c;
        const int s0 = max(A, x0), s1 = min(A + 16, x1);   // this piece's bytes of the packet
        const int q0 = qb + s0, q1 = qb + s1, qa = qb + A;
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
        if (q0 < k.carry) {   // the carried bytes
            const uint4 v = pay_fetch16(k.rs_pend, k.pend_at + qa, k.pend_bytes);
            pay_or(acc, v, q0 - qa, min(q1, k.carry) - qa);
        }
        const int ql = max(q0, k.carry);
        if (ql < q1 && k.nl > 0) {
            // the last line that starts at or before ql
            int lo = 0, hi = k.nl - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)k.lstart[mid] <= ql) lo = mid;
                else hi = mid - 1;
            }
            for (int j = lo; j < k.nl; ++j) {
                const int ls = (int)k.lstart[j], le = (int)k.lstart[j + 1];
                if (ls >= q1) break;
                const uint4 v = pay_fetch16(k.rs_in, (int64_t)k.lsrc[j] + (qa - ls), k.nbytes);
                if (ls <= qa && le >= qa + 16) {   // the line covers the whole piece (most pieces of long lines)
                    acc = v;
                    break;
                }
                pay_or(acc, v, max(ls, q0) - qa, min(le, q1) - qa);
            }
        }
        uint8_t *const o = base + A;
        if (s1 - s0 == 16) {
            *reinterpret_cast<uint4 *>(o) = acc;
        } else {   // a piece shared with a neighbour (or an end of the buffer): this packet's bytes only
            const uint32_t w[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i >= s0 - A && i < s1 - A) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
}

__global__ __launch_bounds__(kPayBlock) void payload_copy_kernel(PayLaunch L) {
    __shared__ uint32_t s_start[kPayWaves][kPayMaxLines + 1];
    __shared__ uint32_t s_src[kPayWaves][kPayMaxLines];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the batch of this workgroup (nb <= 32, tile0 ascending)
    uint32_t bi = 0;
    for (uint32_t j = 1; j < L.nb; ++j)
        if (blockIdx.x >= L.b[j].tile0) bi = j;
    const PayBatchArg &b = L.b[bi];
    const uint32_t n = pay_count(b);
    const uint32_t i0 = ((blockIdx.x - b.tile0) * (uint32_t)kPayWaves + (uint32_t)wave) * (uint32_t)kPayPerWave;
    uint32_t *const lstart = s_start[wave], *const lsrc = s_src[wave];
    for (uint32_t i = i0; i < i0 + (uint32_t)kPayPerWave && i < n; ++i) {   // (wave-uniform bounds; no workgroup barrier)
        const sr_packet pk = b.packets[i];
        const uint64_t off = b.offsets[i];
        const uint32_t carry = min((uint32_t)pk.carry, (uint32_t)SR_DOWNSTREAM_BUF_SIZE);
        const uint32_t nl = min((uint32_t)pk.nlines, kPayMaxLines);
        // the packet's lines, four per lane: their lengths scanned, their sources kept
        uint32_t len[4], src[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t j = 4u * (uint32_t)lane + (uint32_t)u;
            const uint64_t r = (uint64_t)pk.first + j;
            len[u] = src[u] = 0;
            if (j < nl && r < b.max_records) {
                const uint2 w = *reinterpret_cast<const uint2 *>(b.sorted + r);
                src[u] = w.x;
                len[u] = w.y & 0xFFFFu;
            }
            sum += len[u];
        }
        uint32_t at = carry + wave_incl_add32(sum) - sum;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t j = 4u * (uint32_t)lane + (uint32_t)u;
            if (j < nl) {
                lstart[j] = at;
                lsrc[j] = src[u];
            }
            at += len[u];
            if (j + 1 == nl || (nl == 0 && j == 0)) lstart[nl] = at;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // LDS hand-off between the lanes of one wave
        __builtin_amdgcn_wave_barrier();
        const uint32_t end = min(lstart[nl], carry + (uint32_t)SR_DOWNSTREAM_BUF_SIZE);

        PayPacket k;
        k.rs_in = __builtin_amdgcn_make_buffer_rsrc((void *)b.bytes, (short)0, (int)b.nbytes, 0x00020000);
        k.nbytes = b.nbytes;
        const uint64_t pend_total = (uint64_t)L.nds * kPendStride;
        k.pend_bytes = b.pend_in ? (uint32_t)pend_total : 0u;
        k.rs_pend = __builtin_amdgcn_make_buffer_rsrc((void *)b.pend_in, (short)0, (int)k.pend_bytes, 0x00020000);
        k.pend_at = (int64_t)pk.shard * kPendStride;
        k.carry = (int)carry;
        k.nl = (int)nl;
        k.end = (int)end;
        k.lstart = lstart;
        k.lsrc = lsrc;
        // into the arena: [off, off + end), without the carry's room when the host holds the pending
        // bytes, cut at the arena's capacity
        {
            const uint64_t cap = b.payload_cap;
            const int w0 = b.pend_in ? 0 : (int)carry;
            const int w1 = off >= cap ? 0 : (int)min((uint64_t)end, cap - off);
            pay_compose(k, b.payload + off, w0, w1, lane);
        }
        // the open packet is the downstream's pending buffer after the batch
        if (pk.open && b.pend_out && pk.shard < L.nds)
            pay_compose(k, b.pend_out + (size_t)pk.shard * kPendStride, 0,
                        (int)min(end, (uint32_t)SR_DOWNSTREAM_BUF_SIZE), lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the prefix is read to the end before the next packet's
        __builtin_amdgcn_wave_barrier();
    }
}

// Downstreams without a descriptor keep their pending bytes: pend_in[s][:fill_out[s]] -> pend_out[s]
// (fill_out 0: probed dead, or nothing pending). One wave per downstream.
__global__ __launch_bounds__(kPayBlock) void payload_pending_kernel(PayLaunch L) {
    const PayBatchArg &b = L.b[blockIdx.y];
    if (!b.pend_out || !b.pend_in) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * (uint32_t)kPayWaves + (threadIdx.x >> 6);
    if (s >= L.nds) return;
    const uint32_t fill = min((uint32_t)b.fill_out[s], (uint32_t)SR_DOWNSTREAM_BUF_SIZE);
    if (fill == 0) return;
    // the first descriptor whose downstream is >= s
    const uint32_t n = pay_count(b);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (b.packets[mid].shard < s) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && b.packets[lo].shard == s) return;   // its open packet writes the slot
    const uint8_t *const in = b.pend_in + (size_t)s * kPendStride;
    uint8_t *const out = b.pend_out + (size_t)s * kPendStride;
    const uint32_t whole = ((((uintptr_t)in | (uintptr_t)out) & 15u) == 0) ? fill & ~15u : 0u;
    for (uint32_t q = 16u * lane; q < whole; q += 1024u)
        *reinterpret_cast<uint4 *>(out + q) = *reinterpret_cast<const uint4 *>(in + q);
    for (uint32_t q = whole + lane; q < fill; q += 64u) out[q] = in[q];
}

}  // namespace srk
