// log_kernel.hpp — a batch's log text formatted on the device.
//
// At log_level TRACE the reference writes, per datagram, "got packet" and, per line, its WARN or its two
// find_downstream messages (sr-main.c:91,102,115,142,174,184; host/sr_core.c trace_batch). Every input of
// those messages is on the device after the route launch: the framed bytes, the input-order records, the
// 64-bit hashes and the framed datagram ends. These kernels write the messages back to back into one arena,
// each as prefix[level] + header + span + '\n' (log_host.hpp), in the reference's order.
//
// A record owns a group of up to three messages, always in this order:
//   slot 0  "got packet", when the record starts a datagram (its offset is the end before ends[g]);
//   slot 1  the line's message: invalid length, invalid metric, or hash / length / line;
//   slot 2  "pushing to downstream" or "all downstreams are dead".
// Three launches; no workgroup waits for another (no look-back, no spin, no returning atomic):
//   log_lens_kernel   one record per thread: its group's bytes and messages (the datagram by a binary search
//                     of ends, the spans' NUL cuts by 16-byte loads), summed per workgroup of kLogRecs records;
//   log_scan_kernel   one workgroup turns the sums into exclusive bases (DPP wave scans) and writes the
//                     totals;
//   log_write_kernel  a workgroup owns kLogRecs consecutive records, i.e. one contiguous destination range.
//                     It computes the same groups again, scans them, lays every message's descriptor and
//                     header into LDS, and then every thread owns aligned 16-byte pieces of the range
//                     (payload_kernel.hpp's discipline): a piece inside one span is one unaligned dwordx4
//                     buffer load and one aligned dwordx4 store; any other piece is composed byte by byte
//                     from the prefixes and headers in LDS and the input. The pieces a range shares with its
//                     neighbours are byte stores of the range's own bytes, so no two workgroups write the
//                     same byte and nothing is read back.
// The groups are computed twice (once per pass) instead of being kept: per-record scratch would be 8 bytes per
// input byte in the worst case, the sums are 16 bytes per kLogRecs records.
#pragma once

#include "log_host.hpp"
#include "payload_kernel.hpp"

namespace srk {

constexpr int kLogRecs = 128;                 // records (and threads) per workgroup
constexpr int kLogMsgs = 3 * kLogRecs;        // messages a workgroup can hold
constexpr int kLogHdrStride = 68;             // kLogMaxHeader rounded up to 4

struct LogArgs {
    const uint8_t *bytes;
    const sr_record *recs;
    const uint64_t *n_records;
    const uint64_t *hashes;      // null only when warn_only
    const uint32_t *ends;        // [n_ends] framed datagram ends
    const uint8_t *prefix;       // plen[0] TRACE bytes, then plen[1] WARN bytes
    uint8_t *text;
    uint32_t *offsets;           // null or [max_msgs + 1]
    uint8_t *levels;             // null or [max_msgs]
    uint64_t *total, *n_msgs;
    uint64_t *gsum;              // scratch: per workgroup {bytes, messages}, then their exclusive bases
    uint64_t text_cap, max_msgs;
    uint32_t nbytes, rec_room, n_ends, nds;
    uint32_t plen[2];
    uint32_t max_msg, warn_only;
};

struct LogSlot {
    uint32_t on, kind, src, slen;
};

struct LogGroup {
    LogSlot s[3];
    uint64_t hash;
    uint32_t len, route;
};

__device__ __forceinline__ uint32_t log_nrec(const LogArgs &a) {
    const uint64_t n = *a.n_records;
    return (uint32_t)(n < a.rec_room ? n : a.rec_room);
}

// The span [src, src + len) of the input cut before its first NUL. src + len <= nbytes.
__device__ __forceinline__ uint32_t log_nul_cut(__amdgpu_buffer_rsrc_t rsrc, uint32_t src, uint32_t len, uint32_t nbytes) {
    for (uint32_t k = 0; k < len; k += 16u) {
        const uint4 v = pay_fetch16(rsrc, (int64_t)src + k, nbytes);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t z = (w[d] - 0x01010101u) & ~w[d] & 0x80808080u;   // its lowest set bit: the first zero byte
            if (z) return min(k + 4u * (uint32_t)d + ((uint32_t)__builtin_ctz(z) >> 3), len);
        }
    }
    return len;
}

// Record i's group. Every span lies inside [0, nbytes) whatever the record says.
__device__ __forceinline__ LogGroup log_group(const LogArgs &a, __amdgpu_buffer_rsrc_t rsrc, uint32_t i) {
    LogGroup g;
    const uint2 w = *reinterpret_cast<const uint2 *>(a.recs + i);
    const uint32_t off = w.x;
    g.len = w.y & 0xFFFFu;
    g.route = w.y >> 16;
    g.hash = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) g.s[k].on = g.s[k].kind = g.s[k].src = g.s[k].slen = 0u;
    const uint32_t src = min(off, a.nbytes);
    const uint32_t room = a.nbytes - src;
    const uint32_t scan_most = a.max_msg ? a.max_msg : 0xFFFFFFFFu;   // bytes past the cut are never printed
    // slot 0: the datagram this record starts
    if (!a.warn_only && a.n_ends) {
        uint32_t lo = 0, hi = a.n_ends;   // the first datagram whose end is past the record's offset
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.ends[mid] > off) hi = mid;
            else lo = mid + 1u;
        }
        if (lo < a.n_ends && (lo ? a.ends[lo - 1u] : 0u) == off) {
            const uint32_t e = min(a.ends[lo], a.nbytes);
            g.s[0].on = 1u;
            g.s[0].kind = LOG_GOT_PACKET;
            g.s[0].src = src;
            g.s[0].slen = log_nul_cut(rsrc, src, min(e > src ? e - src : 0u, scan_most), a.nbytes);
        }
    }
    // slots 1 and 2: the line
    uint32_t span = g.len;
    if (g.route == SR_ROUTE_INVALID_LENGTH) {
        g.s[1].on = 1u;
        g.s[1].kind = LOG_BAD_LENGTH;
    } else if (g.route == SR_ROUTE_INVALID_FORMAT) {
        g.s[1].on = 1u;
        g.s[1].kind = LOG_BAD_FORMAT;
        span = g.len ? g.len - 1u : 0u;
    } else {
        g.s[1].on = a.warn_only ? 0u : 1u;
        g.s[1].kind = LOG_HASH;
        if (g.route < a.nds) {
            g.s[2].on = a.warn_only ? 0u : 1u;
            g.s[2].kind = LOG_PUSH;
        } else {
            g.s[2].on = 1u;
            g.s[2].kind = LOG_DEAD;
        }
        if (g.s[1].on) g.hash = a.hashes[i];
    }
    if (g.s[1].on) {
        g.s[1].src = src;
        g.s[1].slen = log_nul_cut(rsrc, src, min(min(span, room), scan_most), a.nbytes);
    }
    return g;
}

// bytes of slot k before its '\n' (prefix + header + span, cut at max_msg)
__device__ __forceinline__ uint32_t log_slot_keep(const LogArgs &a, const LogGroup &g, int k, uint32_t &plen, uint32_t &hlen) {
    plen = a.plen[log_kind_warn(g.s[k].kind)];
    hlen = log_header_len(g.s[k].kind, g.hash, g.len, g.route);
    return log_keep(plen, hlen, g.s[k].slen, a.max_msg);
}

__device__ __forceinline__ void log_group_sizes(const LogArgs &a, const LogGroup &g, uint32_t &bytes, uint32_t &msgs) {
    bytes = msgs = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (g.s[k].on) {
            uint32_t plen, hlen;
            bytes += log_slot_keep(a, g, k, plen, hlen) + 1u;
            ++msgs;
        }
}

__global__ __launch_bounds__(kLogRecs) void log_lens_kernel(LogArgs a) {
    __shared__ uint32_t s_wave[kLogRecs / 64][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nrec = log_nrec(a);
    if (blockIdx.x * (uint32_t)kLogRecs >= nrec) return;   // (workgroup-uniform)
    const uint32_t i = blockIdx.x * (uint32_t)kLogRecs + tid;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.bytes, (short)0, (int)a.nbytes, 0x00020000);
    uint32_t bytes = 0, msgs = 0;
    if (i < nrec) {
        const LogGroup g = log_group(a, rsrc, i);
        log_group_sizes(a, g, bytes, msgs);
    }
    const uint32_t ib = wave_incl_add32(bytes), im = wave_incl_add32(msgs);
    if (lane == 63u) {
        s_wave[wave][0] = ib;
        s_wave[wave][1] = im;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t b = 0, m = 0;
        for (int w = 0; w < kLogRecs / 64; ++w) {
            b += s_wave[w][0];
            m += s_wave[w][1];
        }
        a.gsum[2 * (size_t)blockIdx.x] = b;
        a.gsum[2 * (size_t)blockIdx.x + 1] = m;
    }
}

// The workgroups' {bytes, messages} into exclusive bases, in place; the totals. A workgroup's bytes stay below
// 2^32 (kLogMaxBatch), so they are scanned as two 16-bit halves whose sums over 1024 values fit 32 bits.
__global__ __launch_bounds__(1024) void log_scan_kernel(LogArgs a) {
    __shared__ uint32_t s_wave[16][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nrec = log_nrec(a);
    const uint32_t ng = (nrec + (uint32_t)kLogRecs - 1u) / (uint32_t)kLogRecs;
    uint64_t run_b = 0, run_m = 0;
    for (uint32_t g0 = 0; g0 < ng; g0 += 1024u) {
        const uint32_t g = g0 + tid;
        uint32_t lo = 0, hi = 0, m = 0;
        if (g < ng) {
            const uint64_t b = a.gsum[2 * (size_t)g];
            lo = (uint32_t)b & 0xFFFFu;
            hi = (uint32_t)(b >> 16);
            m = (uint32_t)a.gsum[2 * (size_t)g + 1];
        }
        const uint32_t il = wave_incl_add32(lo), ih = wave_incl_add32(hi), im = wave_incl_add32(m);
        if (lane == 63u) {
            s_wave[wave][0] = il;
            s_wave[wave][1] = ih;
            s_wave[wave][2] = im;
        }
        __syncthreads();
        uint64_t before_b = 0, all_b = 0, before_m = 0, all_m = 0;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint64_t tb = (uint64_t)s_wave[w][0] + ((uint64_t)s_wave[w][1] << 16);
            const uint64_t tm = s_wave[w][2];
            before_b += w < wave ? tb : 0u;
            before_m += w < wave ? tm : 0u;
            all_b += tb;
            all_m += tm;
        }
        if (g < ng) {
            a.gsum[2 * (size_t)g] = run_b + before_b + ((uint64_t)(il - lo) + ((uint64_t)(ih - hi) << 16));
            a.gsum[2 * (size_t)g + 1] = run_m + before_m + (im - m);
        }
        run_b += all_b;
        run_m += all_m;
        __syncthreads();
    }
    if (tid == 0) {
        *a.total = run_b;
        *a.n_msgs = run_m;
        if (a.offsets && run_m <= a.max_msgs) a.offsets[run_m] = (uint32_t)run_b;
    }
}

__global__ __launch_bounds__(kLogRecs) void log_write_kernel(LogArgs a) {
    __shared__ uint32_t s_start[kLogMsgs + 1];   // a message's first byte in the workgroup's range
    __shared__ uint32_t s_src[kLogMsgs];         // its span's first input byte
    __shared__ uint32_t s_keep[kLogMsgs];        // its bytes before the '\n'
    __shared__ uint32_t s_meta[kLogMsgs];        // prefix bytes | header bytes << 12 | WARN << 20
    __shared__ uint8_t s_hdr[kLogMsgs][kLogHdrStride];
    __shared__ uint8_t s_pfx[2][kLogMaxPrefix];
    __shared__ uint32_t s_wave[kLogRecs / 64][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nrec = log_nrec(a);
    if (blockIdx.x * (uint32_t)kLogRecs >= nrec) return;   // (workgroup-uniform)
    const uint32_t i = blockIdx.x * (uint32_t)kLogRecs + tid;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.bytes, (short)0, (int)a.nbytes, 0x00020000);
    for (uint32_t p = tid; p < a.plen[0]; p += (uint32_t)kLogRecs) s_pfx[0][p] = a.prefix[p];
    for (uint32_t p = tid; p < a.plen[1]; p += (uint32_t)kLogRecs) s_pfx[1][p] = a.prefix[a.plen[0] + p];
    LogGroup g;
    uint32_t bytes = 0, msgs = 0;
    if (i < nrec) {
        g = log_group(a, rsrc, i);
        log_group_sizes(a, g, bytes, msgs);
    }
    const uint32_t ib = wave_incl_add32(bytes), im = wave_incl_add32(msgs);
    if (lane == 63u) {
        s_wave[wave][0] = ib;
        s_wave[wave][1] = im;
    }
    __syncthreads();
    uint32_t b0 = ib - bytes, m0 = im - msgs, B = 0, M = 0;
    for (uint32_t w = 0; w < (uint32_t)(kLogRecs / 64); ++w) {
        b0 += w < wave ? s_wave[w][0] : 0u;
        m0 += w < wave ? s_wave[w][1] : 0u;
        B += s_wave[w][0];
        M += s_wave[w][1];
    }
    const uint64_t S = a.gsum[2 * (size_t)blockIdx.x];        // the range's first byte of the text
    const uint64_t M0 = a.gsum[2 * (size_t)blockIdx.x + 1];   // its first message
    if (i < nrec) {
        uint32_t at = b0, idx = m0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (g.s[k].on) {
                uint32_t plen, hlen;
                const uint32_t keep = log_slot_keep(a, g, k, plen, hlen);
                const uint32_t warn = log_kind_warn(g.s[k].kind);
                s_start[idx] = at;
                s_src[idx] = g.s[k].src;
                s_keep[idx] = keep;
                s_meta[idx] = plen | (hlen << 12) | (warn << 20);
                log_header(s_hdr[idx], g.s[k].kind, g.hash, g.len, g.route);
                const uint64_t gi = M0 + idx;
                if (a.offsets && gi <= a.max_msgs) a.offsets[gi] = (uint32_t)(S + at);
                if (a.levels && gi < a.max_msgs) a.levels[gi] = warn ? (uint8_t)3 : (uint8_t)0;
                at += keep + 1u;
                ++idx;
            }
    }
    if (tid == 0) s_start[M] = B;
    __syncthreads();
    // bytes [S, S + w1) of the text are this range's, cut at the capacity
    const uint32_t w1 = S >= a.text_cap ? 0u : (uint32_t)min((uint64_t)B, a.text_cap - S);
    if (w1 == 0u || M == 0u) return;
    uint8_t *const dst = a.text + S;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t *const base = dst - mis;            // 16-byte aligned; piece c covers base + 16 c
    const uint32_t x1 = mis + w1;               // the written range in piece coordinates: [mis, x1)
    const uint32_t npieces = (x1 + 15u) >> 4;
    for (uint32_t c = tid; c < npieces; c += (uint32_t)kLogRecs) {
        const uint32_t A = 16u * c;
        const uint32_t s0 = max(A, mis), s1 = min(A + 16u, x1);   // this piece's bytes of the range
        const uint32_t q0 = s0 - mis;                              // as a range position
        // the message that holds q0: the last one that starts at or before it
        uint32_t m = 0, hi = M - 1u;
        while (m < hi) {
            const uint32_t mid = (m + hi + 1u) >> 1;
            if (s_start[mid] <= q0) m = mid;
            else hi = mid - 1u;
        }
        uint32_t ms = s_start[m], mnext = s_start[m + 1u], keep = s_keep[m], src = s_src[m], meta = s_meta[m];
        uint32_t body = (meta & 0xFFFu) + ((meta >> 12) & 0xFFu);   // the span's first byte in the message
        uint4 acc;
        const uint32_t t0 = q0 - ms;
        if (s1 - s0 == 16u && t0 >= body && t0 + 16u <= keep) {   // the piece lies inside one span
            acc = pay_fetch16(rsrc, (int64_t)src + (t0 - body), a.nbytes);
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t x = A + (uint32_t)k;
                if (x >= s0 && x < s1) {
                    const uint32_t q = x - mis;
                    while (q >= mnext && m + 1u < M) {
                        ++m;
                        ms = mnext;
                        mnext = s_start[m + 1u];
                        keep = s_keep[m];
                        src = s_src[m];
                        meta = s_meta[m];
                        body = (meta & 0xFFFu) + ((meta >> 12) & 0xFFu);
                    }
                    const uint32_t t = q - ms, plen = meta & 0xFFFu;
                    uint32_t v;
                    if (t >= keep) v = (uint32_t)'\n';
                    else if (t < plen) v = s_pfx[(meta >> 20) & 1u][t];
                    else if (t < body) v = s_hdr[m][t - plen];
                    else v = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rsrc, src + (t - body), 0, 0);
                    w[k >> 2] |= (v & 0xFFu) << (8 * (k & 3));
                }
            }
            acc = make_uint4(w[0], w[1], w[2], w[3]);
        }
        uint8_t *const o = base + A;
        if (s1 - s0 == 16u) {
            *reinterpret_cast<uint4 *>(o) = acc;
        } else {   // a piece shared with a neighbouring range (or an end of the text): this range's bytes only
            const uint32_t w[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((uint32_t)k >= s0 - A && (uint32_t)k < s1 - A) o[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace srk
