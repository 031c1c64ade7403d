// owner_kernel.hpp — the owner side of the multi-GPU regroup ("Owner side").
//
// After the exchange an owner GPU holds the lines of its shards in source order (exchange.hpp). It is
// the one data thread of those shards: it first drops the pending buffer of every shard that any
// source's launch probed dead (find_downstream, sr-main.c:106), then pushes the received lines
// (push_to_downstream / ds_schedule_flush, sr-main.c:49-83). The packing (mtu_kernel.hpp) and the gather
// (payload_kernel.hpp) do the second step unchanged; the kernels here put the receive buffer into the
// shape those take and move the drop in front of them:
//   owner_dead_or_kernel  a launch's per-batch probed-dead bitmaps ORed into the rank's row of the
//                         [world][nwords] table the ranks then exchange (sr_exchange_dead_run);
//   owner_fold_kernel     one workgroup: the received line total (the sum of recv_counts[p][0]) into one
//                         u64, and fill_eff[s] = 0 where any row of the table has bit s, else fill_in[s].
//                         The packing then runs with fill_in = fill_eff and no bitmap of its own: a
//                         dropped shard's lines are packed with carry 0 instead of being discarded with it;
//   flush_scan_kernel /   ds_flush_timer_cb (sr-main.c:194-204) for pending buffers kept on the device: one
//   flush_copy_kernel     workgroup scans the fills into descriptors and arena offsets, then one wave per
//                         descriptor copies the slot's bytes (aligned 16-byte pieces of the arena from an
//                         unaligned dwordx4 buffer load, the ends as byte stores) and zeroes the fill of
//                         every slot that went out whole.
#pragma once

#include "exchange.hpp"
#include "payload_kernel.hpp"

namespace srk {

constexpr int kOwnerMaxBatches = 32;   // SR_MAX_BATCHES_PER_LAUNCH
constexpr int kOwnerBlock = 1024;      // the fold's and the flush scan's one workgroup
constexpr int kDeadTag = 2;            // sr_transport tag of a bitmap row

struct DeadOrArgs {
    const uint64_t *pd[kOwnerMaxBatches];   // null: the batch contributes nothing
    uint64_t *row;                          // [nwords]
    uint32_t count, nwords;
};

__global__ __launch_bounds__(64) void owner_dead_or_kernel(DeadOrArgs a) {
    const uint32_t w = blockIdx.x * 64u + threadIdx.x;
    if (w >= a.nwords) return;
    uint64_t v = 0;
    for (uint32_t j = 0; j < a.count; ++j)
        if (a.pd[j]) v |= a.pd[j][w];
    a.row[w] = v;
}

struct OwnerFoldArgs {
    const uint64_t *recv_counts;   // [world][2] {lines, bytes}
    const uint64_t *all_dead;      // null or [world][nwords]
    const uint16_t *fill_in;       // null: zeros
    uint64_t *n_out;               // the stream's line count
    uint16_t *fill_eff;            // [nds]
    uint32_t world, nds, nwords;
};

__global__ __launch_bounds__(kOwnerBlock) void owner_fold_kernel(OwnerFoldArgs a) {
    __shared__ uint64_t s_dead[kMaxOwners];   // nwords <= 4096 / 64
    const uint32_t tid = threadIdx.x;
    if (tid < 64u) {   // wave 0: the line total (world <= 64: one source per lane)
        unsigned long long v = tid < a.world ? a.recv_counts[2 * (size_t)tid] : 0ull;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (tid == 0) *a.n_out = v;
    } else if (tid - 64u < a.nwords) {   // waves 1 and up: the bitmap's column-OR
        const uint32_t w = tid - 64u;
        uint64_t v = 0;
        if (a.all_dead)
            for (uint32_t p = 0; p < a.world; ++p) v |= a.all_dead[(size_t)p * a.nwords + w];
        s_dead[w] = v;
    }
    __syncthreads();
    for (uint32_t s = tid; s < a.nds; s += (uint32_t)kOwnerBlock) {
        const bool dead = (s_dead[s >> 6] >> (s & 63u)) & 1ull;
        a.fill_eff[s] = dead ? (uint16_t)0 : (a.fill_in ? a.fill_in[s] : (uint16_t)0);
    }
}

struct FlushArgs {
    uint16_t *fill;          // [nds] in: pending bytes; out: 0 where flushed
    const uint8_t *pend;     // [nds] slots of kPendStride bytes
    sr_packet *packets;      // [max_packets]
    uint64_t *counts;        // 3 u64
    uint8_t *payload;
    uint32_t *offsets;       // [max_packets + 1]
    uint64_t *total;
    uint64_t payload_cap;
    uint32_t nds, max_packets;
};

// descriptors and offsets: a slot with bytes is descriptor number (slots with bytes before it)
__global__ __launch_bounds__(kOwnerBlock) void flush_scan_kernel(FlushArgs a) {
    __shared__ uint32_t s_cnt[16], s_len[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t run_cnt = 0, run_len = 0;
    for (uint32_t s0 = 0; s0 < a.nds; s0 += (uint32_t)kOwnerBlock) {
        const uint32_t s = s0 + tid;
        const uint32_t f = s < a.nds ? min((uint32_t)a.fill[s], (uint32_t)SR_DOWNSTREAM_BUF_SIZE) : 0u;
        const uint32_t has = f ? 1u : 0u;
        const uint32_t ci = wave_incl_add32(has);
        if (lane == 63u) s_cnt[wave] = ci;
        __syncthreads();
        uint32_t cb = 0, call = 0;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t t = s_cnt[w];
            cb += w < wave ? t : 0u;
            call += t;
        }
        const uint32_t idx = run_cnt + cb + ci - has;          // this slot's descriptor
        const bool fits = has && idx < a.max_packets;
        const uint32_t v = fits ? f : 0u;                      // only written descriptors take arena bytes
        const uint32_t li = wave_incl_add32(v);
        if (lane == 63u) s_len[wave] = li;
        __syncthreads();
        uint32_t lb = 0, lall = 0;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t t = s_len[w];
            lb += w < wave ? t : 0u;
            lall += t;
        }
        if (fits) {
            sr_packet pk;
            pk.first = 0;
            pk.nlines = 0;
            pk.shard = (uint16_t)s;
            pk.length = 0;
            pk.carry = (uint16_t)f;
            pk.open = 0;
            a.packets[idx] = pk;
            a.offsets[idx] = run_len + lb + li - v;
        }
        run_cnt += call;
        run_len += lall;
    }
    if (tid == 0) {
        a.counts[0] = run_cnt;
        a.counts[1] = 0;
        a.counts[2] = 0;
        a.offsets[run_cnt < a.max_packets ? run_cnt : a.max_packets] = run_len;
        *a.total = run_len;
    }
}

// one wave per descriptor: the slot's bytes into the arena, cut at the arena's capacity
__global__ __launch_bounds__(kPayBlock) void flush_copy_kernel(FlushArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (uint32_t)kPayWaves + (threadIdx.x >> 6);
    const uint64_t nd = a.counts[0];
    const uint32_t n = (uint32_t)(nd < a.max_packets ? nd : a.max_packets);
    if (i >= n) return;
    const sr_packet pk = a.packets[i];
    const uint32_t s = pk.shard;
    if (s >= a.nds) return;
    const uint32_t f = min((uint32_t)pk.carry, (uint32_t)SR_DOWNSTREAM_BUF_SIZE);
    const uint64_t off = a.offsets[i];
    const uint32_t w1 = off >= a.payload_cap ? 0u : (uint32_t)min((uint64_t)f, a.payload_cap - off);
    const uint32_t pend_bytes = a.nds * kPendStride;   // <= 4096 * 1456
    const uint32_t at = s * kPendStride;
    const uint8_t *const in = a.pend + at;
    uint8_t *const dst = a.payload + off;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.pend, (short)0, (int)pend_bytes, 0x00020000);
    // bytes up to the arena's first 16-byte boundary, whole aligned pieces, the rest
    const uint32_t head = min(w1, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint32_t whole = (w1 - head) & ~15u;
    for (uint32_t q = lane; q < head; q += 64u) dst[q] = in[q];
    for (uint32_t q = head + 16u * lane; q < head + whole; q += 1024u)   // q + 16 <= 1450: inside the slot
        *reinterpret_cast<uint4 *>(dst + q) = pay_fetch16(rs, (int64_t)at + q, pend_bytes);
    for (uint32_t q = head + whole + lane; q < w1; q += 64u) dst[q] = in[q];
    if (lane == 0 && w1 == f) a.fill[s] = 0;   // went out whole
}

// The probed-dead rows over a transport (sr_exchange_dead_run, after the OR kernel): within one group, the
// rank's row to every peer and every peer's row from it, in rank order. Every operation is posted even
// after one fails, so that no peer waits inside its group; the first error is returned.
inline int exchange_dead_rows(const sr_transport &t, int world, int rank, uint64_t *all_dead, uint32_t nwords) {
    if (world == 1) return 0;
    if (!t.group_start || !t.group_end || !t.send || !t.recv) return -EINVAL;
    const size_t row = (size_t)nwords * sizeof(uint64_t);
    int rc = t.group_start(t.user);
    if (rc) return rc;
    int bad = 0;
    for (int q = 0; q < world; ++q) {
        if (q == rank) continue;
        int r = t.send(t.user, all_dead + (size_t)rank * nwords, row, q, kDeadTag);
        if (r && !bad) bad = r;
        r = t.recv(t.user, all_dead + (size_t)q * nwords, row, q, kDeadTag);
        if (r && !bad) bad = r;
    }
    rc = t.group_end(t.user);
    return bad ? bad : rc;
}

}  // namespace srk
