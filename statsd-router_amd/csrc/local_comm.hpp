// local_comm.hpp — the in-process backend of sr_comm on the device: local_pull_kernel and the HIP side
// of the rendezvous board (local_board.hpp; include/sr_route.h: sr_comm_open_local).
//
// INVARIANT (the machines are shared): no device work is ever enqueued that waits on something not yet
// recorded. Every event is recorded (hipEventRecord has returned) before its handle is posted on the
// board; the only device-side waits are hipStreamWaitEvent on such events; no kernel polls memory; and
// the board's `broken` flag is checked under the board's lock, held while the pull is enqueued. A peer
// that never comes costs host time (bounded by sr_comm_set_timeout), never a stuck stream.
//
// A group's data movement is ONE kernel on the receiver's stream: local_pull_kernel copies every segment
// {src in a peer's allocation, dst in mine, bytes} of the group (up to kPullSegs per launch; more are
// split into several launches). The segment table travels in the kernel arguments, so two groups in
// flight on one stream (sizes, then data) never share a table.
//
// Events come from a ring per communicator (hipEventDisableTiming). A ring slot that is recorded again
// before a peer's hipStreamWaitEvent on it only makes that peer wait for the later record, which is
// also already enqueued: later, never unrecorded. The rings are handed to the group when a communicator
// closes and destroyed with the group, since a peer may still be about to wait for a rank's last event.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "local_board.hpp"
#include "payload_kernel.hpp"

namespace srk {

constexpr uint32_t kPullSegs = 192;          // segments per launch
constexpr uint32_t kPullPieceLog = 14;       // destination-aligned pieces of 16 KiB
constexpr uint32_t kPullPiece = 1u << kPullPieceLog;
constexpr int kPullBlock = 256;              // 256 lanes x 16 bytes x kPullUnroll = one piece
constexpr int kPullUnroll = 4;
constexpr uint32_t kPullMaxGrid = 2048;      // workgroups per launch at most (they stride over the pieces)
constexpr size_t kPullMaxSeg = (size_t)1 << 30;   // longer copies are cut: the buffer descriptor's range is 32 bits
static_assert(kPullBlock * 16 * kPullUnroll == (int)kPullPiece, "a workgroup pass is one piece");

// Addresses are 48 bits: the low words apart, both high halves in one word (four words per segment, so
// that kPullSegs of them fit the kernel arguments).
struct PullArgs {
    uint32_t src_lo[kPullSegs];
    uint32_t dst_lo[kPullSegs];
    uint32_t hi[kPullSegs];      // src bits 32..47 | dst bits 32..47 << 16
    uint32_t bytes[kPullSegs];   // 1 .. kPullMaxSeg
    uint32_t n, pieces;          // segments; pieces of all of them
};
static_assert(sizeof(PullArgs) < 3584, "kernel argument size");

// pieces of a segment: the 16 KiB-aligned blocks of the destination's address space it touches
inline uint32_t pull_piece_count(uint64_t dst, uint32_t bytes) {
    return (uint32_t)(((dst + bytes + (kPullPiece - 1)) >> kPullPieceLog) - (dst >> kPullPieceLog));
}

typedef uint32_t PullU32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) PullU32x4 PullGlobalU32x4;
typedef __attribute__((address_space(1))) uint8_t PullGlobalU8;

// The multi-segment copy. A workgroup takes pieces p = blockIdx.x, + gridDim.x, ...; a piece finds its
// segment in the segments' piece prefix sums (LDS). Inside a piece every lane owns aligned 16-byte units
// of the destination: a unit that lies whole inside the segment is one aligned dwordx4 store fed by one
// 16-byte buffer load at the matching (arbitrarily aligned) source byte; the segment's first and last
// partial units are byte stores of the segment's own bytes, fed by byte loads wherever a 16-byte load
// would cross an end of the source (pay_fetch16). Nothing outside [src, src + bytes) is read, nothing
// outside [dst, dst + bytes) is written, and each byte is written once.
__global__ __launch_bounds__(kPullBlock) void local_pull_kernel(PullArgs a) {
    __shared__ uint32_t s_end[kPullBlock];   // inclusive prefix of the segments' piece counts
    __shared__ uint32_t s_wave[kPullBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t cnt = 0;
    if (tid < a.n) {
        const uint64_t d = ((uint64_t)(a.hi[tid] >> 16) << 32) | a.dst_lo[tid];
        cnt = (uint32_t)(((d + a.bytes[tid] + (kPullPiece - 1)) >> kPullPieceLog) - (d >> kPullPieceLog));
    }
    const uint32_t incl = wave_incl_add32(cnt);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < (uint32_t)(kPullBlock / 64); ++w) before += w < wave ? s_wave[w] : 0u;
    s_end[tid] = before + incl;
    __syncthreads();

    for (uint32_t p = blockIdx.x; p < a.pieces; p += gridDim.x) {
        uint32_t lo = 0, hi = a.n - 1u;   // the first segment whose prefix passes p
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_end[mid] > p) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t seg = lo;
        const uint32_t k = p - (seg ? s_end[seg - 1u] : 0u);   // the piece's index in its segment
        const uint32_t h = a.hi[seg], nb = a.bytes[seg];
        const uint64_t src = ((uint64_t)(h & 0xFFFFu) << 32) | a.src_lo[seg];
        const uint64_t d = ((uint64_t)(h >> 16) << 32) | a.dst_lo[seg];
        const uint64_t A0 = ((d >> kPullPieceLog) + k) << kPullPieceLog;
        const uint64_t w_lo = A0 > d ? A0 : d;
        const uint64_t w_hi = A0 + kPullPiece < d + nb ? A0 + kPullPiece : d + nb;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)src, (short)0, (int)nb, 0x00020000);
        uint4 v[kPullUnroll];
#pragma unroll
        for (int u = 0; u < kPullUnroll; ++u) {
            const uint64_t A = A0 + 16u * (uint32_t)(u * kPullBlock + (int)tid);
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (A + 16u > w_lo && A < w_hi) v[u] = pay_fetch16(rsrc, (int64_t)(A - d), nb);
        }
#pragma unroll
        for (int u = 0; u < kPullUnroll; ++u) {
            const uint64_t A = A0 + 16u * (uint32_t)(u * kPullBlock + (int)tid);
            // (the destination is rebuilt from integers: the global address space is said outright, or the
            // stores would be flat ones)
            if (A >= w_lo && A + 16u <= w_hi) {
                *(PullGlobalU32x4 *)A = PullU32x4{v[u].x, v[u].y, v[u].z, v[u].w};
            } else if (A + 16u > w_lo && A < w_hi) {   // an end of the segment: its own bytes only
                const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                const int b0 = A < w_lo ? (int)(w_lo - A) : 0, b1 = A + 16u > w_hi ? (int)(w_hi - A) : 16;
                PullGlobalU8 *const o = (PullGlobalU8 *)A;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (i >= b0 && i < b1) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

// Enqueue the copies of one group on `stream`: kPullSegs segments per launch, longer copies cut.
inline int pull_launch(hipStream_t stream, const BoardSeg *segs, size_t n) {
    PullArgs a;
    a.n = a.pieces = 0;
    auto flush = [&]() -> int {
        if (!a.n) return 0;
        const uint32_t grid = a.pieces < kPullMaxGrid ? a.pieces : kPullMaxGrid;
        hipLaunchKernelGGL(local_pull_kernel, dim3(grid), dim3(kPullBlock), 0, stream, a);
        a.n = a.pieces = 0;
        return hipGetLastError() == hipSuccess ? 0 : -EIO;
    };
    for (size_t i = 0; i < n; ++i) {
        const uint64_t s = (uint64_t)(uintptr_t)segs[i].src, d = (uint64_t)(uintptr_t)segs[i].dst;
        if (!segs[i].bytes) continue;
        if (!s || !d || ((s + segs[i].bytes) >> 48) || ((d + segs[i].bytes) >> 48)) return -EINVAL;
        for (size_t off = 0; off < segs[i].bytes; off += kPullMaxSeg) {
            const size_t len = segs[i].bytes - off < kPullMaxSeg ? segs[i].bytes - off : kPullMaxSeg;
            int rc;
            if (a.n == kPullSegs && (rc = flush())) return rc;
            const uint64_t ss = s + off, dd = d + off;
            a.src_lo[a.n] = (uint32_t)ss;
            a.dst_lo[a.n] = (uint32_t)dd;
            a.hi[a.n] = (uint32_t)(ss >> 32) | ((uint32_t)(dd >> 32) << 16);
            a.bytes[a.n] = (uint32_t)len;
            a.pieces += pull_piece_count(dd, (uint32_t)len);
            ++a.n;
        }
    }
    return flush();
}

// The ranks' meeting place (sr_comm_group): the board, and the event rings of closed communicators.
struct LocalGroup {
    explicit LocalGroup(int world) : board(world) {}
    LocalBoard board;
    std::mutex mu;
    std::vector<hipEvent_t> retired;
};

constexpr int kLocalEvents = 64;

// One rank of a group (the local half of sr_comm).
struct LocalComm {
    LocalGroup *group = nullptr;
    int rank = -1;
    hipEvent_t events[kLocalEvents] = {};
    int n_events = 0;
    unsigned next_event = 0;
    bool in_group = false;
    std::vector<BoardOp> ops;
};

// run_group's device: the calling rank's stream.
struct LocalDev {
    LocalComm *lc;
    hipStream_t stream;
    int record(void **ev) {
        hipEvent_t e = lc->events[lc->next_event++ % (unsigned)lc->n_events];
        if (hipEventRecord(e, stream) != hipSuccess) return -EIO;
        *ev = (void *)e;
        return 0;
    }
    int wait(void *ev) { return hipStreamWaitEvent(stream, (hipEvent_t)ev, 0) == hipSuccess ? 0 : -EIO; }
    int pull(const BoardSeg *segs, size_t n) { return pull_launch(stream, segs, n); }
};

inline int local_events_create(LocalComm &lc) {
    for (lc.n_events = 0; lc.n_events < kLocalEvents; ++lc.n_events)
        if (hipEventCreateWithFlags(&lc.events[lc.n_events], hipEventDisableTiming) != hipSuccess) return -ENOMEM;
    return 0;
}

// the ring goes to the group (destroyed with it): a peer may still wait for this rank's last event
inline void local_events_retire(LocalComm &lc) {
    std::lock_guard<std::mutex> lk(lc.group->mu);
    for (int i = 0; i < lc.n_events; ++i) lc.group->retired.push_back(lc.events[i]);
    lc.n_events = 0;
}

// A capturing stream cannot take a collective that does host work in between.
inline int local_stream_ok(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) return -EIO;
    return st == hipStreamCaptureStatusNone ? 0 : -EINVAL;
}

}  // namespace srk
