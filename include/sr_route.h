/*
 * sr_route.h — C ABI of the MI355X-native statsd-router hot path.
 *
 * The reference (hulu/statsd-router) has no plugin or FFI API: its hot path is the libev
 * callback `udp_read_cb` (sr-main.c:149-191), which frames one datagram and, per '\n'-terminated
 * line, calls `process_data_line` (sr-main.c:137-147) -> `hash` (sr-main.c:120-134) ->
 * `find_downstream` (sr-main.c:86-117) -> `push_to_downstream` (sr-main.c:73-83).
 * This header replaces the per-line calls with one call per BATCH of framed datagrams:
 * the GPU classifies every line (length gate, ':' presence, sdbm name hash, consistent-hash
 * shard pick) and returns one record per line in input order. The host caller keeps the
 * reference's side effects: it walks the records and does push_to_downstream, the WARN log
 * lines (exact reference text) and the dead-downstream buffer drop (sr-main.c:106).
 *
 * Conventions (mirroring the reference):
 *   - every function returns 0 or a negative errno value; nothing aborts;
 *   - a context is not thread-safe: use one per data thread / HIP stream, like one libev loop
 *     per thread (sr-main.c:237-308);
 *   - the alive bitmap is a snapshot (the reference reads the `alive:1` bit of
 *     ds_health_client_s (sr-types.h:25) racily per line; a per-batch snapshot is a valid
 *     linearisation of that).
 *
 * No torch or HIP types appear in the signatures: device pointers are plain pointers and the
 * stream is an opaque `void *` (a hipStream_t).
 */
#ifndef SR_ROUTE_H
#define SR_ROUTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants of the reference contract ------------------------------------------------ */
#define SR_DATA_BUF_SIZE        4096u  /* sr-main.h:46: recv buffer; recv() reads at most 4095 B */
#define SR_MAX_DATAGRAM         (SR_DATA_BUF_SIZE - 1u)   /* sr-main.c:163 */
#define SR_DOWNSTREAM_BUF_SIZE  1450u  /* sr-types.h:30: a valid line is shorter than this      */
#define SR_MIN_LINE_LENGTH      6u     /* sr-main.c:180: `line_length > 5`                        */
#define SR_MAX_LINE_LENGTH      (SR_DOWNSTREAM_BUF_SIZE - 1u)  /* sr-main.c:180: `< 1450`         */
#define SR_MAX_DOWNSTREAMS      65533u /* shard ids must fit below the SR_ROUTE_* codes         */

/* ---- per-line verdicts -------------------------------------------------------------------- */
enum sr_verdict {
    SR_VALID          = 0, /* routed: process_data_line -> find_downstream -> push (sr-main.c:103) */
    SR_INVALID_LENGTH = 1, /* WARN "udp_read_cb: invalid length %d of metric %.*s" (sr-main.c:184)  */
    SR_INVALID_FORMAT = 2, /* WARN "process_data_line: invalid metric %s" (sr-main.c:142)            */
    SR_ALL_DEAD       = 3  /* WARN "find_downstream: all downstreams are dead" (sr-main.c:115)       */
};

/* `route` field: the shard id (0..n_downstreams-1) for SR_VALID, else one of these codes. */
#define SR_ROUTE_INVALID_LENGTH 0xFFFDu
#define SR_ROUTE_INVALID_FORMAT 0xFFFEu
#define SR_ROUTE_ALL_DEAD       0xFFFFu

/* One record per '\n'-terminated line, in input order. 8 bytes, little-endian, no padding. */
typedef struct sr_record {
    uint32_t offset; /* byte offset of the line's first byte in the batch                  */
    uint16_t length; /* bytes including the '\n' (saturates at 0xFFFF; lines > 4096 B only  */
                     /* occur when the caller breaks the framing contract)                  */
    uint16_t route;  /* shard id, or SR_ROUTE_*                                             */
} sr_record;

static inline int sr_record_verdict(const sr_record *r) {
    return r->route < SR_ROUTE_INVALID_LENGTH ? SR_VALID : (int)(r->route - 0xFFFCu);
}

/* ---- host-side framing (no GPU) ----------------------------------------------------------- */
/* Frame one received datagram exactly as udp_read_cb does (sr-main.c:163-173): keep at most
 * SR_MAX_DATAGRAM bytes (the recv() cap) and append '\n' if the last kept byte is not one.
 * Writes at most len+1 (<= 4096) bytes to dst; returns the framed length (0 for an empty datagram).
 * dst must not overlap src. */
size_t sr_frame_datagram(uint8_t *dst, const uint8_t *src, size_t len);

/* Frame `count` datagrams back to back into dst (capacity dst_cap). Returns the total framed
 * length, or (size_t)-1 if dst_cap is too small. */
size_t sr_frame_datagrams(uint8_t *dst, size_t dst_cap, const uint8_t *const *dgrams,
                          const size_t *lens, size_t count);

/* The framed size of datagrams that stay where recvmmsg left them (host only, nothing is moved):
 * datagram j occupies bytes [j * stride, j * stride + lens[j]) of `slots`. Returns what sr_frame_datagrams
 * would return for them, looking at one byte per datagram, and, with ends != NULL, ends[j] = the framed end
 * offset (exclusive) after datagram j (an empty datagram repeats the previous value). A caller that frames
 * on the device (sr_frame_slots) gets the route launch's nbytes from here. */
size_t sr_frame_slots_size(const uint8_t *slots, size_t stride, const uint16_t *lens, size_t count,
                           uint32_t *ends);

/* ---- context -------------------------------------------------------------------------------- */
typedef struct sr_ctx sr_ctx;

/* Open a context on HIP device `device` for batches of at most max_batch_bytes framed bytes and
 * n_downstreams shards (the order of the `downstream=` list in statsd-router.conf, sr-init.c:61-121).
 * All downstreams start alive. Allocates device buffers and a HIP stream.
 * Returns 0, -EINVAL, -ENODEV or -ENOMEM. */
int sr_open(sr_ctx **ctx, int device, size_t max_batch_bytes, uint32_t n_downstreams);

/* Snapshot of the health checker's alive bits (sr-health-client.c:15-18,37-40):
 * bit k of alive_bitmap[k/64] = downstream k alive. ceil(n_downstreams/64) words. */
int sr_set_alive(sr_ctx *ctx, const uint64_t *alive_bitmap);

/* Enqueue work on `stream` (a hipStream_t) instead of the context's own stream (NULL restores it). */
int sr_set_stream(sr_ctx *ctx, void *stream);

/* Lane layout of the route kernel. Timing only: the records are identical bit for bit.
 *   SR_LAYOUT_UNIFORM  every line of a tile gets the same lane group, sized by the tile's mean
 *                      line length (best for uniform lengths);
 *   SR_LAYOUT_SEGMENTS a tile of mixed lengths gets one lane per 64-byte name segment, lines packed
 *                      back to back (best when short and long lines share tiles);
 *   SR_LAYOUT_CHUNKS   every lane hashes the 64 bytes it loaded; lines spanning lanes are joined
 *                      by a block scan of partial hashes, lines spanning tiles by a look-back
 *                      (independent of the line lengths; best for mixed lengths);
 *   SR_LAYOUT_AUTO     (default) every 32nd launch outside stream capture (and the first) is a
 *                      segment-layout probe that weighs the traffic; chunks while at least a quarter
 *                      of the tiles of the last probe took the segment layout (back below a tenth),
 *                      uniform otherwise. A graph captured from the context keeps the layout of its
 *                      capture.
 * Returns 0 or -EINVAL. */
#define SR_LAYOUT_AUTO 0
#define SR_LAYOUT_UNIFORM 1
#define SR_LAYOUT_SEGMENTS 2
#define SR_LAYOUT_CHUNKS 3
int sr_set_layout(sr_ctx *ctx, int layout);

/* The layout the last route launch of the context used (SR_LAYOUT_UNIFORM, _SEGMENTS or _CHUNKS;
 * 0 before the first launch), or -EINVAL. */
int sr_last_layout(const sr_ctx *ctx);

/* Where the route kernel of the context's last route launch computed the sdbm name hash. Timing only:
 * the hashes are identical bit for bit.
 *   SR_HASH_VALU    the vector ALU (Horner steps);
 *   SR_HASH_MATRIX  the matrix cores (i8 MFMA limb sums): the uniform and chunk layouts with every
 *                   shard alive, or with two or more shards dead and their probes deferred.
 * 0 before the first launch, or -EINVAL. */
#define SR_HASH_VALU 1
#define SR_HASH_MATRIX 2
int sr_last_hash_engine(const sr_ctx *ctx);

/* Host-memory batch: copy `bytes` (concatenated framed datagrams; the last byte must be '\n'
 * unless nbytes == 0) to the device, classify every line, copy min(n, max_records) records (and,
 * if hashes != NULL, the 64-bit sdbm name hashes; 0 for invalid lines) back, and synchronise.
 * *n_records = number of lines n. Returns 0, or -ENOSPC if n > max_records (the first
 * max_records records are still valid), -EINVAL, -EIO. */
int sr_route_batch(sr_ctx *ctx, const uint8_t *bytes, size_t nbytes, sr_record *out,
                   size_t max_records, size_t *n_records, uint64_t *hashes);

/* The dead-downstream side effect of the last sr_route_batch call: find_downstream zeroes
 * active_buffer_length of every DEAD downstream its probe visits (sr-main.c:106). With the batch's
 * alive snapshot a dead downstream receives no line in that batch, so the caller reproduces the
 * effect exactly by dropping the pending buffer of every downstream whose bit is set here, before
 * it pushes the batch's lines. Writes ceil(n_downstreams/64) words (none when n_downstreams == 0).
 * Returns 0 or -EINVAL. */
int sr_last_probed_dead(const sr_ctx *ctx, uint64_t *bitmap);

/* Device-resident batch (asynchronous, enqueued on the context's stream): d_bytes, d_out,
 * d_hashes (may be NULL) and d_n_records are device pointers. Lines past max_records are counted
 * but not written; the line count is stored to *d_n_records when the work completes.
 * The input buffer needs no padding. Returns 0 or -EINVAL / -EIO (launch failure). */
int sr_route_device(sr_ctx *ctx, const uint8_t *d_bytes, size_t nbytes, sr_record *d_out,
                    size_t max_records, uint64_t *d_hashes, uint64_t *d_n_records);

/* Several device-resident batches in ONE launch (asynchronous, on the context's stream): the
 * batches of several data threads (the reference's threads_num sockets, sr-main.c:237-308) are
 * routed together, each exactly as sr_route_device would route it alone. Up to
 * SR_MAX_BATCHES_PER_LAUNCH batches share a kernel launch; larger counts are split into several
 * launches. Each batch must fit max_batch_bytes. Returns 0 or -EINVAL / -EIO. */
#define SR_MAX_BATCHES_PER_LAUNCH 32u
typedef struct sr_batch {
    const uint8_t *d_bytes;  /* framed datagrams, device memory                         */
    size_t nbytes;
    sr_record *d_out;        /* max_records records, device memory                      */
    size_t max_records;
    uint64_t *d_hashes;      /* NULL or max_records u64, device memory                  */
    uint64_t *d_n_records;   /* device u64: the batch's line count                      */
    uint64_t *d_probed_dead; /* NULL, or max(1, ceil(n_downstreams/64)) device u64: bit k  */
                             /* set iff some line of the batch probed dead downstream k   */
                             /* (find_downstream zeroes its active buffer, sr-main.c:106) */
} sr_batch;
int sr_route_device_many(sr_ctx *ctx, const sr_batch *batches, size_t count);

/* ---- multi-GPU regroup ------------------------------------------------------ */
/* Pack the VALID lines of a routed batch by owner GPU (owner of shard s = s % n_owners), ready for
 * an all-to-all: for owner 0..n_owners-1 in turn, its lines in input order, each starting at a
 * 4-byte aligned position (zero fill in between); d_out_recs gets one record per packed line in
 * the same order, with `offset` relative to the start of its owner's chunk. d_owner_counts
 * receives {lines, bytes} per owner (2*n_owners u64: the all-to-all split sizes). Lines routed
 * to no shard are not packed (their WARN stays with the GPU that received them).
 * d_recs / d_n_records: the output of sr_route_device for the same batch (same stream).
 * out_cap must be >= SR_PACK_CAPACITY(nbytes) (else -EINVAL), and SR_PACK_CAPACITY(nbytes) must fit
 * 32 bits (nbytes up to ~2.8 GB); d_out_recs needs max_records entries.
 * Asynchronous on the context's stream. n_owners in 1..64. Returns 0, -EINVAL, -ENOMEM, -EIO.
 * The first call (or one with a larger max_records / n_owners) allocates scratch: not inside
 * stream capture. */
#define SR_MAX_OWNERS 64u
#define SR_PACK_CAPACITY(nbytes) ((nbytes) + (nbytes) / 2u + 4u)
int sr_pack_by_owner(sr_ctx *ctx, const uint8_t *d_bytes, size_t nbytes, const sr_record *d_recs,
                     const uint64_t *d_n_records, size_t max_records, uint32_t n_owners,
                     uint8_t *d_out_bytes, size_t out_cap, sr_record *d_out_recs,
                     uint64_t *d_owner_counts);

/* sr_pack_by_owner over the batches of one route launch at once (one size exchange per launch):
 * batches[j].d_bytes / nbytes / d_out (its records) / max_records / d_n_records as given to
 * sr_route_device_many. Owner chunks hold batch 0's lines, then batch 1's, ..., each in input
 * order; record offsets are relative to the owner's chunk. out_cap >= SR_PACK_CAPACITY(total
 * bytes) (< 4 GiB), d_out_recs >= sum of max_records. count <= SR_MAX_BATCHES_PER_LAUNCH. */
int sr_pack_many_by_owner(sr_ctx *ctx, const sr_batch *batches, size_t count, uint32_t n_owners,
                          uint8_t *d_out_bytes, size_t out_cap, sr_record *d_out_recs,
                          uint64_t *d_owner_counts);

/* sr_pack_many_by_owner in two calls, so that the rank's own chunk can be written straight into its
 * place in the exchange's receive buffers (no local copy in sr_exchange_data):
 * sr_pack_owner_sizes: the split sizes alone into d_owner_counts (u64 [n_owners][2], as
 *   sr_pack_many_by_owner's), e.g. for sr_exchange_sizes; the context remembers d_owner_counts.
 * sr_pack_owner_scatter: the lines and records of the same batches (the next pack call on the context),
 *   owner `own`'s chunk to d_own_bytes / d_own_recs (its d_owner_counts bytes / lines, offsets relative to
 *   the chunk as always), every other owner's to d_out_bytes / d_out_recs at the usual places (out_cap as
 *   sr_pack_many_by_owner). With own = the comm's rank and d_own_* = d_recv_bytes + recv_byte0 /
 *   d_recv_recs + recv_line0 of peers[rank] (sr_exchange_plan), the following sr_exchange_data on this
 *   context skips the own chunk's copies. d_own_bytes must be 4-byte aligned. own = -1: every chunk to
 *   d_out_bytes / d_out_recs (sr_pack_many_by_owner's output; d_own_* unused). Both asynchronous on the
 *   context's stream. Returns 0, -EINVAL (scatter without sizes, own out of range), -ENOMEM, -EIO.
 * The two calls pair one to one: the scatter uses the tile bases and split sizes of the context's last
 * sizes call, and must be given the same batch descriptors and n_owners (else -EINVAL); a sizes call in
 * between replaces them. */
int sr_pack_owner_sizes(sr_ctx *ctx, const sr_batch *batches, size_t count, uint32_t n_owners,
                        uint64_t *d_owner_counts);
int sr_pack_owner_scatter(sr_ctx *ctx, const sr_batch *batches, size_t count, uint32_t n_owners, int own,
                          uint8_t *d_own_bytes, sr_record *d_own_recs, uint8_t *d_out_bytes, size_t out_cap,
                          sr_record *d_out_recs);

/* ---- multi-GPU exchange of owner packs (RCCL over xGMI, or in process) ----------------------- */
/* One process per GPU; shard s is owned by GPU s % world. After sr_pack_by_owner /
 * sr_pack_many_by_owner (n_owners = world), two collective calls per route launch move every
 * owner's lines to it. RCCL is loaded at sr_comm_open (dlopen of librccl.so.1; a copy already in
 * the process is shared); without it sr_comm_open returns -ENOSYS.
 *
 * sr_comm_id: a fresh communicator id, made by one rank and handed to the others out of band.
 * sr_comm_open: join the communicator as `rank` of `world` on HIP device `device` (collective:
 *   every rank calls it). Returns 0, -EINVAL, -ENOSYS (no RCCL), -EIO. */
#define SR_COMM_ID_BYTES 128u
typedef struct sr_comm sr_comm;
int sr_comm_id(uint8_t id[SR_COMM_ID_BYTES]);
int sr_comm_open(sr_comm **comm, const uint8_t id[SR_COMM_ID_BYTES], int world, int rank, int device);
void sr_comm_close(sr_comm *comm);

/* ---- in-process communicator: ranks as threads of one process, no RCCL ------------------------ */
/* The data threads of one process (the reference's data_pipe_thread's, one per socket, on GPU
 * i % devices) regroup among themselves without RCCL: everything they need is in one address space,
 * and RCCL cannot put two ranks on one GPU. A group is the ranks' meeting place (host only, no GPU);
 * every rank's thread then opens its communicator on it, and that sr_comm works in every call that
 * takes one (sr_exchange_sizes, sr_exchange_data, sr_regroup_launch, sr_exchange_dead, sr_comm_close):
 * the calls run the same sequence as on RCCL, only the five collectives underneath differ.
 *
 * How it moves data: a sender posts {pointer, bytes, an event recorded on its stream}; the receiver
 * makes its stream wait for that event and copies every chunk of the group with ONE kernel on its own
 * stream (a pull), then the sender's stream waits for the pull. Guarantees:
 *   - stream order as on RCCL: a receive is complete in the receiver's stream order where the group
 *     ended, and the sender's later work on its stream is ordered after the peers' reads of its buffers;
 *   - messages between one pair under one tag match in posting order; sizes that differ give -EMSGSIZE
 *     at the receiver and break the group;
 *   - the end of a group BLOCKS THE HOST until every peer this rank has operations with has posted and
 *     pulled (the device work is still asynchronous). So the collectives cannot be captured in a graph:
 *     a capturing stream returns -EINVAL;
 *   - nothing is ever enqueued on the device that waits for something not yet recorded: an absent peer
 *     costs host time only, never a stuck stream.
 * Ranks on different devices need peer access both ways (enabled at open); that path has not been run
 * (DESIGN.md §8).
 *
 * sr_comm_group_open : world in 1..SR_MAX_OWNERS. Returns 0, -EINVAL, -ENOMEM.
 * sr_comm_group_close: 0, -EINVAL, or -EBUSY while a communicator of the group is open.
 * sr_comm_open_local : rank `rank` of the group on HIP device `device`, called once per rank by the
 *   thread that owns the rank; it does not wait for the other ranks and never needs RCCL. Returns 0,
 *   -EINVAL (bad rank or group), -ENODEV (bad device), -EBUSY (rank taken), -ENOTSUP (a peer on another
 *   device without peer access), -ENOMEM. Close with sr_comm_close, before the group.
 * sr_comm_set_timeout: bounds every host wait of a collective on the comm (RCCL comms: the sequence-
 *   word spin of sr_exchange_sizes; local comms also the waits for peers) to `ms` milliseconds; 0, the
 *   default, is no deadline. A wait that runs out returns -ETIMEDOUT and breaks the communicator (a
 *   local comm: its whole group, whose waiting ranks are woken with -EPIPE); every later collective on
 *   a broken communicator returns -EPIPE at once; sr_comm_close still works. sr_exchange_sizes has
 *   one deadline for all of its waits (its all-to-all, then the spin or the stream's drain), `ms`
 *   from the call. A local collective that fails after it posted its sends still orders the caller's
 *   stream after every read of those buffers that a peer had enqueued (none is enqueued once the
 *   group is broken), so they may be reused in stream order. Returns 0 or -EINVAL.
 * sr_comm_transport  : *out = the communicator as an sr_transport (below) bound to ctx's stream, for
 *   sr_exchange_run, sr_regroup_run, sr_exchange_dead_run or sends and receives of the caller's own
 *   (tags 0..2). out->user belongs to the comm and is valid until the next sr_comm_transport on it or
 *   its close. Returns 0 or -EINVAL. */
typedef struct sr_comm_group sr_comm_group;
struct sr_transport;
int sr_comm_group_open(sr_comm_group **g, int world);
int sr_comm_group_close(sr_comm_group *g);
int sr_comm_open_local(sr_comm **comm, sr_comm_group *g, int rank, int device);
int sr_comm_set_timeout(sr_comm *comm, uint32_t ms);
int sr_comm_transport(sr_comm *comm, sr_ctx *ctx, struct sr_transport *out);

/* Collective, on the context's stream: all-to-all of the split sizes d_owner_counts (u64
 * [world][2] {lines, bytes} per owner, the pack's output) into d_recv_counts (u64 [world][2] per
 * source rank; one rank: a device copy, no collective), then both to the host: h_sent / h_received
 * (u64 [world][2]) are valid on return (the launch's one host round trip). One kernel writes them to
 * mapped pinned memory behind a sequence word the host spins on (polling the stream for errors), so the
 * call returns as soon as the sizes land, not when the stream drains: the caller's later work on the
 * context's stream is ordered after them as usual. The spin has no deadline unless sr_comm_set_timeout
 * gave the comm one. Returns 0, -EINVAL, -EIO, -ETIMEDOUT / -EPIPE (sr_comm_set_timeout). */
int sr_exchange_sizes(sr_ctx *ctx, sr_comm *comm, const uint64_t *d_owner_counts, uint64_t *d_recv_counts,
                      uint64_t *h_sent, uint64_t *h_received);

/* Collective, asynchronous on the context's stream: every owner chunk of d_packed / d_packed_recs
 * (the pack's output) goes to its owner; the chunks received from sources 0, 1, ... land back to
 * back in d_recv_bytes (sum of h_received bytes) and d_recv_recs (sum of h_received lines), each
 * record's offset rebased into d_recv_bytes. Per source, every shard's lines keep their input
 * order. h_sent / h_received as sr_exchange_sizes returned them. Returns 0, -EINVAL, -EIO. */
int sr_exchange_data(sr_ctx *ctx, sr_comm *comm, const uint8_t *d_packed, const sr_record *d_packed_recs,
                     const uint64_t *h_sent, const uint64_t *h_received, uint8_t *d_recv_bytes,
                     sr_record *d_recv_recs);

/* The plan of one exchange (host only, no GPU): what sr_exchange_data moves to and from each peer.
 * For peer q, the pack's records [send_line0, send_line0 + send_lines) and bytes [send_byte0, +send_bytes)
 * go to q; q's chunk lands at records [recv_line0, +recv_lines) and bytes [recv_byte0, +recv_bytes) of
 * the receive buffers, and its records' offsets move by recv_byte0 (the rebase). peers[rank] is the
 * rank's own chunk: a local copy, not a send. The reference analogue is the SO_REUSEPORT split of
 * datagrams over data threads (sr-main.c:253-271,363-367); the plan is what regroups them by owner. */
typedef struct sr_exchange_peer {
    uint64_t send_line0, send_lines, send_byte0, send_bytes;
    uint64_t recv_line0, recv_lines, recv_byte0, recv_bytes;
} sr_exchange_peer;

/* Fill peers[world] from the split sizes (u64 [world][2] {lines, bytes}, as sr_exchange_sizes returns
 * them) and totals[4] = {lines sent, bytes sent, lines received, bytes received} (totals may be NULL).
 * Returns 0, or -EINVAL: bad world/rank, the own chunk's sent and received sizes differ, or a received
 * total does not fit the u32 record offsets. */
int sr_exchange_plan(int world, int rank, const uint64_t *h_sent, const uint64_t *h_received,
                     sr_exchange_peer *peers, uint64_t *totals);

/* The transport an exchange runs on. sr_exchange_data uses the communicator's own (sr_comm_transport;
 * RCCL: ncclSend/ncclRecv in one group, the
 * own chunk by hipMemcpyAsync, the rebase by a kernel, all on the context's stream); a host that moves
 * the chunks another way (tests: torch.distributed gloo over host memory) supplies its own. Every
 * callback returns 0 or a negative errno. tag 0 = line bytes, 1 = records, 2 = a probed-dead bitmap row
 * (sr_exchange_dead_run) (a send of `bytes` bytes to
 * `peer` matches that peer's recv of the same tag from this rank). rebase: add peers[p].recv_byte0 to
 * the offset of records [recv_line0, +recv_lines) of every source p. */
typedef struct sr_transport {
    void *user;
    int (*group_start)(void *user);
    int (*group_end)(void *user);
    int (*send)(void *user, const void *buf, size_t bytes, int peer, int tag);
    int (*recv)(void *user, void *buf, size_t bytes, int peer, int tag);
    int (*copy)(void *user, void *dst, const void *src, size_t bytes);
    int (*rebase)(void *user, sr_record *recs, const sr_exchange_peer *peers, int world, uint64_t n_lines);
} sr_transport;

/* One exchange on a caller-supplied transport: sr_exchange_plan, then within one group_start/group_end
 * the sends and receives of every peer q != rank in rank order (bytes, then records; zero-sized ones
 * skipped), then the own chunk's copies, then one rebase of all received records. Buffers are whatever
 * the transport addresses (device memory for RCCL). Returns 0, -EINVAL or the first callback error. */
int sr_exchange_run(const sr_transport *t, int world, int rank, const uint64_t *h_sent,
                    const uint64_t *h_received, const uint8_t *packed, const sr_record *packed_recs,
                    uint8_t *recv_bytes, sr_record *recv_recs);

/* One route launch's whole regroup in one call, for the host loop that runs it every launch:
 * sr_pack_owner_sizes (n_owners = the comm's world), sr_exchange_sizes (the one host round trip),
 * sr_exchange_plan, then sr_pack_owner_scatter with the rank's own chunk written into its place in the
 * receive buffers and sr_exchange_data. Only the host work between the sizes arriving and the scatter's
 * launch stays on the critical path (no interpreter in between). h_sent / h_received (u64 [world][2])
 * hold the split sizes on return, also when the receive buffers are too small: then nothing is
 * scattered or sent and -ENOSPC is returned; the caller allocates the sizes' totals (sr_exchange_plan)
 * and finishes with sr_pack_owner_scatter and sr_exchange_data as above. packed_cap / d_packed_recs as
 * sr_pack_many_by_owner's out_cap / d_out_recs; recv_bytes_cap / recv_recs_cap in bytes / records.
 * Returns 0, -ENOSPC, -EINVAL, -ENOMEM, -EIO. Collective: every rank of the comm calls it. */
int sr_regroup_launch(sr_ctx *ctx, sr_comm *comm, const sr_batch *batches, size_t count,
                      uint64_t *d_owner_counts, uint64_t *d_recv_counts, uint8_t *d_packed, size_t packed_cap,
                      sr_record *d_packed_recs, uint8_t *d_recv_bytes, size_t recv_bytes_cap,
                      sr_record *d_recv_recs, size_t recv_recs_cap, uint64_t *h_sent, uint64_t *h_received);

/* sr_regroup_launch on any transport: the same sequence (split sizes, size exchange, plan, scatter with
 * the own chunk in place, exchange without the own chunk's copy, rebase) with `sizes` in place of
 * sr_exchange_sizes and `t` in place of RCCL; sr_regroup_launch is this call on RCCL. `sizes` gets t->user
 * and must leave h_sent / h_received (u64 [world][2]) valid and d_recv_counts written (ordered before
 * the context's later work) when it returns; it is collective like the transport. The device work of the
 * call is enqueued on the context's stream and not waited for: a transport that reads or writes device
 * buffers from the host first waits for that stream (sr_sync). Used to run the multi-rank sequence
 * without RCCL (ranks as threads on one GPU, or processes over gloo). Returns as sr_regroup_launch; after
 * -ENOSPC (the sizes exchanged, nothing scattered or sent: the peers' sends to this rank stay posted)
 * the caller finishes with sr_pack_owner_scatter (own = -1) and sr_exchange_run on the same transport. */
typedef int (*sr_sizes_fn)(void *user, const uint64_t *d_owner_counts, uint64_t *d_recv_counts, uint64_t *h_sent,
                           uint64_t *h_received);
int sr_regroup_run(sr_ctx *ctx, const sr_transport *t, sr_sizes_fn sizes, int world, int rank,
                   const sr_batch *batches, size_t count, uint64_t *d_owner_counts, uint64_t *d_recv_counts,
                   uint8_t *d_packed, size_t packed_cap, sr_record *d_packed_recs, uint8_t *d_recv_bytes,
                   size_t recv_bytes_cap, sr_record *d_recv_recs, size_t recv_recs_cap, uint64_t *h_sent,
                   uint64_t *h_received);

/* The rebase of sr_exchange_data alone (asynchronous on the context's stream): records
 * [peers[p].recv_line0, +recv_lines) of d_recv_recs move by peers[p].recv_byte0, p = 0..world-1.
 * world <= SR_MAX_OWNERS; the sources' record ranges must be back to back from 0. Returns 0, -EINVAL, -EIO. */
int sr_exchange_rebase(sr_ctx *ctx, sr_record *d_recv_recs, const sr_exchange_peer *peers, int world);

/* ---- per-downstream MTU packing ------------------------------------------ */
/* push_to_downstream (sr-main.c:73-83) appends each routed line to its downstream's active buffer,
 * flushing the buffer first when the line would not fit in DOWNSTREAM_BUF_SIZE (1450) bytes
 * (ds_schedule_flush, sr-main.c:49-71): per downstream a greedy packing of its lines in arrival
 * order, starting from the bytes already pending. sr_pack_packets computes it on the device.
 *
 * Records are first regrouped stably ("sorted"): the valid lines of downstream 0, 1, ..., N-1 in
 * arrival order, then every unrouted line (invalid length / format, all dead) in input order.
 * A packet is a run of consecutive sorted lines, led by `carry` bytes of the downstream's buffer
 * pending before the batch (only a downstream's first packet of the batch can have carry > 0).
 * Per downstream with lines in the batch: every packet the batch flushes (open = 0), in order,
 * then its new pending buffer (open = 1, last). Downstreams without lines get no descriptor; their
 * pending bytes carry over unchanged, except those probed dead, which are dropped (sr-main.c:106). */
typedef struct sr_packet {
    uint32_t first;   /* index in the sorted records of the packet's first line of this batch */
    uint16_t nlines;  /* lines of this batch in the packet                                   */
    uint16_t shard;   /* downstream                                                          */
    uint16_t length;  /* bytes of those lines                                                */
    uint16_t carry;   /* pending bytes from before the batch that lead the packet            */
    uint32_t open;    /* 1: the downstream's pending buffer after the batch (not flushed)    */
} sr_packet;

#define SR_MAX_PACK_DOWNSTREAMS 4096u
/* Descriptor room that always suffices (two consecutive flushed packets hold > 1450 bytes). */
#define SR_MAX_PACKETS(nbytes, n_downstreams) \
    (2u * (uint64_t)(nbytes) / SR_DOWNSTREAM_BUF_SIZE + 5u * (uint64_t)(n_downstreams) + 4u)

/* Device-resident packing of a routed batch (asynchronous on the context's stream):
 *   d_recs, d_n_records, max_records: the output of sr_route_device(_many) for the batch;
 *   d_fill_in  : NULL (nothing pending) or n_downstreams u16, pending bytes per downstream (<= 1450);
 *   d_probed_dead: NULL or the batch's probed-dead bitmap (sr_batch.d_probed_dead);
 *   d_sorted   : max_records records; d_packets: max_packets descriptors;
 *   d_counts   : 3 u64 = {descriptors, valid lines, lines} (descriptors past max_packets are not
 *                written: check d_counts[0] <= max_packets);
 *   d_fill_out : n_downstreams u16, pending bytes after the batch (may alias d_fill_in only if the
 *                caller does not need d_fill_in afterwards).
 * n_downstreams <= SR_MAX_PACK_DOWNSTREAMS. The first call (or one with a larger max_records)
 * allocates scratch: not inside stream capture. Returns 0, -EINVAL, -ENOMEM, -EIO. */
int sr_pack_packets(sr_ctx *ctx, const sr_record *d_recs, const uint64_t *d_n_records, size_t max_records,
                    const uint16_t *d_fill_in, const uint64_t *d_probed_dead, sr_record *d_sorted,
                    sr_packet *d_packets, size_t max_packets, uint64_t *d_counts, uint16_t *d_fill_out);

/* Several batches packed in one set of launches (the batches of several data threads, each with
 * its own pending bytes: batches are independent). Fields as in sr_pack_packets. count <=
 * SR_MAX_BATCHES_PER_LAUNCH. Same allocation rule as sr_pack_packets. */
typedef struct sr_pack_batch {
    const sr_record *d_recs;         /* routed records and their count (sr_route_device(_many))   */
    const uint64_t *d_n_records;
    size_t max_records;
    const uint16_t *d_fill_in;       /* NULL or n_downstreams u16                                 */
    const uint64_t *d_probed_dead;   /* NULL or the batch's probed-dead bitmap                    */
    sr_record *d_sorted;
    sr_packet *d_packets;
    size_t max_packets;
    uint64_t *d_counts;              /* 3 u64: {descriptors, valid lines, lines}                  */
    uint16_t *d_fill_out;
} sr_pack_batch;
int sr_pack_packets_many(sr_ctx *ctx, const sr_pack_batch *batches, size_t count);

/* Route and pack device-resident batches in one call: sr_route_device_many over `route` (one launch)
 * followed by sr_pack_packets_many over `pack`, whose batch i must read what route batch i writes
 * (pack[i].d_recs == route[i].d_out, same d_n_records, max_records and d_probed_dead; -EINVAL
 * otherwise). Identical outputs; with every shard alive and at most 16 downstreams the route kernel
 * also hands each 16 KiB tile's per-downstream line counts to the packing, which then sorts the
 * records without a counting pass of its own over them. count <= SR_MAX_BATCHES_PER_LAUNCH. */
int sr_route_pack_many(sr_ctx *ctx, const sr_batch *route, const sr_pack_batch *pack, size_t count);

/* Host-memory batch, routed and packed in one call (what a data thread's read callback needs):
 * `fill` (n_downstreams u16) is the pending bytes per downstream before the batch and receives the
 * pending bytes after it; `sorted` (max_records) the regrouped records; `packets` (max_packets) the
 * descriptors; probed_dead (ceil(n/64) words, may be NULL) the dead downstreams whose pending
 * buffer the batch drops. Synchronous: one stream synchronisation (sr_route_pack_submit /
 * sr_route_pack_result on a slot of its own). Returns 0, -ENOSPC (records or descriptors did not
 * fit: outputs incomplete), -EINVAL, -ENOMEM, -EIO. */
int sr_route_pack_batch(sr_ctx *ctx, const uint8_t *bytes, size_t nbytes, uint16_t *fill, sr_record *sorted,
                        size_t max_records, size_t *n_records, size_t *n_valid, sr_packet *packets,
                        size_t max_packets, size_t *n_packets, uint64_t *probed_dead);

/* sr_route_pack_batch in two halves, for a data thread that overlaps a batch's GPU work with its own
 * work on the previous batch (double buffering; reference: udp_read_cb, sr-main.c:149-191).
 * sr_route_pack_submit enqueues on the context's stream the copy of `bytes` to the device, the route,
 * the packing and one copy-out kernel that writes the batch's outputs (counts included) into
 * page-locked memory the context owns for slot `slot` (0 or 1), and returns without waiting.
 * fill: the pending bytes per downstream before the batch, or NULL to continue from the pending
 * bytes the previous submission (of either slot, or sr_route_pack_batch) leaves on the device, all
 * zero before the first: consecutive batches chain without a host round trip. `bytes` must stay
 * unchanged until the slot's result is taken. sr_route_pack_result waits for the slot (its one
 * synchronisation) and points *res at its outputs, valid until the slot is submitted again.
 * A slot holds one batch at a time. Returns 0, -EBUSY (slot in use / not submitted), -ENOSPC
 * (result: records or descriptors did not fit), -EINVAL, -ENOMEM, -EIO. */
typedef struct sr_pack_result {
    const sr_record *sorted;      /* n_records: valid lines by downstream, then the unrouted lines */
    size_t n_records, n_valid;
    const sr_packet *packets;     /* n_packets descriptors (sr_pack_packets)                       */
    size_t n_packets;
    const uint16_t *fill;         /* n_downstreams: pending bytes after the batch                  */
    const uint64_t *probed_dead;  /* ceil(n_downstreams/64) words (sr-main.c:106)                  */
} sr_pack_result;
int sr_route_pack_submit(sr_ctx *ctx, int slot, const uint8_t *bytes, size_t nbytes, const uint16_t *fill);
int sr_route_pack_result(sr_ctx *ctx, int slot, sr_pack_result *res);

/* TRACE logging (log_level 0, the reference's default: sr-init.c:252). The reference logs, per line
 * that reaches find_downstream, its sdbm hash and its first live pick (sr-main.c:91,102), so a router
 * at that level needs every line's verdict, hash and shard in INPUT order. With sr_set_trace(ctx, 1)
 * every later sr_route_pack_submit / sr_route_pack_batch also has the route kernel write each line's
 * hash (0 for lines that fail the length or ':' test) and the copy-out kernel return the records in
 * input order with the hashes; sr_route_pack_trace points at them after sr_route_pack_result(slot),
 * valid until the slot is submitted again (slot 2: the last sr_route_pack_batch). Off by default: it
 * costs 16 bytes per line of PCIe and host memory. Returns 0, -EINVAL, -EBUSY (not traced). */
int sr_set_trace(sr_ctx *ctx, int on);
int sr_route_pack_trace(sr_ctx *ctx, int slot, const sr_record **records, const uint64_t **hashes,
                        size_t *n_records);

/* ---- packet payloads (wire format) ----------------------------------------------------------- */
/* sr_pack_packets describes the packets; sr_pack_payloads gathers their bytes on the device, as
 * ds_flush_cb sends them (sr-main.c:21-46): per descriptor its `carry` pending bytes followed by its
 * `nlines` lines with no padding, the packets back to back in one arena.
 *   d_offsets[i] = exclusive prefix sum of carry + length over the batch's n = min(d_counts[0],
 *                  max_packets) descriptors, d_offsets[n] = *d_total = the arena bytes needed;
 *   d_payload    : bytes [d_offsets[i], d_offsets[i+1]) are packet i (flushed and open packets alike).
 *                  Nothing at or past min(total, payload_cap) is written: *d_total > payload_cap or
 *                  d_counts[0] > max_packets tells the caller that the arena is incomplete.
 *                  SR_PAYLOAD_CAPACITY always suffices;
 *   d_pend_in    : the pending bytes before the batch, slot s at d_pend_in + s * SR_PENDING_STRIDE. NULL:
 *                  the first `carry` bytes of a packet are left unwritten (room for a caller that holds
 *                  the pending bytes on the host and copies them in itself);
 *   d_pend_out   : NULL, or the pending bytes after the batch in the same layout: slot s receives the
 *                  bytes of downstream s's open packet, or, when s has no descriptor, the first
 *                  d_fill_out[s] bytes of d_pend_in's slot (none when s was probed dead). Bytes of a slot
 *                  at or past d_fill_out[s] are not written. Needs d_pend_in and must not be d_pend_in:
 *                  a flushed packet reads the slot its downstream's open packet writes, so consecutive
 *                  batches alternate between two buffers.
 * Asynchronous on the context's stream, after the packing of the same batches; no scratch, so the calls
 * can be captured in a graph. count in 1..SR_MAX_BATCHES_PER_LAUNCH. Returns 0, -EINVAL (a null
 * required pointer, d_pend_out without d_pend_in or equal to it, count out of range), -ENOMEM, -EIO. */
#define SR_PENDING_STRIDE 1456u   /* one downstream's pending slot: 1450 rounded up to 16 */
#define SR_PAYLOAD_CAPACITY(nbytes, n_downstreams) \
    ((uint64_t)(nbytes) + (uint64_t)SR_DOWNSTREAM_BUF_SIZE * (n_downstreams))

typedef struct sr_payload_batch {
    const uint8_t *d_bytes;  size_t nbytes;        /* the routed batch                               */
    const sr_record *d_sorted; size_t max_records; /* sr_pack_batch.d_sorted / max_records           */
    const sr_packet *d_packets; size_t max_packets;
    const uint64_t *d_counts;                      /* sr_pack_batch.d_counts                         */
    const uint16_t *d_fill_out;                    /* sr_pack_batch.d_fill_out                       */
    const uint8_t *d_pend_in;                      /* NULL (room left for the carry) or n * STRIDE   */
    uint8_t *d_pend_out;                           /* NULL or n * STRIDE; needs d_pend_in; != it     */
    uint8_t *d_payload;  size_t payload_cap;
    uint32_t *d_offsets;                           /* max_packets + 1                                */
    uint64_t *d_total;                             /* bytes needed                                   */
} sr_payload_batch;
int sr_pack_payloads_many(sr_ctx *ctx, const sr_payload_batch *batches, size_t count);
int sr_pack_payloads(sr_ctx *ctx, const sr_payload_batch *batch);   /* count = 1 */

/* The payloads of the host-memory path. With sr_set_payloads(ctx, 1) every later sr_route_pack_submit /
 * sr_route_pack_batch also gathers the batch's packets (d_pend_in = NULL: the host holds the pending
 * bytes, so each packet's first `carry` bytes are room) into page-locked memory of the slot;
 * sr_route_pack_payloads points at the arena and its n_packets + 1 offsets after
 * sr_route_pack_result(slot), valid until the slot is submitted again (slot 2: the last
 * sr_route_pack_batch). Off by default: the slot's device-to-host bytes grow from 8 per line to 8 plus the
 * line. Returns 0, -EINVAL, -EBUSY (the slot is in flight or was submitted with the switch off). */
int sr_set_payloads(sr_ctx *ctx, int on);
int sr_route_pack_payloads(sr_ctx *ctx, int slot, const uint8_t **payload, const uint32_t **offsets,
                           size_t *n_packets);

/* ---- framing on the device: datagrams straight from their recvmmsg slots ------------------------ */
/* recvmmsg leaves a strided array of slots and a length per slot. sr_frame_slots frames them on the device
 * exactly as sr_frame_datagrams does on the host (udp_read_cb, sr-main.c:163-173): for each j in order the
 * first n = min(lens[j], SR_MAX_DATAGRAM) bytes of slot j, then one '\n' when n > 0 and byte n - 1 is not
 * one; nothing for n = 0.
 *   d_slots / d_lens: device-readable memory (device memory, or page-locked host memory by its device
 *                     address); datagram j at d_slots + j * stride;
 *   d_bytes / cap   : the framed batch. Nothing at or past min(total, cap) is written;
 *   d_ends          : NULL, or count u32: the framed end offset (exclusive) after datagram j;
 *   d_total         : the framed bytes needed (= d_ends[count - 1]); it may exceed cap.
 * Asynchronous on the context's stream. The first call with count > 0 allocates the context's scan scratch,
 * once and at its full size (not inside stream capture); later calls allocate nothing and can be captured
 * in a graph. count == 0 writes *d_total = 0 and nothing else. Returns 0, -EINVAL (a null context or
 * required pointer, stride < SR_DATA_BUF_SIZE or > SR_MAX_SLOT_STRIDE, count > SR_MAX_SLOTS), -ENOMEM, -EIO. */
#define SR_MAX_SLOTS 65536u
#define SR_MAX_SLOT_STRIDE 134217728u   /* 128 MiB: offsets inside a gather run stay below 2^31 */
typedef struct sr_slot_batch {
    const uint8_t *d_slots; size_t stride;   /* stride >= SR_DATA_BUF_SIZE; any byte alignment */
    const uint16_t *d_lens; size_t count;    /* count <= SR_MAX_SLOTS; values above 4095 are capped */
    uint8_t *d_bytes; size_t cap;            /* framed batch out */
    uint32_t *d_ends;                        /* NULL or count entries */
    uint64_t *d_total;                       /* framed bytes needed (may exceed cap) */
} sr_slot_batch;
int sr_frame_slots(sr_ctx *ctx, const sr_slot_batch *b);

/* sr_route_pack_submit with the framing on the device instead of a host-to-device copy of a framed batch:
 * `slots` is page-locked host memory that the device can read (sr_alloc_host), datagram j at slots +
 * j * stride, lens[j] bytes long. The function asks for the memory's device address and returns -EINVAL
 * when it has none. lens is copied into the slot's staging and is free on return; the datagrams must stay
 * unchanged until the slot's result is taken. The framed size comes from sr_frame_slots_size; -EINVAL when
 * it exceeds max_batch_bytes; 0 (no datagrams, or only empty ones) behaves as sr_route_pack_submit(NULL, 0).
 * The frame kernels read the slots in place and write the context's input buffer; route, packing, copy-out
 * and the optional trace and payloads follow unchanged, and record offsets refer to the framed stream.
 * sr_route_pack_result returns -EIO when the device's framed total differs from the host's, i.e. the
 * caller changed the slots while the batch was in flight. Other returns as sr_route_pack_submit. */
int sr_route_pack_submit_slots(sr_ctx *ctx, int slot, const uint8_t *slots, size_t stride,
                               const uint16_t *lens, size_t count, const uint16_t *fill);

/* ---- log text on the device ------------------------------------------------------------------------ */
/* At log_level TRACE (the reference's default, sr-init.c:252) udp_read_cb writes more log text than it routes:
 * "got packet" per datagram (sr-main.c:174) and two find_downstream messages per valid line (:91,102), next to
 * the WARN messages of the lines it drops (:115,142,184). sr_format_log writes a routed batch's messages on
 * the device, in the reference's order and bytes, back to back into one arena: datagrams in order, inside each
 * its lines in order, and per line
 *   TRACE "udp_read_cb: got packet " + the datagram's framed bytes, when the line starts a datagram: its offset
 *         is the end before d_ends[g] and d_ends[g] is greater (an empty datagram gets none; lines at or after
 *         the last end, or all lines with d_ends == NULL, get none);
 *   then  route SR_ROUTE_INVALID_LENGTH: WARN "udp_read_cb: invalid length %d of metric " + the line, '\n' included;
 *         route SR_ROUTE_INVALID_FORMAT: WARN "process_data_line: invalid metric " + the line without its '\n';
 *         any other route: TRACE "find_downstream: hash = %lx, length = %d, line = " + the line, '\n' included,
 *         followed by TRACE "find_downstream: pushing to downstream %d" when route < n_downstreams (the
 *         context's), else WARN "find_downstream: all downstreams are dead".
 * A run of input bytes is printed as "%.*s" prints it: it stops before its first NUL byte. With min_level =
 * 3 (WARN) only the WARN messages are written, in the same order, and d_hashes may be NULL.
 * On the wire a message is prefix[level] + text + '\n': d_prefix holds prefix_len[0] bytes for TRACE followed
 * by prefix_len[1] bytes for WARN (each at most SR_LOG_MAX_PREFIX). max_msg > 0 cuts prefix + text to max_msg
 * bytes before the '\n' (2047: log_msg's 2048-byte buffer, sr-util.c:14-27); it must exceed both prefix
 * lengths.
 *   d_text / text_cap : the messages. Nothing at or past min(*d_total, text_cap) is written;
 *   d_total           : the bytes needed; the text is complete iff *d_total <= text_cap;
 *   d_n_msgs          : the messages; the index is complete iff *d_n_msgs <= max_msgs;
 *   d_offsets         : NULL, or max_msgs + 1 u32: entry i < min(n, max_msgs) is the first byte of message i,
 *                       entry min(n, max_msgs) the end of the last indexed message (the total when the index
 *                       is complete); later entries are not written. Entries are 32-bit: an index serves
 *                       texts below 4 GiB (the totals are 64-bit);
 *   d_levels          : NULL, or max_msgs u8: 0 (TRACE) or 3 (WARN) per indexed message.
 * Only min(*d_n_records, max_records, nbytes) records are read (a line has at least one byte, so a real
 * record count never exceeds nbytes; the third bound keeps the grid finite for a wrong one); every byte read
 * lies inside [0, nbytes) whatever the records say. nbytes <= max_batch_bytes and <= 2^30. Inputs and outputs may sit at any byte alignment
 * (d_recs, d_hashes, d_ends, d_offsets, d_total, d_n_msgs at their types').
 * Asynchronous on the context's stream. The first call allocates the context's scan scratch, once and at its
 * full size (not inside stream capture); later calls allocate nothing and can be captured in a graph.
 * Returns 0, -EINVAL, -ENOMEM, -EIO.
 *
 * Room that always suffices for a framed batch and its own records:
 *   SR_LOG_MAX_MSGS: a line yields one message, or two when it passes the length gate (>= 6 bytes), so at most
 *     one per byte; plus one "got packet" per datagram.
 *   SR_LOG_TEXT_CAPACITY: with P = the longer prefix, a line of L bytes costs at most L * (P + 42) bytes: a
 *     one-byte line is P + "udp_read_cb: invalid length 1 of metric " (40) + the byte + '\n' = P + 42; 2..5
 *     bytes: P + 40 + L + 1; an invalid length of 1450 or more: P + 44 + L + 1; an invalid metric (L >= 6):
 *     P + 34 + L; a routed line (L >= 6): at most P + 64 + L + 1 with a 16-digit hash and a 4-digit length,
 *     then at most P + 45 ("pushing to downstream 65532" + '\n'), together 2 P + 110 + L <= L (P + 42). A datagram costs
 *     P + 24 + its bytes + 1. The lines' bytes and the datagrams' bytes are each at most nbytes. */
#define SR_LOG_MAX_PREFIX 256u
#define SR_LOG_MAX_MSGS(nbytes, n_datagrams) ((uint64_t)(nbytes) + (uint64_t)(n_datagrams))
#define SR_LOG_TEXT_CAPACITY(nbytes, n_datagrams, prefix_max) \
    ((uint64_t)(nbytes) * ((uint64_t)(prefix_max) + 43u) + (uint64_t)(n_datagrams) * ((uint64_t)(prefix_max) + 25u))

typedef struct sr_log_batch {
    const uint8_t *d_bytes; size_t nbytes;            /* the routed batch                                  */
    const sr_record *d_recs; const uint64_t *d_n_records; size_t max_records;   /* input order            */
    const uint64_t *d_hashes;                         /* NULL allowed only with min_level > 0 (TRACE)      */
    const uint32_t *d_ends; size_t n_datagrams;       /* framed datagram ends; NULL / 0: no "got packet"   */
    int min_level;                                    /* 0 (TRACE) or 3 (WARN)                             */
    const uint8_t *d_prefix; uint32_t prefix_len[2];  /* TRACE bytes, then WARN bytes                      */
    uint32_t max_msg;                                 /* 0: no cut                                         */
    uint8_t *d_text; size_t text_cap;
    uint32_t *d_offsets; uint8_t *d_levels; size_t max_msgs;   /* both optional                           */
    uint64_t *d_total; uint64_t *d_n_msgs;
} sr_log_batch;
int sr_format_log(sr_ctx *ctx, const sr_log_batch *b);

/* The log text of the host-memory path. With sr_set_logtext(ctx, min_level, text_cap, max_msg), min_level 0
 * (TRACE) or 3 (WARN), every later sr_route_pack_submit / sr_route_pack_submit_slots / sr_route_pack_batch also
 * formats the batch's log (sr_format_log over the batch's input-order records) into page-locked memory of the
 * slot; a negative min_level turns the switch off (the default). The arena is sized once: text_cap bytes
 * (0: SR_LOG_DEFAULT_TEXT_CAP(max_batch_bytes)) and an index with room for every message of a text that fits
 * it. At TRACE the route kernel also writes the hashes, as with sr_set_trace (whose outputs stay available next
 * to the text when it is on). Returns 0, -EINVAL (max_batch_bytes above 2^30), -EBUSY (a slot is in flight).
 *
 * sr_route_pack_set_prefix / sr_route_pack_set_ends stage, for the slot's NEXT submission only, the two prefixes
 * (each at most SR_LOG_MAX_PREFIX bytes; none staged: empty) and the framed datagram ends of a
 * sr_route_pack_submit / sr_route_pack_batch (slot 2) batch (n <= SR_MAX_SLOTS; none staged: no "got packet").
 * Both are copied and are free for reuse on return. sr_route_pack_submit_slots takes its ends from the frame
 * kernels instead. A max_msg that does not exceed both staged prefix lengths makes the submission return
 * -EINVAL. Return 0, -EINVAL (switch off, bad slot or lengths), -EBUSY (the slot is in flight), -ENOMEM.
 *
 * sr_route_pack_logtext points at the slot's text, its total (the bytes needed), the offsets (*n_msgs + 1) and
 * the levels (*n_msgs = the messages indexed) after sr_route_pack_result(slot), valid until the slot is
 * submitted again (slot 2: the last sr_route_pack_batch). Returns 0 when text and index are complete, -ENOSPC
 * when either did not fit (the caller formats that batch itself: nothing else is lost), -EINVAL, -EBUSY (the
 * slot is in flight or was submitted with the switch off). */
#define SR_LOG_DEFAULT_TEXT_CAP(max_batch_bytes) ((uint64_t)(max_batch_bytes) * 8u + 65536u)
int sr_set_logtext(sr_ctx *ctx, int min_level_or_off, size_t text_cap, uint32_t max_msg);
int sr_route_pack_set_prefix(sr_ctx *ctx, int slot, const uint8_t *trace, size_t tlen, const uint8_t *warn,
                             size_t wlen);
int sr_route_pack_set_ends(sr_ctx *ctx, int slot, const uint32_t *ends, size_t n);
int sr_route_pack_logtext(sr_ctx *ctx, int slot, const uint8_t **text, uint64_t *total, const uint32_t **offsets,
                          const uint8_t **levels, size_t *n_msgs);

/* ---- name statistics on the device: hot names and distinct names per shard ---------------------------- */
/* The shard of a line is a pure function of its name, so one hot name is one overloaded downstream. This stage
 * consumes what the route launch leaves on the device (the input-order records and the 64-bit name hashes) and
 * keeps, per context, sketches that answer "which names carry the traffic" and "how many distinct names does
 * shard k hold". Everything is exact and deterministic (tests/stats_expect.py restates it in numpy).
 *
 * State, from sr_stats_open or the last sr_stats_reset:
 *   lines[4], bytes[4]        per verdict (sr_record_verdict): the records seen and the sum of their `length`;
 *   ignored                   records whose route is neither below n_downstreams nor an SR_ROUTE_* code; they
 *                             touch nothing else;
 *   shard_lines[n], shard_bytes[n]   the same sums per shard over the valid lines; total = lines[SR_VALID].
 * Per valid record with name hash h, m = fmix64(h) (the MurmurHash3 finaliser: m ^= m >> 33; m *=
 * 0xff51afd7ed558ccd; m ^= m >> 33; m *= 0xc4ceb9fe1a85ec53; m ^= m >> 33):
 *   distinct names (HyperLogLog, 2^p u8 registers per shard): idx = m >> (64 - p), w = m << p,
 *     rho = w == 0 ? 64 - p + 1 : clz64(w) + 1, reg[shard][idx] = max(reg, rho);
 *   lines per name (count-min sketch, D rows of W u64 cells, one per context): a = (u32)m, b = (u32)(m >> 32) | 1,
 *     row r adds 1 to cell (a + r * b) & (W - 1) (32-bit wrapping); est(h) = the minimum over the rows. It never
 *     underestimates; overestimates (colliding cells) are part of the contract;
 *   hot names, settled after every record of the call is counted: T = max(hot_min_lines, ceil(total / hot_div));
 *     every valid record of this call with est(h) >= T puts its name into the hot table (hot_slots entries)
 *     unless it is there; a name stays until reset; one that finds no room sets hot_overflow. Equal hashes are
 *     equal names: which line supplies the bytes is not specified.
 * The name is the line's bytes before its first ':' inside the line clipped to [0, nbytes) (a record without a
 * ':' there: the whole clipped run); name_len is its full length, the first min(name_len, SR_STATS_NAME_MAX)
 * bytes are stored, the rest of `name` is zero. Only min(*d_n_records, max_records) records of a batch are
 * read, and no byte outside [0, nbytes).
 *
 * sr_stats_config: all six zero selects the defaults below. Limits: hll_p in SR_STATS_MIN_P..SR_STATS_MAX_P
 *   with n_downstreams << hll_p at most SR_STATS_MAX_REGS; cms_rows in 1..SR_STATS_MAX_ROWS; cms_width a power
 *   of two, at least SR_STATS_MIN_WIDTH, with cms_rows * cms_width <= SR_STATS_MAX_CELLS (a workgroup keeps the
 *   whole sketch in LDS as u32: 64 KiB); hot_slots a power of two in SR_STATS_MIN_SLOTS..SR_STATS_MAX_SLOTS;
 *   hot_div >= 1.
 * sr_stats_open  : allocates everything, once (not inside stream capture). 0, -EINVAL, -ENOMEM, -EBUSY (open).
 * sr_stats_update: the batches of one route launch (count in 1..SR_MAX_BATCHES_PER_LAUNCH), asynchronous on the
 *   context's stream; it allocates nothing, so it can be captured in a graph. d_hashes as the route launch
 *   wrote them (sr_batch.d_hashes). -EINVAL before any launch for a null required pointer (d_n_records; d_recs
 *   and d_hashes with max_records > 0; d_bytes with nbytes > 0), d_hashes == NULL, a bad count or a context
 *   that is not open; nbytes and max_records at most 0xFFFFFFF0.
 * sr_stats_reset : back to the state after open, asynchronous.
 * sr_stats_read  : synchronises the stream and returns a host snapshot (sr_stats_free). Hot entries carry
 *   lines = est(hash) from this snapshot and are sorted by lines descending, then hash ascending.
 * sr_stats_close : waits for the stream and frees the stage, switch included (sr_close does it too); the stage
 *   can then be opened again with another configuration. 0, -EINVAL, -EBUSY (a slot is in flight).
 *
 * Host only (no GPU; on any snapshot, also one a caller assembled itself: the arrays have the sizes noted in
 * the structure, `hot` has room for cfg.hot_slots entries):
 *   sr_name_hash        : the reference's sdbm over `len` bytes with signed `char` (sr-main.c:120-134);
 *   sr_stats_estimate   : est(hash);
 *   sr_stats_cardinality: the distinct names of `shard`, or of all shards together (SR_STATS_ALL: register-wise
 *     maximum). The standard estimator: alpha_m * m^2 / sum(2^-reg), m = 2^p; linear counting m * ln(m / V)
 *     when that is at most 2.5 m and V > 0 registers are zero; alpha = 0.673 / 0.697 / 0.709 for m = 16 / 32 /
 *     64, else 0.7213 / (1 + 1.079 / m); no large-range correction. A negative value: bad arguments;
 *   sr_stats_merge      : `from` added into `into` (same config and n_downstreams, else -EINVAL): counters and
 *     cells add, registers take the maximum, the hot entries are united, estimated again and sorted again;
 *     hot_overflow is set when either had it or the union does not fit. This is what lets several data
 *     threads or GPUs give one answer. */
#define SR_STATS_NAME_MAX   108u      /* name bytes kept per hot entry: an entry is 128 bytes */
#define SR_STATS_ALL        0xFFFFFFFFu
#define SR_STATS_MIN_P      4u
#define SR_STATS_MAX_P      12u
#define SR_STATS_MAX_REGS   67108864u /* 2^26 registers over all shards */
#define SR_STATS_MAX_ROWS   8u
#define SR_STATS_MIN_WIDTH  256u
#define SR_STATS_MAX_CELLS  16384u
#define SR_STATS_MIN_SLOTS  4u
#define SR_STATS_MAX_SLOTS  4096u
#define SR_STATS_DEFAULT_P          10u
#define SR_STATS_DEFAULT_ROWS       4u
#define SR_STATS_DEFAULT_WIDTH      4096u
#define SR_STATS_DEFAULT_SLOTS      256u
#define SR_STATS_DEFAULT_HOT_DIV    256u
#define SR_STATS_DEFAULT_HOT_MIN    1024u

typedef struct sr_stats_config {
    uint32_t hll_p, cms_rows, cms_width, hot_slots, hot_div, hot_min_lines;
} sr_stats_config;

typedef struct sr_stats_batch {
    const uint8_t *d_bytes; size_t nbytes;        /* the routed batch                                     */
    const sr_record *d_recs;                      /* input-order records (sr_batch.d_out)                 */
    const uint64_t *d_n_records; size_t max_records;
    const uint64_t *d_hashes;                     /* max_records u64 (sr_batch.d_hashes); required        */
} sr_stats_batch;

typedef struct sr_stats_hot {
    uint64_t hash;
    uint64_t lines;                               /* est(hash) in the snapshot that holds the entry       */
    uint32_t name_len;                            /* the name's full length                               */
    uint8_t name[SR_STATS_NAME_MAX];              /* its first bytes, zero filled                         */
} sr_stats_hot;

typedef struct sr_stats_snapshot {
    sr_stats_config cfg;                          /* the effective values (defaults filled in)            */
    uint32_t n_downstreams;
    uint32_t hot_overflow;
    uint64_t lines[4], bytes[4];                  /* per sr_verdict                                       */
    uint64_t ignored;
    uint64_t *shard_lines, *shard_bytes;          /* [n_downstreams]                                      */
    uint8_t *regs;                                /* [n_downstreams << hll_p], shard major                */
    uint64_t *cells;                              /* [cms_rows * cms_width], row major                    */
    sr_stats_hot *hot;                            /* n_hot entries, room for cfg.hot_slots                */
    uint32_t n_hot;
} sr_stats_snapshot;

int sr_stats_open(sr_ctx *ctx, const sr_stats_config *cfg);
int sr_stats_update(sr_ctx *ctx, const sr_stats_batch *batches, size_t count);
int sr_stats_reset(sr_ctx *ctx);
int sr_stats_read(sr_ctx *ctx, sr_stats_snapshot **out);
void sr_stats_free(sr_stats_snapshot *snap);
int sr_stats_close(sr_ctx *ctx);
uint64_t sr_name_hash(const uint8_t *bytes, size_t len);
uint64_t sr_stats_estimate(const sr_stats_snapshot *snap, uint64_t hash);
double sr_stats_cardinality(const sr_stats_snapshot *snap, uint32_t shard);
int sr_stats_merge(sr_stats_snapshot *into, const sr_stats_snapshot *from);

/* The name statistics of the host-memory path. With sr_set_name_stats(ctx, cfg) (cfg as sr_stats_open takes it;
 * the stage is opened when it is not yet, and an open stage keeps its configuration and state) every later
 * sr_route_pack_submit / sr_route_pack_submit_slots / sr_route_pack_batch also runs sr_stats_update over the
 * slot's input-order records and the route kernel's hashes, on the device: the hashes are requested as
 * sr_set_trace requests them, but nothing more crosses PCIe per batch. Read with sr_stats_read. NULL turns the
 * switch off (the state stays until sr_stats_close). Off by default: nothing is allocated, launched or copied.
 * Returns 0, -EINVAL, -ENOMEM, -EBUSY (a slot is in flight). */
int sr_set_name_stats(sr_ctx *ctx, const sr_stats_config *cfg_or_null);

/* ---- plain counters coalesced on the device -------------------------------------------------------- */
/* When a name is hot, most bytes sent to its downstream are copies of one line `<name>:<n>|c` that differ in a
 * small integer. This stage adds those integers together before the packets are packed. It consumes what the
 * route launch leaves on the device (the input-order records and the 64-bit name hashes) and writes a shorter
 * record list; the merged lines' text is appended to the batch itself, so sr_pack_packets and sr_pack_payloads
 * run unchanged on the result. Exact and deterministic (tests/coalesce_expect.py restates it); best effort by
 * construction: every merge made is exact, not every possible merge is made.
 *
 * Of a batch the first n = min(*d_n_records, max_records) records are read, d_hashes as given (never recomputed),
 * and no byte outside [0, nbytes).
 *
 * Plain counter: record i = (offset o, length L, route r) with r < n_downstreams, 6 <= L <= 1449,
 *   o + L <= nbytes, byte o + L - 1 a '\n', a first ':' in [o, o + L - 1) at k with
 *   1 <= k <= SR_COALESCE_NAME_MAX, and the bytes between that ':' and the '\n' exactly -?[0-9]{1,9}\|c (no '+',
 *   no tenth digit, no sample rate, no other type, no float, no empty value, no tags, no '\r'). Its name is the
 *   k bytes before the ':', its value v the decimal number ("-0" and leading zeros are accepted). Every other
 *   record, hostile ones included, passes through untouched.
 * Groups: with S slots per batch the slot of plain counter i is fmix64(hash_i) & (S - 1) (fmix64 as in the name
 *   statistics above). A slot's owner is the plain counter with the lowest index among those of the slot.
 *   Plain counter i joins its slot's owner o iff hash_i == hash_o, route_i == route_o, k_i == k_o and the name
 *   bytes are equal (the bytes are compared: sdbm collides, and adding two metrics together would be data
 *   corruption). A plain counter that does not join passes through untouched. The table is direct mapped: no
 *   probing, no overflow, no dependence on the order of execution.
 * Output: the records come out in input order into d_out, each as it was, except in groups of two or more
 *   members: there the owner becomes {offset = nbytes + a, length = k + 1 + len(dec) + 3, route} and the other
 *   members are dropped. The merged line is name ':' dec(sum of the group's values) "|c\n" (the sum a signed
 *   64-bit number; dec has a '-' when negative, no leading zeros, "0" for zero), and `a` is the total length of
 *   the merged lines of owners earlier in input order. The merged text goes to d_bytes + nbytes + a: the caller
 *   leaves append_cap bytes of room behind the batch. Of the text the first min(d_counts[3], append_cap) bytes
 *   are written and nothing at or past append_cap; the text is complete iff d_counts[3] <= append_cap, and only
 *   then are the merged records' offsets (nbytes + a, 32 bits) usable.
 *   d_counts: four u64 {records out, records dropped, groups merged, appended bytes needed}; &d_counts[0] is
 *   what a caller passes on as d_n_records. sr_pack_payloads then takes nbytes + append_cap as its nbytes.
 * Bounds: a merged line has 6..1449 bytes (hence k >= 1 and k <= 1425 = 1449 - 1 - 20 - 3). A group of c lines
 *   whose longest value has d digits sums to at most d + digits(c) digits and a sign, and
 *   1 + digits(c) <= 5 (c - 1) for every c >= 2: a merged line is never longer than its group's lines together.
 *   So for records that do not overlap (the route launch's never do) the appended bytes never exceed nbytes,
 *   and SR_COALESCE_APPEND_CAPACITY(nbytes) always suffices. |sum| < 2^60 since nbytes <= 2^30.
 *
 * sr_coalesce_config: slots = 0 selects SR_COALESCE_DEFAULT_SLOTS, otherwise a power of two in
 *   SR_COALESCE_MIN_SLOTS..SR_COALESCE_MAX_SLOTS.
 * sr_coalesce_open : allocates the tables once, SR_MAX_BATCHES_PER_LAUNCH x slots x 16 bytes (owner u32, members
 *   u32, sum i64); not inside stream capture. 0, -EINVAL, -ENOMEM, -EBUSY (the stage is open).
 * sr_coalesce      : count in 1..SR_MAX_BATCHES_PER_LAUNCH batches, asynchronous on the context's stream. Its
 *   per-record scratch is allocated on the first call or on one with more records (sum of max_records) than
 *   any before; later calls allocate nothing and can be captured in a graph. -EINVAL before any launch for a
 *   null required pointer (d_n_records, d_counts, d_hashes; d_recs and d_out with max_records > 0; d_bytes
 *   with nbytes > 0), d_out == d_recs, nbytes > 2^30, nbytes + append_cap > 0xFFFFFFF0,
 *   max_records > 0xFFFFFFF0, a bad count or a context whose stage is not open. d_recs and d_out are aligned as
 *   sr_record (4 bytes), d_hashes and d_counts to 8; d_bytes has any alignment.
 * sr_coalesce_close: waits for the stream and frees the stage, switch included (sr_close does it too). 0,
 *   -EINVAL, -EBUSY (a slot is in flight).
 *
 * Host only (no GPU):
 *   sr_coalesce_parse : the plain-counter test on one line of `len` bytes ('\n' included); 1 and *name_len = k,
 *     *value = v, or 0 (name_len and value may be NULL);
 *   sr_coalesce_format: writes name ':' dec(sum) "|c\n" to dst (name_len + 24 bytes always suffice) and returns
 *     its length. */
#define SR_COALESCE_NAME_MAX       1425u
#define SR_COALESCE_MIN_SLOTS      16u
#define SR_COALESCE_MAX_SLOTS      4194304u   /* 2^22 */
#define SR_COALESCE_DEFAULT_SLOTS  65536u
#define SR_COALESCE_MAX_BYTES      1073741824u   /* 2^30: a batch's nbytes */
#define SR_COALESCE_APPEND_CAPACITY(nbytes) (nbytes)

typedef struct sr_coalesce_config {
    uint32_t slots;
} sr_coalesce_config;

typedef struct sr_coalesce_batch {
    uint8_t *d_bytes; size_t nbytes;              /* the routed batch; the merged text goes behind it      */
    size_t append_cap;                            /* room behind d_bytes + nbytes                          */
    const sr_record *d_recs;                      /* input-order records (sr_batch.d_out)                  */
    const uint64_t *d_n_records; size_t max_records;
    const uint64_t *d_hashes;                     /* max_records u64 (sr_batch.d_hashes); required         */
    sr_record *d_out;                             /* max_records records; not d_recs                       */
    uint64_t *d_counts;                           /* 4 u64: out, dropped, groups, appended bytes needed    */
} sr_coalesce_batch;

int sr_coalesce_open(sr_ctx *ctx, const sr_coalesce_config *cfg);
int sr_coalesce_close(sr_ctx *ctx);
int sr_coalesce(sr_ctx *ctx, const sr_coalesce_batch *batches, size_t count);
int sr_coalesce_parse(const uint8_t *line, size_t len, uint32_t *name_len, int64_t *value);
size_t sr_coalesce_format(uint8_t *dst, const uint8_t *name, uint32_t name_len, int64_t sum);

/* The coalescing of the host-memory path. With sr_set_coalesce(ctx, cfg) (cfg as sr_coalesce_open takes it; the
 * stage is opened when it is not yet, and the context's input buffer is allocated again with max_batch_bytes of
 * room behind it) every later sr_route_pack_submit / sr_route_pack_submit_slots / sr_route_pack_batch runs
 * sr_coalesce between the route and the packing: the hashes are requested as sr_set_trace requests them, and the
 * packing and the payloads (sr_set_payloads) work on the coalesced records. `sorted`, `packets`, `fill`,
 * n_records and n_valid then describe the coalesced batch; records in `sorted` with offset >= nbytes point into
 * the merged text, at offset - nbytes. The trace (sr_route_pack_trace), the log text and the name statistics keep
 * the original input-order records, so logs and statistics are byte-identical to the switch being off. NULL
 * turns the switch off (the stage stays open until sr_coalesce_close, which fails with -EBUSY while a slot is in
 * flight). Off by default: nothing is allocated, launched or copied.
 * Returns 0, -EINVAL (max_batch_bytes > 2^30 or 2 * max_batch_bytes > 0xFFFFFFF0, a bad cfg), -ENOMEM, -EBUSY (a
 * slot is in flight).
 * sr_route_pack_coalesced: after sr_route_pack_result(slot) (for sr_route_pack_batch: slot 2), a page-locked copy
 * of the batch's merged text (*len bytes, valid until the slot's next submission) and the stage's four counts.
 * -EBUSY when the slot is in flight or was submitted with the switch off. */
int sr_set_coalesce(sr_ctx *ctx, const sr_coalesce_config *cfg_or_null);
int sr_route_pack_coalesced(sr_ctx *ctx, int slot, const uint8_t **text, size_t *len, uint64_t counts[4]);

/* ---- name rules on the device: drop or keep metrics by name and prefix ----------------------------- */
/* A block list or an allow list for a router that fronts a shared statsd tier. The stage sits between the route
 * launch and the packing (or sr_coalesce): it consumes the input-order records, and the hashes when given, and
 * writes a shorter record list; sr_pack_packets, sr_pack_payloads and sr_coalesce run unchanged on the result.
 * Exact and deterministic (tests/rules_expect.py restates it).
 *
 * Rule set: n_rules rules, 0 <= n_rules <= SR_RULES_MAX, and a default action. A rule is {pattern, len, kind,
 *   action}: kind SR_RULE_PREFIX or SR_RULE_EXACT, action SR_RULE_DROP or SR_RULE_KEEP, the pattern 1 to
 *   SR_RULES_PATTERN_MAX bytes of any value except ':' and '\n' (NUL and high bytes are allowed). The patterns of
 *   a set hold at most SR_RULES_TEXT_MAX bytes together. Two rules of the same kind and bytes are -EINVAL. A
 *   default action of SR_RULE_DROP makes the set an allow list.
 * Subject records: a record (o, L, r) is subject to the rules iff r < n_downstreams, L >= 1 and
 *   o + L <= nbytes. Every other record (invalid lines, all-dead lines, hostile records) passes through
 *   untouched and unmatched. No byte outside [0, nbytes) is ever read.
 * Match, on bytes only: a PREFIX rule of length p matches iff p <= L - 1 and bytes [o, o + p) equal the pattern.
 *   An EXACT rule matches iff p + 1 <= L - 1, bytes [o, o + p) equal the pattern and byte o + p is ':'. A pattern
 *   holds no ':', so for a routed line a match implies that the first ':' is at or behind p: a PREFIX match is a
 *   prefix of the name and an EXACT match is the whole name. No name length is needed.
 * Which rule wins: the longest matching pattern; between an EXACT and a PREFIX rule of one text the EXACT one.
 *   The order of the rules does not matter. No match gives the default action; its index is n_rules.
 * Output: d_out receives the records whose action is KEEP and those that are not subject, in input order. When
 *   d_hashes and d_hashes_out are both given the hashes are compacted alongside (so sr_coalesce can follow).
 *   The optional d_match (u16 per input record) receives the winning rule's index: n_rules for the default,
 *   SR_RULES_NOT_SUBJECT for a record that is not subject. d_counts: four u64 {records out, records dropped,
 *   bytes dropped, subject records}; &d_counts[0] is what the next stage takes as d_n_records. Of a batch the
 *   first min(*d_n_records, max_records) records are read.
 * Hits: the context keeps {lines, bytes} as u64 per rule and for the default, n_rules + 1 pairs, accumulated
 *   over all calls since sr_rules_open or the last sr_rules_reset.
 *
 * sr_rules_open : compiles and uploads the set; not inside stream capture. 0, -EINVAL (a bad set, or the
 *   context's stream is capturing), -EBUSY (the stage is open), -ENOMEM.
 * sr_rules      : count in 1..SR_MAX_BATCHES_PER_LAUNCH batches, asynchronous on the context's stream. Its
 *   scratch is allocated on the first call or on one with more records (sum of max_records) than any before;
 *   later calls allocate nothing and can be captured in a graph. -EINVAL before any launch for a null required
 *   pointer (d_n_records, d_counts; d_recs and d_out with max_records > 0; d_bytes with nbytes > 0),
 *   d_out == d_recs, d_hashes_out == d_hashes (when given), d_counts == d_n_records, nbytes > 0xFFFFFFF0,
 *   max_records > 0xFFFFFFF0, a bad count or a context whose stage is not open. d_recs and d_out are aligned as
 *   sr_record (4 bytes), d_hashes, d_hashes_out and d_counts to 8, d_match to 2; d_bytes has any alignment.
 * sr_rules_read : waits for the stream and copies the first min(n, n_rules + 1) pairs of hits (the default's is
 *   the last, at n_rules); returns how many it copied, or -EINVAL.
 * sr_rules_reset: zeroes the hits, in stream order.
 * sr_rules_close: waits for the stream and frees the stage, switch included (sr_close does it too). 0, -EINVAL,
 *   -EBUSY (a slot is in flight).
 *
 * Host only (no GPU):
 *   sr_rules_check     : 0 or -EINVAL for a set, as sr_rules_open judges it;
 *   sr_rules_match     : the winning rule's index for one line of `len` bytes ('\n' included; len = 0 and
 *     len = 1 match nothing), n_rules for the default, -EINVAL for a bad set or a null line;
 *   sr_rules_parse_text: the rule file's format into a config that the caller frees with sr_rules_free. One rule
 *     per line: `drop <pattern>` or `keep <pattern>` for an exact name, a trailing `*` marks a prefix;
 *     `default drop` or `default keep` sets the default (at most once; keep without it); a line that begins
 *     with `#` is a comment and empty lines are skipped. The pattern is every byte after the single space up to
 *     the end of the line, so it may hold spaces, '#' and a '\r'. An exact name that ends in `*` cannot be
 *     written in the file (the C structure can express it). On error -EINVAL and *err_line = the 1-based line
 *     at fault: an unknown word, a missing or bad pattern, a duplicate (the second of the two), too many rules
 *     or too many pattern bytes. */
#define SR_RULES_MAX          256u
#define SR_RULES_PATTERN_MAX  64u
#define SR_RULES_TEXT_MAX     4096u
#define SR_RULES_NOT_SUBJECT  0xFFFFu
#define SR_RULE_PREFIX        0u
#define SR_RULE_EXACT         1u
#define SR_RULE_DROP          0u
#define SR_RULE_KEEP          1u

typedef struct sr_rule {
    const uint8_t *pattern;
    uint32_t len;
    uint8_t kind;       /* SR_RULE_PREFIX, SR_RULE_EXACT */
    uint8_t action;     /* SR_RULE_DROP, SR_RULE_KEEP    */
} sr_rule;

typedef struct sr_rules_config {
    const sr_rule *rules;
    uint32_t n_rules;
    uint32_t default_action;
} sr_rules_config;

typedef struct sr_rules_batch {
    const uint8_t *d_bytes; size_t nbytes;        /* the routed batch                                      */
    const sr_record *d_recs;                      /* input-order records (sr_batch.d_out)                  */
    const uint64_t *d_n_records; size_t max_records;
    sr_record *d_out;                             /* max_records records; not d_recs                       */
    const uint64_t *d_hashes;                     /* optional: max_records u64 (sr_batch.d_hashes) ...     */
    uint64_t *d_hashes_out;                       /* ... compacted into these, when both are given         */
    uint16_t *d_match;                            /* optional: max_records u16, the winning rule's index   */
    uint64_t *d_counts;                           /* 4 u64: out, dropped, bytes dropped, subject           */
} sr_rules_batch;

typedef struct sr_rule_hits {
    uint64_t lines, bytes;
} sr_rule_hits;

int sr_rules_open(sr_ctx *ctx, const sr_rules_config *cfg);
int sr_rules_close(sr_ctx *ctx);
int sr_rules(sr_ctx *ctx, const sr_rules_batch *batches, size_t count);
int sr_rules_read(sr_ctx *ctx, sr_rule_hits *hits, size_t n);
int sr_rules_reset(sr_ctx *ctx);
int sr_rules_check(const sr_rules_config *cfg);
int sr_rules_match(const sr_rules_config *cfg, const uint8_t *line, size_t len);
int sr_rules_parse_text(const char *text, size_t len, sr_rules_config **out, size_t *err_line);
void sr_rules_free(sr_rules_config *cfg);

/* The name rules of the host-memory path. With sr_set_name_rules(ctx, cfg) (the stage is opened with cfg; an
 * open stage is closed first, hits included) every later sr_route_pack_submit / sr_route_pack_submit_slots /
 * sr_route_pack_batch runs the route launch, then sr_rules, then sr_coalesce when sr_set_coalesce is on, then the
 * packing, in place of the fused route and pack. Rules run before the coalescing, so dropped lines are never
 * merged. `sorted`, `packets`, `fill`, n_records and n_valid then describe the kept lines. The trace
 * (sr_route_pack_trace), the log text and the name statistics keep the original records: logs and statistics are
 * byte-identical to the switch being off, and a muted name stays visible among the hot names. NULL turns the
 * switch off (the stage and its hits stay until sr_rules_close). Off by default: nothing is allocated, launched
 * or copied.
 * Returns 0, -EINVAL (a bad set), -ENOMEM, -EBUSY (a slot is in flight).
 * sr_route_pack_rules: after sr_route_pack_result(slot) (for sr_route_pack_batch: slot 2), the batch's four
 * counts. -EBUSY when the slot is in flight or was submitted with the switch off. */
int sr_set_name_rules(sr_ctx *ctx, const sr_rules_config *cfg_or_null);
int sr_route_pack_rules(sr_ctx *ctx, int slot, uint64_t counts[4]);

/* ---- line grammar on the device: count or drop lines that no statsd would parse --------------------- */
/* The router forwards any line that has a ':' and a legal length. This stage looks at what stands behind the
 * name: it consumes the input-order records of a route launch, and the hashes when given, judges every line
 * against the statsd line grammar below and writes a shorter record list, as sr_rules does; sr_rules, sr_coalesce
 * and the packing run unchanged on the result. Exact and deterministic (tests/validate_expect.py restates it).
 *
 * Subject records: a record (o, L, r) is subject iff r < n_downstreams, L >= 1 and o + L <= nbytes (sr_rules'
 *   rule). Every other record passes through untouched with the reason SR_VALID_NOT_SUBJECT. No byte outside
 *   [0, nbytes) is ever read.
 * Content: the content C of a subject record is its L bytes without the last byte when that byte is '\n'. A line
 *   that ends its batch without a newline is judged on all L bytes.
 * Byte classes: TB is 0x21..0x7E except '|'; NB is TB except ':'. A '\n', NUL or high byte inside C is simply
 *   outside both classes.
 * Judgement: the first failing step gives the reason; the steps in this order:
 *   1. p = the index of the first ':' in C. None: NO_COLON. p == 0: EMPTY_NAME. A byte of C[0:p] outside NB:
 *      NAME_BYTE.
 *   2. C[p+1:] is split at every '|' into the fields f0 .. fk. k == 0: NO_TYPE.
 *   3. f1 is one of c g ms h s d, and its bit (SR_VALID_TYPE_*) is set in accept_types; otherwise TYPE.
 *   4. f0 against the type; anything else, the empty value included, is VALUE:
 *        number = [0-9]{1,20}(\.[0-9]{1,20})?
 *        c: -?number     g: [+-]?number     ms, h, d: number     s: 1 to 64 bytes of TB
 *   5. f2 .. fk from left to right: a field begins with '@' or '#', there is at most one of each and '@' comes
 *      before '#'; otherwise SECTION. After '@' comes number and the type is c, ms, h or d; otherwise RATE.
 *      After '#' come 1 or more bytes of TB (':' and ',' are legal there); otherwise TAGS.
 *   6. OK.
 * Configuration: a subject record whose reason's bit is set in drop_mask is dropped; every other record is kept.
 *   drop_mask == 0 counts and drops nothing. -EINVAL: bit 0 (OK) or a bit at or above SR_VALID_REASONS in
 *   drop_mask, accept_types == 0, an unknown bit in accept_types.
 * Output, as sr_rules: d_out receives the kept and the non-subject records in input order; when d_hashes and
 *   d_hashes_out are both given the hashes are compacted alongside. The optional d_reason (u8 per input record)
 *   receives the reason. d_counts: four u64 {records out, records dropped, bytes dropped, subject records};
 *   &d_counts[0] is what the next stage takes as d_n_records. Of a batch the first
 *   min(*d_n_records, max_records) records are read.
 * Hits: the context keeps {lines, bytes} as u64 per reason, SR_VALID_REASONS pairs (index 0: the OK lines),
 *   accumulated over all calls since sr_validate_open or the last sr_validate_reset.
 *
 * sr_validate_open, sr_validate, sr_validate_read, sr_validate_reset, sr_validate_close: as their sr_rules
 *   namesakes — the same returns, the same alignment rules (d_reason has any alignment) and pointer checks
 *   (d_out != d_recs, d_hashes_out != d_hashes, d_counts != d_n_records, nbytes and max_records at most
 *   0xFFFFFFF0), scratch on the first call or a larger one, capturable afterwards, 1..SR_MAX_BATCHES_PER_LAUNCH
 *   batches per call; sr_close closes the stage. sr_validate_read copies the first min(n, SR_VALID_REASONS) pairs.
 *
 * Host only (no GPU):
 *   sr_validate_check      : 0 or -EINVAL for a configuration;
 *   sr_validate_line       : the reason of one line of `len` bytes ('\n' included when it has one; len >= 1),
 *     -EINVAL for a bad configuration, a null line or len == 0;
 *   sr_validate_reason_name: ok, no_colon, empty_name, name_byte, no_type, type, value, section, rate, tags;
 *     NULL for any other number;
 *   sr_validate_parse_spec : `count` (drop nothing), `drop` (drop every reason but OK) or a comma list of reason
 *     names to drop, into *cfg_out with every type accepted; anything else is -EINVAL. */
#define SR_VALID_OK           0u
#define SR_VALID_NO_COLON     1u
#define SR_VALID_EMPTY_NAME   2u
#define SR_VALID_NAME_BYTE    3u
#define SR_VALID_NO_TYPE      4u
#define SR_VALID_TYPE         5u
#define SR_VALID_VALUE        6u
#define SR_VALID_SECTION      7u
#define SR_VALID_RATE         8u
#define SR_VALID_TAGS         9u
#define SR_VALID_REASONS      10u
#define SR_VALID_NOT_SUBJECT  0xFFu
#define SR_VALID_TYPE_C       1u
#define SR_VALID_TYPE_G       2u
#define SR_VALID_TYPE_MS      4u
#define SR_VALID_TYPE_H       8u
#define SR_VALID_TYPE_S       16u
#define SR_VALID_TYPE_D       32u
#define SR_VALID_TYPES_ALL    63u

typedef struct sr_validate_config {
    uint32_t drop_mask;      /* bit r: drop the lines of reason r (never bit 0) */
    uint32_t accept_types;   /* SR_VALID_TYPE_* bits                            */
} sr_validate_config;

typedef struct sr_validate_batch {
    const uint8_t *d_bytes; size_t nbytes;        /* the routed batch                                      */
    const sr_record *d_recs;                      /* input-order records (sr_batch.d_out)                  */
    const uint64_t *d_n_records; size_t max_records;
    sr_record *d_out;                             /* max_records records; not d_recs                       */
    const uint64_t *d_hashes;                     /* optional: max_records u64 (sr_batch.d_hashes) ...     */
    uint64_t *d_hashes_out;                       /* ... compacted into these, when both are given         */
    uint8_t *d_reason;                            /* optional: max_records u8, the line's reason           */
    uint64_t *d_counts;                           /* 4 u64: out, dropped, bytes dropped, subject           */
} sr_validate_batch;

typedef struct sr_validate_hits {
    uint64_t lines, bytes;
} sr_validate_hits;

int sr_validate_open(sr_ctx *ctx, const sr_validate_config *cfg);
int sr_validate_close(sr_ctx *ctx);
int sr_validate(sr_ctx *ctx, const sr_validate_batch *batches, size_t count);
int sr_validate_read(sr_ctx *ctx, sr_validate_hits *hits, size_t n);
int sr_validate_reset(sr_ctx *ctx);
int sr_validate_check(const sr_validate_config *cfg);
int sr_validate_line(const sr_validate_config *cfg, const uint8_t *line, size_t len);
const char *sr_validate_reason_name(uint32_t reason);
int sr_validate_parse_spec(const char *text, sr_validate_config *cfg_out);

/* The line grammar of the host-memory path. With sr_set_validate(ctx, cfg) (the stage is opened with cfg; an open
 * stage is closed first, hits included) every later sr_route_pack_submit / sr_route_pack_submit_slots /
 * sr_route_pack_batch runs the route launch, then sr_validate, then sr_rules when sr_set_name_rules is on, then
 * sr_coalesce when sr_set_coalesce is on, then the packing. The grammar runs first, so rule hits and merges see
 * only kept lines. `sorted`, `packets`, `fill`, n_records and n_valid then describe the kept lines. The trace
 * (sr_route_pack_trace), the log text and the name statistics keep the route launch's records: logs and statistics
 * are byte-identical to the switch being off. NULL turns the switch off (the stage and its hits stay until
 * sr_validate_close). Off by default: nothing is allocated, launched or copied.
 * Returns 0, -EINVAL (a bad configuration), -ENOMEM, -EBUSY (a slot is in flight).
 * sr_route_pack_validate: after sr_route_pack_result(slot) (for sr_route_pack_batch: slot 2), the batch's four
 * counts. -EBUSY when the slot is in flight or was submitted with the switch off. */
int sr_set_validate(sr_ctx *ctx, const sr_validate_config *cfg_or_null);
int sr_route_pack_validate(sr_ctx *ctx, int slot, uint64_t counts[4]);

/* ---- sample rates on the device: thin hot timers the way a client would have ----------------------- */
/* Timers, histograms and distributions (|ms, |h, |d) cannot be added together as sr_coalesce adds plain counters,
 * and a hot name of them overloads its shard all the same. Every statsd has one answer: send one line in k and
 * mark it `|@<1/k>`, so that the server scales the counts back. This stage does that for clients that do not: it
 * counts the lines per name in a batch, thins the names that exceed a limit, and writes the kept lines with the
 * sample rate inserted. It consumes the input-order records and the hashes of a route launch and writes a shorter
 * record list, as sr_rules and sr_validate do; sr_coalesce and the packing run unchanged on the result. A sampled
 * `|c` line carries an '@' and so is no longer a plain counter: sr_coalesce does not merge it. Exact and
 * deterministic (tests/sample_expect.py restates it).
 *
 * Subject records: a record (o, L, r) is subject iff r < n_downstreams, L >= 1 and o + L <= nbytes (sr_rules'
 *   rule). No byte outside [0, nbytes) is ever read.
 * Sampleable: a subject record is sampleable iff all of the following hold:
 *   1. 6 <= L <= SR_SAMPLE_LINE_MAX (1441 = 1449 - SR_SAMPLE_EXTRA_MAX) and the last byte is '\n'. The content C
 *      is the first L - 1 bytes.
 *   2. p = the index of the first ':' in C, and p >= 1.
 *   3. q = the index of the first '|' in C[p+1:], as an index into C. It exists and q > p + 1 (a value of at
 *      least one byte).
 *   4. e = the index of the next '|' behind q, or len(C) when there is none. C[q+1:e] is exactly one of c, ms, h,
 *      d, and that type's bit (SR_VALID_TYPE_C, _MS, _H, _D) is set in the configuration's `types`.
 *   5. Either e == len(C), or e + 1 < len(C) and C[e+1] == '#'.
 *   So a line that already carries an '@' section is not sampleable, nor is one with an empty or unknown type.
 *   Name bytes, the value's shape and the tags are not judged: that is sr_validate's work, which runs before this
 *   stage. Every record that is not sampleable passes through untouched. ins = e is the insertion point.
 * Count: with S slots per batch the slot of a sampleable record i is fmix64(hash_i) & (S - 1), fmix64 being the
 *   MurmurHash3 finaliser that the name statistics use and hash_i = d_hashes[i] as given (never recomputed).
 *   c(slot) is the number of sampleable records of the batch in that slot. No names are compared: names that share
 *   a slot share a count and a budget. That is harmless here, because every kept line still carries the rate by
 *   which its own slot was thinned, so the server's scaled counts stay unbiased per line.
 * Step: the ladder K is 1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 5000, 10000 (SR_SAMPLE_STEPS entries) and
 *   the rate texts R are "", 0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002, 0.001, 0.0005, 0.0002, 0.0001. The
 *   step j of a sampleable record is the smallest j with c <= (u64)limit * K[j]; without such a j it is 12.
 * Keep: a sampleable record with j == 0 is kept as it is. With j >= 1 record i (its index in the stage's input)
 *   is kept iff ((u >> 32) * K[j]) >> 32 == 0 with u = fmix64(hash_i ^ (seed + i * 0x9E3779B97F4A7C15)), all modulo
 *   2^64, and seed = cfg.seed + batch.seed_add. A Bernoulli draw per line, as a client makes it; deterministic for
 *   a seed and independent of the order of execution.
 * Output: d_out receives, in input order, the records that are not sampleable and the kept records of step 0 as
 *   they were, nothing for the dropped ones, and for a kept record of step j >= 1
 *   {offset = nbytes + a, length = L + 2 + len(R[j]), route}: its text line[0:ins] + "|@" + R[j] + line[ins:L] is
 *   written to d_bytes + nbytes + a, a being the total length of the rewritten lines of earlier records. When
 *   d_hashes_out is given the hashes are compacted alongside (so sr_coalesce can follow). The optional d_step (u8
 *   per input record) receives SR_SAMPLE_NOT_SAMPLEABLE, or j with bit 7 set when the record was dropped.
 *   d_counts: four u64 {records out, records dropped, lines rewritten, appended bytes needed}; &d_counts[0] is
 *   what the next stage takes as d_n_records. Of the text the first min(d_counts[3], append_cap) bytes are
 *   written, nothing at or past append_cap; the text is complete iff d_counts[3] <= append_cap (an offset is
 *   taken modulo 2^32, which only an incomplete text can reach). Of a batch the first
 *   min(*d_n_records, max_records) records are read.
 *   SR_SAMPLE_APPEND_CAPACITY(nbytes) = nbytes + (nbytes / 6) * 8 always suffices for records that do not
 *   overlap: the rewritten lines are lines of the batch, together at most nbytes bytes, each of them has at least
 *   6 bytes, so there are at most nbytes / 6 of them, and each grows by at most SR_SAMPLE_EXTRA_MAX = 8 bytes
 *   ("|@0.0001").
 * Hits: the context keeps {seen, kept} as u64 per step, SR_SAMPLE_STEPS pairs, accumulated over all calls since
 *   sr_sample_open or the last sr_sample_reset.
 * Configuration: slots 0 selects SR_SAMPLE_DEFAULT_SLOTS, otherwise a power of two in SR_SAMPLE_MIN_SLOTS ..
 *   SR_SAMPLE_MAX_SLOTS; limit >= 1; types non-zero and within C | MS | H | D; reserved 0. Anything else -EINVAL.
 *
 * sr_sample_open : allocates the table (slots u32 for each of SR_MAX_BATCHES_PER_LAUNCH batches) and the hits;
 *   not inside stream capture. 0, -EINVAL, -EBUSY (the stage is open), -ENOMEM.
 * sr_sample      : count in 1..SR_MAX_BATCHES_PER_LAUNCH batches, asynchronous on the context's stream. Scratch
 *   is allocated on the first call or a larger one; later calls allocate nothing and can be captured in a graph.
 *   -EINVAL before any launch for a null required pointer (d_n_records, d_counts, d_hashes; d_recs and d_out with
 *   max_records > 0; d_bytes with nbytes > 0 or append_cap > 0), d_out == d_recs, d_hashes_out == d_hashes,
 *   d_counts == d_n_records, nbytes > SR_SAMPLE_MAX_BYTES (2^30), nbytes + append_cap > 0xFFFFFFF0,
 *   max_records > 0xFFFFFFF0, a bad count or a stage that is not open. Alignment as sr_validate (d_step: any).
 * sr_sample_read : waits for the stream and copies the first min(n, SR_SAMPLE_STEPS) pairs; returns how many.
 * sr_sample_reset: zeroes the hits, in stream order.
 * sr_sample_close: waits for the stream and frees the stage (sr_close does it too). 0, -EINVAL, -EBUSY.
 *
 * Host only (no GPU):
 *   sr_sample_check     : 0 or -EINVAL for a configuration;
 *   sr_sample_parse     : 1 when the line of `len` bytes is sampleable under `types` (*ins and *type_bit are then
 *     set), else 0; -EINVAL for a null line;
 *   sr_sample_step      : the step for a limit and a count;
 *   sr_sample_keep      : 1 or 0, the keep rule (step >= SR_SAMPLE_STEPS: -EINVAL);
 *   sr_sample_rate_text : R[step], NULL for any other number;
 *   sr_sample_rewrite   : writes line[0:ins] + "|@" + R[step] + line[ins:len] to dst and returns its length (dst has
 *     len + SR_SAMPLE_EXTRA_MAX bytes of room; 0 for step == 0, step >= SR_SAMPLE_STEPS or ins > len);
 *   sr_sample_parse_spec: `<limit>` or `<limit>:<comma list of c, ms, h, d>` into *cfg_out; the default types are
 *     ms, h, d, the seed is 0 and the slots are the default; anything else is -EINVAL. */
#define SR_SAMPLE_STEPS          13u
#define SR_SAMPLE_EXTRA_MAX      8u
#define SR_SAMPLE_LINE_MAX       1441u
#define SR_SAMPLE_NOT_SAMPLEABLE 0xFFu
#define SR_SAMPLE_DROPPED        0x80u
#define SR_SAMPLE_DEFAULT_SLOTS  65536u
#define SR_SAMPLE_MIN_SLOTS      16u
#define SR_SAMPLE_MAX_SLOTS      (1u << 22)
#define SR_SAMPLE_MAX_BYTES      ((size_t)1 << 30)
#define SR_SAMPLE_TYPES_ALL      (1u | 4u | 8u | 32u)   /* SR_VALID_TYPE_C | _MS | _H | _D */
#define SR_SAMPLE_APPEND_CAPACITY(nbytes) ((size_t)(nbytes) + ((size_t)(nbytes) / 6u) * 8u)

typedef struct sr_sample_config {
    uint32_t slots;      /* 0: SR_SAMPLE_DEFAULT_SLOTS                        */
    uint32_t limit;      /* lines of one slot a batch keeps at full rate, >= 1 */
    uint32_t types;      /* SR_VALID_TYPE_C | _MS | _H | _D bits               */
    uint32_t reserved;   /* 0                                                  */
    uint64_t seed;
} sr_sample_config;

typedef struct sr_sample_batch {
    uint8_t *d_bytes; size_t nbytes;              /* the routed batch; the rewritten lines go behind it    */
    size_t append_cap;                            /* room behind d_bytes + nbytes                          */
    const sr_record *d_recs;                      /* input-order records (sr_batch.d_out)                  */
    const uint64_t *d_n_records; size_t max_records;
    const uint64_t *d_hashes;                     /* max_records u64 (sr_batch.d_hashes); required         */
    sr_record *d_out;                             /* max_records records; not d_recs                       */
    uint64_t *d_hashes_out;                       /* optional: the hashes, compacted alongside             */
    uint8_t *d_step;                              /* optional: max_records u8, the record's step           */
    uint64_t *d_counts;                           /* 4 u64: out, dropped, rewritten, appended bytes needed */
    uint64_t seed_add;                            /* added to the configuration's seed                     */
} sr_sample_batch;

typedef struct sr_sample_hits {
    uint64_t seen, kept;
} sr_sample_hits;

int sr_sample_open(sr_ctx *ctx, const sr_sample_config *cfg);
int sr_sample_close(sr_ctx *ctx);
int sr_sample(sr_ctx *ctx, const sr_sample_batch *batches, size_t count);
int sr_sample_read(sr_ctx *ctx, sr_sample_hits *hits, size_t n);
int sr_sample_reset(sr_ctx *ctx);
int sr_sample_check(const sr_sample_config *cfg);
int sr_sample_parse(const uint8_t *line, size_t len, uint32_t types, uint32_t *ins, uint32_t *type_bit);
uint32_t sr_sample_step(uint32_t limit, uint64_t c);
int sr_sample_keep(uint64_t hash, uint64_t seed, uint64_t index, uint32_t step);
const char *sr_sample_rate_text(uint32_t step);
size_t sr_sample_rewrite(uint8_t *dst, const uint8_t *line, size_t len, uint32_t ins, uint32_t step);
int sr_sample_parse_spec(const char *text, sr_sample_config *cfg_out);

/* The sample rates of the host-memory path. With sr_set_sample(ctx, cfg) (the stage is opened with cfg; an open
 * stage is closed first, hits included) every later sr_route_pack_submit / sr_route_pack_submit_slots /
 * sr_route_pack_batch runs the route launch, then sr_validate when sr_set_validate is on, then sr_rules when
 * sr_set_name_rules is on, then sr_sample, then sr_coalesce when sr_set_coalesce is on, then the packing: each
 * stage reads the one before's records, count and hashes. Sampling stands before the coalescing because sr_coalesce
 * does not hand hashes on; a sampled `|c` line is no longer a plain counter and is not merged.
 * The context's input buffer is allocated again with SR_SAMPLE_APPEND_CAPACITY(max_batch_bytes) of room behind the
 * batch, and the coalescing's max_batch_bytes behind that when both are (or were) on: a batch's rewritten lines lie
 * at d_in + nbytes, sr_coalesce takes nbytes + SR_SAMPLE_APPEND_CAPACITY(nbytes) as its nbytes and writes its merged
 * text behind that, and the payload gather (sr_set_payloads) takes the whole as its batch. Records in `sorted`
 * with offset in [nbytes, nbytes + SR_SAMPLE_APPEND_CAPACITY(nbytes)) point into the rewritten text, at
 * offset - nbytes; those behind it into the merged text. seed_add is the number of submissions accepted on the
 * context since sr_set_sample (empty ones included), so the first uses cfg.seed and successive batches thin
 * different positions. `sorted`, `packets`, `fill`, n_records and n_valid describe the thinned batch (whose lines
 * may be up to SR_SAMPLE_EXTRA_MAX bytes longer: the slots' packets and payloads are sized for it). The trace
 * (sr_route_pack_trace), the log text and the name statistics keep the route launch's records: logs and
 * statistics are byte-identical to the switch being off. NULL turns the switch off (the stage and its hits stay
 * until sr_sample_close). Off by default: nothing is allocated, launched or copied.
 * Returns 0, -EINVAL (a bad configuration, max_batch_bytes > SR_SAMPLE_MAX_BYTES, or a buffer that would pass
 * 0xFFFFFFF0 bytes), -ENOMEM, -EBUSY (a slot is in flight).
 * sr_route_pack_sample: after sr_route_pack_result(slot) (for sr_route_pack_batch: slot 2), a page-locked copy of
 * the batch's rewritten text (*len bytes, valid until the slot's next submission), the stage's four counts and the
 * seed the batch was thinned under (cfg.seed + seed_add). -EBUSY when the slot is in flight or was submitted with
 * the switch off. */
int sr_set_sample(sr_ctx *ctx, const sr_sample_config *cfg_or_null);
int sr_route_pack_sample(sr_ctx *ctx, int slot, const uint8_t **text, size_t *len, uint64_t counts[4], uint64_t *seed);

/* ---- owner side of the multi-GPU regroup: received lines into packets ------------------------------ */
/* After sr_regroup_launch / sr_regroup_run the lines of the shards a GPU owns lie in d_recv_bytes /
 * d_recv_recs: every source's chunk in source order 0, 1, ..., each chunk batch 0's lines, then batch
 * 1's, in input order. The owner is the one data thread of those shards: per shard it first drops the
 * pending buffer of every shard that ANY source's launch probed dead (find_downstream zeroes
 * active_buffer_length of the dead downstreams it visits, sr-main.c:106), then pushes the received
 * lines (push_to_downstream / ds_schedule_flush, sr-main.c:49-83). The drop comes first because a source
 * with a newer alive snapshot may send lines to a shard that another source still probed dead: the old
 * pending bytes go, the new lines stay. (A source that flags a shard sends it no lines, so placing every
 * flagging source before every sending one is a valid serial order per shard.) Per launch:
 *   route with sr_batch.d_probed_dead -> sr_regroup_launch -> sr_exchange_dead -> sr_owner_pack
 *   -> copy of the arena to the host; sr_flush_pending on the flush tick (ds_flush_timer_cb).
 *
 * sr_exchange_dead_run: the launch's probed-dead bitmaps to every owner. d_all_dead is u64
 *   [world][nwords], nwords = max(1, ceil(n_downstreams / 64)). One kernel on the context's stream ORs
 *   batches[j].d_probed_dead (NULL: nothing) over the launch's `count` batches (0..
 *   SR_MAX_BATCHES_PER_LAUNCH) into row `rank`; then, within one group_start / group_end, row `rank` is
 *   sent to every peer q != rank and row q received from it, in rank order, nwords * 8 bytes each under
 *   tag 2. world == 1 makes no transport call. Only group_start, group_end, send and recv of the
 *   transport are used; a transport that moves the rows from the host first waits for the context's
 *   stream. Returns 0, -EINVAL or the first callback error (every operation is posted even so).
 * sr_exchange_dead: the same on RCCL (ncclSend / ncclRecv on the context's stream), asynchronous.
 *   Collective: every rank of the comm calls it once per launch, after sr_regroup_launch. */
int sr_exchange_dead_run(sr_ctx *ctx, const sr_transport *t, int world, int rank, const sr_batch *batches,
                         size_t count, uint64_t *d_all_dead);
int sr_exchange_dead(sr_ctx *ctx, sr_comm *comm, const sr_batch *batches, size_t count, uint64_t *d_all_dead);

/* sr_owner_pack: one launch's receive buffer into packets (asynchronous on the context's stream).
 * With dead = the column-OR of d_all_dead's rows and fill_eff[s] = 0 for s in dead, else d_fill_in[s], the
 * outputs are those of sr_pack_packets(d_recv_recs, the sum of d_recv_counts[p][0], max_records,
 * fill_eff, NULL, ...) and, with d_payload, of sr_pack_payloads on d_recv_bytes: a dropped shard's first
 * packet has carry 0 and reads nothing of d_pend_in, and a dropped shard without lines leaves
 * d_fill_out[s] = 0 bytes in its d_pend_out slot. One small kernel (the fold) writes the line total and
 * fill_eff into memory of the context; the packing and the gather run unchanged. Shards this GPU does not
 * own receive no lines and pass through (apart from the drop).
 * Rules of sr_pack_packets (descriptors past max_packets not written: check d_counts[0]) and, with
 * d_payload, of sr_pack_payloads (d_pend_out needs d_pend_in and must not be it, so consecutive launches
 * alternate two pending buffers; SR_PAYLOAD_CAPACITY(recv_nbytes, n_downstreams) always suffices; check
 * *d_total <= payload_cap). d_fill_out may be d_fill_in. world in 1..SR_MAX_OWNERS, n_downstreams <=
 * SR_MAX_PACK_DOWNSTREAMS. The first call (or one with a larger max_records) allocates scratch: not
 * inside stream capture. Returns 0, -EINVAL, -ENOMEM, -EIO. */
typedef struct sr_owner_batch {
    const uint8_t *d_recv_bytes;   /* the receive buffers of sr_regroup_launch                           */
    size_t recv_nbytes;            /* host value: the sum of h_received's bytes                          */
    const sr_record *d_recv_recs;
    size_t max_records;            /* room of d_recv_recs and of d_sorted                                */
    const uint64_t *d_recv_counts; /* u64 [world][2] {lines, bytes} per source                           */
    int world;
    const uint64_t *d_all_dead;    /* NULL (nothing dropped) or u64 [world][nwords] (sr_exchange_dead)   */
    const uint16_t *d_fill_in;     /* NULL (nothing pending) or n_downstreams u16                        */
    sr_record *d_sorted;           /* as sr_pack_packets from here on                                    */
    sr_packet *d_packets;
    size_t max_packets;
    uint64_t *d_counts;            /* 3 u64: {descriptors, valid lines, lines}                           */
    uint16_t *d_fill_out;
    const uint8_t *d_pend_in;      /* as sr_payload_batch from here on (used only with d_payload)        */
    uint8_t *d_pend_out;
    uint8_t *d_payload;            /* NULL: descriptors only                                             */
    size_t payload_cap;
    uint32_t *d_offsets;           /* max_packets + 1                                                    */
    uint64_t *d_total;
} sr_owner_batch;
int sr_owner_pack(sr_ctx *ctx, const sr_owner_batch *batch);

/* sr_flush_pending: ds_flush_timer_cb (sr-main.c:194-204) for pending buffers that live on the device:
 * every downstream s with d_fill[s] > 0, in downstream order, becomes one descriptor {first 0, nlines 0,
 * shard s, length 0, carry d_fill[s], open 0} whose bytes are the first d_fill[s] bytes of slot s of
 * d_pend (SR_PENDING_STRIDE apart). d_counts (3 u64) = {descriptors needed, 0, 0}; with n =
 * min(d_counts[0], max_packets), d_offsets[i] is the exclusive prefix sum of carry over the n written
 * descriptors, d_offsets[n] = *d_total, and arena bytes [d_offsets[i], d_offsets[i+1]) are packet i;
 * nothing at or past min(total, payload_cap) is written. Then d_fill[s] = 0 for every downstream whose
 * packet is whole in the arena; one cut off by max_packets or by payload_cap keeps its fill (flush again
 * with more room: nothing is lost silently). SR_PAYLOAD_CAPACITY(0, n_downstreams) always suffices.
 * Asynchronous on the context's stream; no scratch, so the call can be captured in a graph.
 * n_downstreams <= SR_MAX_PACK_DOWNSTREAMS. Returns 0, -EINVAL (a null pointer where its room is not
 * 0), -EIO. */
int sr_flush_pending(sr_ctx *ctx, uint16_t *d_fill, const uint8_t *d_pend, sr_packet *d_packets,
                     size_t max_packets, uint64_t *d_counts, uint8_t *d_payload, size_t payload_cap,
                     uint32_t *d_offsets, uint64_t *d_total);

/* Developer and test knobs of one context (A/B runs and tests only; the library reads no environment
 * variable and no knob changes any record, packet or count, only which kernels produce them):
 *   SR_KNOB_LB_SPIN       polls of a predecessor tile's tail granules before route_chunk_kernel
 *                         computes the straddling line itself (default 65536; 0 always computes it);
 *   SR_KNOB_DEFER_PICKS   first picks the route kernel makes before deferring a probe when two or
 *                         more shards are dead (1 default, or 2);
 *   SR_KNOB_MTU_CHUNK     packing chunk lines: 0 = by the launch's shape (default), 2048 or 4608;
 *   SR_KNOB_MTU_XCD       1 (default): batches' packing chunks on one XCD from eight batches up;
 *   SR_KNOB_MTU_WALK      1 (default): the chain walked inside mtu_emit up to 64 shards; 0: mtu_chain;
 *   SR_KNOB_HIST          1 (default): sr_route_pack_many / sr_route_pack_* hand the route kernel's tile
 *                         histograms to the packing; 0: the packing counts the records itself;
 *   SR_KNOB_PREFETCH      tiles ahead (default 96; 0 off; up to 4096) whose 128-byte lines a chunk-layout
 *                         tile workgroup touches after issuing its own loads (an L2 / memory-side cache
 *                         warm-up for the tile its XCD runs later);
 *   SR_KNOB_FUSE_DEFER    1: a route + pack launch with two or more (at most 16) dead shards leaves its
 *                         deferred probes to the packing's counting pass; 0 (default): probe_defer_kernel
 *                         (measured level on C3 / C5, slower on C4).
 * Returns 0 or -EINVAL (unknown knob or value). */
#define SR_KNOB_LB_SPIN 1
#define SR_KNOB_DEFER_PICKS 2
#define SR_KNOB_MTU_CHUNK 3
#define SR_KNOB_MTU_XCD 4
#define SR_KNOB_MTU_WALK 5
#define SR_KNOB_HIST 7
#define SR_KNOB_PREFETCH 8
#define SR_KNOB_FUSE_DEFER 9
int sr_set_knob(sr_ctx *ctx, int knob, int64_t value);

/* Page-locked host memory for the batches and outputs of the host-memory calls (their copies then
 * run at full link rate). The device can also read it in place: it is what sr_route_pack_submit_slots
 * takes as `slots`. NULL on failure. */
void *sr_alloc_host(size_t bytes);
void sr_free_host(void *p);

/* Wait for all work enqueued by this context. */
int sr_sync(sr_ctx *ctx);

void sr_close(sr_ctx *ctx);

/* Version / build information string (static storage). */
const char *sr_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SR_ROUTE_H */
