// sr_route.hip — the C ABI of include/sr_route.h on MI355X (gfx950).
//
// Device code: route_kernel.hpp (one pass per batch: tokenise, validate, sdbm name hash, shard
// pick; reference sr-main.c:86-191). Host helpers: route_host.hpp. This file only adds the
// exported entry points, their argument checking and the host<->device copies of the
// host-memory variant.

#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <new>

#include "../../include/sr_route.h"
#include "coalesce_kernel.hpp"
#include "exchange.hpp"
#include "frame_host.hpp"
#include "frame_kernel.hpp"
#include "local_comm.hpp"
#include "log_kernel.hpp"
#include "mtu_kernel.hpp"
#include "owner_kernel.hpp"
#include "payload_kernel.hpp"
#include "regroup_kernel.hpp"
#include "route_host.hpp"
#include "rules_kernel.hpp"
#include "sample_kernel.hpp"
#include "stats_kernel.hpp"
#include "validate_kernel.hpp"

using namespace srk;

struct sr_ctx {
    int device;
    hipStream_t own_stream;
    hipStream_t stream;
    DeviceState ds;
    // buffers of the host-memory path (sr_route_batch)
    uint8_t *d_in;
    sr_record *d_out;
    size_t d_out_cap;
    uint64_t *d_hash;
    size_t d_hash_cap;
    uint64_t *d_count;
    uint64_t *d_probed;           // probed-dead bitmap of the host-memory path
    uint64_t *h_probed;           // its copy after the last sr_route_batch
    // scratch of sr_pack_by_owner
    uint2 *d_pack_tiles;          // tile counts | tile bases
    size_t pack_tiles_cap;        // entries per array
    uint64_t *d_owner_start;
    // scratch of sr_pack_packets (capacities: record tiles, chunks)
    uint32_t mtu_ntiles, mtu_chunks;
    uint32_t *d_mtu_tiles, *d_mtu_keys, *d_mtu_chunks;
    uint64_t *d_mtu_table;
    uint32_t *d_mtu_gp;    // per chunk: bytes per packet start (kMtuChunk u16), then the first prefix sums
    // sr_pack_owner_sizes / sr_pack_owner_scatter: the split sizes of the pack in progress, and where its
    // scatter wrote owner `own`'s chunk (sr_exchange_data then skips that chunk's copy)
    uint64_t *own_counts;
    uint64_t own_shape;   // key of that pack's batches and owners (pack_shape; the scatter must match)
    int own_set, own;
    uint8_t *own_bytes;
    sr_record *own_recs;
    // buffers of sr_route_pack_batch
    sr_record *d_sorted;
    size_t d_sorted_cap;
    sr_packet *d_packets;
    size_t d_packets_cap;
    uint16_t *d_fill;             // [3][nds]: two chained outputs, then the uploaded fill of a submission
    int fill_cur;                 // region of d_fill holding the last submission's output (0 or 1)
    uint64_t *d_mcounts;          // 3 u64
    // sr_owner_pack: the receive buffer's line total and the pending fills after the dead-downstream drop
    uint64_t *d_owner_n;
    uint16_t *d_owner_fill;       // [nds]
    uint32_t *d_frame;            // sr_frame_slots: kFrameMaxGroups sums | SR_MAX_SLOTS workgroup-local ends
    uint64_t *d_log;              // sr_format_log: {bytes, messages} per kLogRecs records of a full batch
    int trace;                    // sr_set_trace: submissions also return input-order records + hashes
    int payloads;                 // sr_set_payloads: submissions also return the packets' bytes
    // sr_set_logtext: submissions also return the batch's log text (log_level < 0: off)
    int logtext, log_level;
    size_t log_cap, log_msgs;     // the slots' text bytes and index entries
    uint32_t log_max_msg;
    uint32_t *d_ends;             // slot submissions at TRACE: the frame kernels' datagram ends (SR_MAX_SLOTS)
    StatsState stats;             // sr_stats_open: the name statistics' device state
    int name_stats;               // sr_set_name_stats: submissions also run sr_stats_update on the device
    CoalesceState coalesce;       // sr_coalesce_open: the coalescing stage's tables and scratch
    int coalesce_on;              // sr_set_coalesce: submissions coalesce between the route and the packing
    sr_record *d_cout;            // ... into these records (one per byte of the largest batch) ...
    uint64_t *d_ccounts;          // ... and these four counts
    RulesState rules;             // sr_rules_open: the name rules' table, hits and scratch
    int rules_on;                 // sr_set_name_rules: submissions run the rules between the route and the packing
    sr_record *d_rout;            // ... into these records (one per byte of the largest batch) ...
    size_t d_rout_cap;
    uint64_t *d_rhash;            // ... these hashes, when the coalescing follows ...
    size_t d_rhash_cap;
    uint64_t *d_rcounts;          // ... and these four counts
    ValidateStage validate;       // sr_validate_open: the line grammar's configuration, hits and scratch
    int validate_on;              // sr_set_validate: submissions run the grammar between the route and the name rules
    sr_record *d_vout;            // ... into these records (one per byte of the largest batch) ...
    size_t d_vout_cap;
    uint64_t *d_vhash;            // ... these hashes, when the coalescing follows ...
    size_t d_vhash_cap;
    uint64_t *d_vcounts;          // ... and these four counts
    SampleStage sample;           // sr_sample_open: the sample-rate stage's table, hits and scratch
    int sample_on;                // sr_set_sample: submissions thin hot names between the name rules and the coalescing
    sr_record *d_sout;            // ... into these records (one per byte of the largest batch) ...
    size_t d_sout_cap;
    uint64_t *d_shash;            // ... these hashes, when the coalescing follows ...
    size_t d_shash_cap;
    uint64_t *d_scounts;          // ... and these four counts
    uint64_t sample_subs;         // submissions accepted since sr_set_sample: the next one's seed_add
    size_t d_in_cap;              // d_in's bytes once a switch has allocated it again (0: max_batch)
    // packing knobs (sr_set_knob): forced chunk lines (0: by shape), XCD-local chunks, chain walked in emit
    uint32_t mtu_chunk;
    int mtu_xcd, mtu_walk;
    int hist;                     // SR_KNOB_HIST: route + pack launches hand the tiles' histograms over
    int fuse_defer;               // SR_KNOB_FUSE_DEFER: the counting pass runs the route launch's deferred probes
    // page-locked, device-mapped outputs of sr_route_pack_submit: slots 0 and 1, slot 2 is
    // sr_route_pack_batch's own
    struct Slot {
        uint8_t *host;            // one allocation: records | packets | fill out | probed | counts | fill in
        uint8_t *dev;             // its device-mapped address
        size_t rec_cap, pk_cap;
        hipEvent_t done;
        int busy;                 // submitted, result not taken
        sr_record *sorted;
        sr_packet *packets;
        uint16_t *fill, *fill_in;
        uint64_t *probed, *counts;   // counts[3]: the framed total the device found (slot submissions)
        uint16_t *lens_in;        // sr_route_pack_submit_slots: the staged datagram lengths (SR_MAX_SLOTS)
        int framed;               // the batch in the slot was framed on the device ...
        uint64_t frame_bytes;     // ... and the host expects this many framed bytes
        // sr_set_trace: input-order records and per-line hashes (one more page-locked allocation)
        uint8_t *thost, *tdev;
        size_t trec_cap;
        int traced;               // the batch in the slot was submitted with trace on
        // sr_set_payloads: the packets' bytes, their offsets and the total (one more page-locked allocation)
        uint8_t *phost, *pdev;
        size_t pay_cap, poff_cap; // arena bytes; offsets - 1 (descriptors)
        int payloaded;            // the batch in the slot was submitted with payloads on
        // sr_set_coalesce: merged text | {4 counts, input records} (one more page-locked allocation)
        uint8_t *chost, *cdev;
        size_t ctext_cap;
        int coalesced;            // the batch in the slot was submitted with the coalescing on
        // sr_set_name_rules: {4 counts, input records} (one more page-locked allocation)
        uint64_t *rhost, *rdev;
        int ruled;                // the batch in the slot was submitted with the name rules on
        // sr_set_validate: {4 counts, input records} (one more page-locked allocation)
        uint64_t *vhost, *vdev;
        int validated;            // the batch in the slot was submitted with the line grammar on
        // sr_set_sample: rewritten text | {4 counts, input records} (one more page-locked allocation)
        uint8_t *shost, *sdev;
        size_t stext_cap;
        int sampled;              // the batch in the slot was submitted with the sample rates on ...
        uint64_t sseed;           // ... under this seed (the configuration's + seed_add)
        // sr_set_logtext: text | offsets | levels | {total, messages} | staged prefixes | staged ends
        uint8_t *lhost, *ldev;
        size_t ltext_cap, lmsg_cap;
        uint32_t stage_plen[2];   // sr_route_pack_set_prefix, for the next submission
        size_t stage_ends;        // sr_route_pack_set_ends, for the next submission
        int logged;               // the batch in the slot was submitted with the log text on
    } slot[3];
};

static void free_ptr(void *p) { (void)hipFree(p); }

#ifndef SR_CHUNK_ABL
#define SR_CHUNK_ABL 0u   // developer ablation builds of route_chunk_kernel only (chunk_kernel.hpp)
#endif

// The product launches KV_UNIFORM, KV_SEGMENTS or KV_CHUNKS (identical records;
// DeviceState::choose_segments picks by the lane-layout policy). Ablation variants (records wrong by design in some of them)
// exist only in builds made with -DSR_ABLATION_VARIANTS (`make VARIANTS=1`, developer A/B runs;
// never the shipped library): SR_VARIANT in the environment then selects one.
static int launch_product(DeviceState &ds, const RouteParams &p, hipStream_t stream) {
    const bool seg = ds.choose_segments(stream);
    if (ds.last_layout == SR_LAYOUT_CHUNKS) {
        if (ds.dead == 0) return launch_route<KV_CHUNKS | KV_ALIVE | SR_CHUNK_ABL>(ds, p, stream);
        return launch_route<KV_CHUNKS | SR_CHUNK_ABL>(ds, p, stream);
    }
    if (ds.dead == 0) {   // every shard alive: the variants without the probe
        if (seg) return launch_route<KV_SEGMENTS | KV_ALIVE>(ds, p, stream);
        return launch_route<KV_UNIFORM | KV_ALIVE>(ds, p, stream);
    }
    if (seg) return launch_route<KV_SEGMENTS | KV_PICKS>(ds, p, stream);
    return launch_route<KV_UNIFORM | KV_PICKS>(ds, p, stream);
}
#ifdef SR_ABLATION_VARIANTS
static int launch_variant(DeviceState &ds, const RouteParams &p, hipStream_t stream) {
    static const int v = [] {
        const char *e = getenv("SR_VARIANT");
        if (!e || !*e) return 0;
        if (!strcmp(e, "no_mid_base")) return 14;
        // upper bounds, not routing (records wrong or missing; line counts still exact)
        if (!strcmp(e, "fake_base")) return 7;
        if (!strcmp(e, "no_hash")) return 8;
        if (!strcmp(e, "no_lines")) return 9;
        return 0;
    }();
    switch (v) {
    case 14: return launch_route<ABL_NO_MID_BASE>(ds, p, stream);
    case 7: return launch_route<ABL_FAKE_BASE>(ds, p, stream);
    case 8: return launch_route<ABL_NO_HASH>(ds, p, stream);
    case 9: return launch_route<ABL_NO_LINES>(ds, p, stream);
    default: return launch_product(ds, p, stream);
    }
}
#else
static int launch_variant(DeviceState &ds, const RouteParams &p, hipStream_t stream) {
    return launch_product(ds, p, stream);
}
#endif

extern "C" {

size_t sr_frame_datagram(uint8_t *dst, const uint8_t *src, size_t len) {
    // udp_read_cb: recv(fd, buffer, DATA_BUF_SIZE - 1, 0) (sr-main.c:163), then append '\n'
    // unless the datagram already ends with one (sr-main.c:171-173). Empty -> nothing (:170).
    size_t n = len < SR_MAX_DATAGRAM ? len : SR_MAX_DATAGRAM;
    if (n == 0) return 0;
    memcpy(dst, src, n);
    if (dst[n - 1] != '\n') dst[n++] = '\n';
    return n;
}

size_t sr_frame_datagrams(uint8_t *dst, size_t dst_cap, const uint8_t *const *dgrams, const size_t *lens,
                          size_t count) {
    size_t pos = 0;
    for (size_t i = 0; i < count; ++i) {
        const size_t need = (lens[i] < SR_MAX_DATAGRAM ? lens[i] : SR_MAX_DATAGRAM) + 1;
        if (pos + need > dst_cap) return (size_t)-1;
        pos += sr_frame_datagram(dst + pos, dgrams[i], lens[i]);
    }
    return pos;
}

size_t sr_frame_slots_size(const uint8_t *slots, size_t stride, const uint16_t *lens, size_t count, uint32_t *ends) {
    if (count && (!slots || !lens)) return 0;
    return frame_slots_size(slots, stride, lens, count, ends);
}

void *sr_alloc_host(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void sr_free_host(void *p) {
    if (p) (void)hipHostFree(p);
}

const char *sr_version(void) {
    return "statsd-router-mi355x 0.5 (gfx950 route_kernel: 16 KiB tiles x 256 threads, per-batch scanners, up to 32 batches per launch)";
}

void sr_close(sr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->ds.release();
    (void)hipFree(c->d_in);
    (void)hipFree(c->d_out);
    (void)hipFree(c->d_hash);
    (void)hipFree(c->d_count);
    (void)hipFree(c->d_probed);
    free(c->h_probed);
    (void)hipFree(c->d_pack_tiles);
    (void)hipFree(c->d_owner_start);
    free_ptr(c->d_mtu_tiles);
    free_ptr(c->d_mtu_keys);
    free_ptr(c->d_mtu_chunks);
    free_ptr(c->d_mtu_table);
    free_ptr(c->d_mtu_gp);
    free_ptr(c->d_sorted);
    free_ptr(c->d_packets);
    free_ptr(c->d_fill);
    free_ptr(c->d_mcounts);
    free_ptr(c->d_owner_n);
    free_ptr(c->d_owner_fill);
    free_ptr(c->d_frame);
    free_ptr(c->d_log);
    free_ptr(c->d_ends);
    free_ptr(c->stats.d_base);
    free_ptr(c->coalesce.d_table);
    free_ptr(c->coalesce.d_scratch);
    free_ptr(c->coalesce.d_tiles);
    free_ptr(c->d_cout);
    free_ptr(c->d_ccounts);
    free_ptr(c->rules.d_table);
    free_ptr(c->rules.d_hits);
    free_ptr(c->rules.d_match);
    free_ptr(c->rules.d_tiles);
    free_ptr(c->d_rout);
    free_ptr(c->d_rhash);
    free_ptr(c->d_rcounts);
    free_ptr(c->validate.d_hits);
    free_ptr(c->validate.d_reason);
    free_ptr(c->validate.d_tiles);
    free_ptr(c->sample.d_table);
    free_ptr(c->sample.d_hits);
    free_ptr(c->sample.d_scratch);
    free_ptr(c->sample.d_tiles);
    free_ptr(c->d_sout);
    free_ptr(c->d_shash);
    free_ptr(c->d_scounts);
    free_ptr(c->d_vout);
    free_ptr(c->d_vhash);
    free_ptr(c->d_vcounts);
    for (auto &sl : c->slot) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.thost) (void)hipHostFree(sl.thost);
        if (sl.phost) (void)hipHostFree(sl.phost);
        if (sl.lhost) (void)hipHostFree(sl.lhost);
        if (sl.chost) (void)hipHostFree(sl.chost);
        if (sl.rhost) (void)hipHostFree(sl.rhost);
        if (sl.vhost) (void)hipHostFree(sl.vhost);
        if (sl.shost) (void)hipHostFree(sl.shost);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    free(c);
}

int sr_open(sr_ctx **out, int device, size_t max_batch_bytes, uint32_t n_downstreams) {
    if (!out) return -EINVAL;
    *out = nullptr;
    if (max_batch_bytes == 0 || max_batch_bytes > 0xFFFFFFF0ull || n_downstreams > SR_MAX_DOWNSTREAMS)
        return -EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
    if (hipSetDevice(device) != hipSuccess) return -ENODEV;
    sr_ctx *c = (sr_ctx *)calloc(1, sizeof(sr_ctx));
    if (!c) return -ENOMEM;
    new (&c->ds) DeviceState();
    c->device = device;
    c->mtu_xcd = 1;
    c->mtu_walk = 1;
    c->hist = 1;
    c->fuse_defer = 0;   // measured level or slower (C4: too few counting waves): profiles/r05/fused_deferral_ab_r5r.jsonl
    int rc = -ENOMEM;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) goto fail;
    c->stream = c->own_stream;
    if ((rc = c->ds.init(max_batch_bytes, n_downstreams)) != 0) goto fail;
    rc = -ENOMEM;
    if (hipMalloc(&c->d_in, max_batch_bytes) != hipSuccess) goto fail;
    if (hipMalloc(&c->d_count, sizeof(uint64_t)) != hipSuccess) goto fail;
    if (hipMalloc(&c->d_probed, (c->ds.nwords ? c->ds.nwords : 1) * sizeof(uint64_t)) != hipSuccess) goto fail;
    if (!(c->h_probed = (uint64_t *)calloc(c->ds.nwords ? c->ds.nwords : 1, sizeof(uint64_t)))) goto fail;
    *out = c;
    return 0;
fail:
    sr_close(c);
    return rc;
}

int sr_set_alive(sr_ctx *c, const uint64_t *alive) {
    if (!c || (!alive && c->ds.nds)) return -EINVAL;
    (void)hipSetDevice(c->device);
    return c->ds.set_alive(alive, c->stream);
}

int sr_set_stream(sr_ctx *c, void *stream) {
    if (!c) return -EINVAL;
    c->stream = stream ? (hipStream_t)stream : c->own_stream;
    return 0;
}

int sr_set_layout(sr_ctx *c, int layout) {
    if (!c || layout < SR_LAYOUT_AUTO || layout > SR_LAYOUT_CHUNKS) return -EINVAL;
    c->ds.layout_mode = layout;
    return 0;
}

int sr_last_layout(const sr_ctx *c) { return c ? c->ds.last_layout : -EINVAL; }
int sr_last_hash_engine(const sr_ctx *c) { return c ? c->ds.last_hash_engine : -EINVAL; }

int sr_set_knob(sr_ctx *c, int knob, int64_t v) {
    if (!c) return -EINVAL;
    switch (knob) {
    case SR_KNOB_LB_SPIN:
        if (v < 0 || v > 0xFFFFFFFFll) return -EINVAL;
        c->ds.lb_spin = (uint32_t)v;
        return 0;
    case SR_KNOB_FUSE_DEFER:
        if (v != 0 && v != 1) return -EINVAL;
        c->fuse_defer = (int)v;
        return 0;
    case SR_KNOB_PREFETCH:
        if (v < 0 || v > 4096) return -EINVAL;
        c->ds.prefetch = (uint32_t)v;
        return 0;
    case SR_KNOB_DEFER_PICKS:
        if (v != 1 && v != 2) return -EINVAL;
        c->ds.defer_picks = (uint32_t)v;
        return 0;
    case SR_KNOB_MTU_CHUNK:
        if (v != 0 && v != kMtuChunkSmall && v != kMtuChunk) return -EINVAL;
        c->mtu_chunk = (uint32_t)v;
        return 0;
    case SR_KNOB_MTU_XCD:
    case SR_KNOB_MTU_WALK:
    case SR_KNOB_HIST:
        if (v != 0 && v != 1) return -EINVAL;
        (knob == SR_KNOB_MTU_XCD ? c->mtu_xcd : knob == SR_KNOB_MTU_WALK ? c->mtu_walk : c->hist) = (int)v;
        return 0;
    default:
        return -EINVAL;
    }
}

int sr_set_trace(sr_ctx *c, int on) {
    if (!c) return -EINVAL;
    c->trace = on ? 1 : 0;
    return 0;
}

int sr_set_payloads(sr_ctx *c, int on) {
    if (!c) return -EINVAL;
    c->payloads = on ? 1 : 0;
    return 0;
}

int sr_sync(sr_ctx *c) {
    if (!c) return -EINVAL;
    (void)hipSetDevice(c->device);
    return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : -EIO;
}

int sr_last_probed_dead(const sr_ctx *c, uint64_t *bitmap) {
    if (!c || (!bitmap && c->ds.nwords)) return -EINVAL;
    if (c->ds.nwords) memcpy(bitmap, c->h_probed, c->ds.nwords * sizeof(uint64_t));
    return 0;
}

int sr_route_device(sr_ctx *c, const uint8_t *d_bytes, size_t nbytes, sr_record *d_out, size_t max_records,
                    uint64_t *d_hashes, uint64_t *d_n_records) {
    if (!c || !d_n_records || (nbytes && !d_bytes) || nbytes > c->ds.max_batch) return -EINVAL;
    if (max_records && !d_out) return -EINVAL;
    (void)hipSetDevice(c->device);
    const RouteParams p = c->ds.params(d_bytes, nbytes, d_out, max_records, d_hashes, d_n_records);
    return launch_variant(c->ds, p, c->stream);
}

int sr_route_device_many(sr_ctx *c, const sr_batch *batches, size_t count) {
    static_assert(SR_MAX_BATCHES_PER_LAUNCH == (unsigned)kMaxBatches, "launch batch limit");
    if (!c || (count && !batches)) return -EINVAL;
    for (size_t i = 0; i < count; ++i) {
        const sr_batch &b = batches[i];
        if (!b.d_n_records || (b.nbytes && !b.d_bytes) || b.nbytes > c->ds.max_batch) return -EINVAL;
        if (b.max_records && !b.d_out) return -EINVAL;
    }
    (void)hipSetDevice(c->device);
    for (size_t i0 = 0; i0 < count; i0 += kMaxBatches) {
        RouteParams p = c->ds.params();
        for (size_t i = i0; i < count && i < i0 + kMaxBatches; ++i)
            DeviceState::add_batch(p, batches[i].d_bytes, batches[i].nbytes, batches[i].d_out, batches[i].max_records,
                                   batches[i].d_hashes, batches[i].d_n_records, batches[i].d_probed_dead);
        const int rc = launch_variant(c->ds, p, c->stream);
        if (rc) return rc;
    }
    return 0;
}

// The owner pack's tile: 256 records per chunk, two chunks per tile when the pack's lines are short,
// one when they are long (more than 192 bytes per record slot on average: C5's mixed lines, C3, C4).
// Every call with the same batches picks the same (sr_pack_owner_sizes and _scatter share the tiles).
static int pack_chunks_for(const PackBatch *in, uint32_t nb) {
    uint64_t bytes = 0, recs = 0;
    for (uint32_t j = 0; j < nb; ++j) {
        bytes += in[j].nbytes;
        recs += in[j].max_records;
    }
    return bytes > 192ull * (recs ? recs : 1) ? 1 : kPackMaxChunks;
}

// The owner pack: kPackSizes = count + scan (the split sizes into d_owner_counts), kPackScatter =
// the lines and records (owner `own` into own_bytes / own_recs when own >= 0)
enum : int { kPackSizes = 1, kPackScatter = 2 };
static int pack_launch(sr_ctx *c, const PackBatch *in, uint32_t nb, uint32_t n_owners, uint8_t *d_out_bytes,
                       size_t out_cap, sr_record *d_out_recs, uint64_t *d_owner_counts, int phases = kPackSizes | kPackScatter,
                       int own = -1, uint8_t *own_bytes = nullptr, sr_record *own_recs = nullptr) {
    PackParams p;
    memset(&p, 0, sizeof(p));
    const int ch = pack_chunks_for(in, nb);
    const uint32_t tile = (uint32_t)(kPackBlock * ch);
    uint32_t ntiles = 0;
    for (uint32_t j = 0; j < nb; ++j) {
        p.b[j] = in[j];
        p.b[j].tile0 = ntiles;
        ntiles += (in[j].max_records + tile - 1) / tile;
    }
    p.nb = nb ? nb : 1;
    p.n_owners = n_owners;
    p.ntiles = ntiles;
    const size_t need = (size_t)(ntiles ? ntiles : 1) * n_owners;
    if (need > c->pack_tiles_cap) {
        (void)hipFree(c->d_pack_tiles);
        c->d_pack_tiles = nullptr;
        c->pack_tiles_cap = 0;
        if (hipMalloc(&c->d_pack_tiles, 2 * need * sizeof(uint2)) != hipSuccess) return -ENOMEM;
        c->pack_tiles_cap = need;
    }
    if (!c->d_owner_start && hipMalloc(&c->d_owner_start, 2 * SR_MAX_OWNERS * sizeof(uint64_t)) != hipSuccess)
        return -ENOMEM;
    p.tile_counts = c->d_pack_tiles;
    p.tile_base = c->d_pack_tiles + c->pack_tiles_cap;
    p.owner_start = c->d_owner_start;
    p.owner_counts = d_owner_counts;
    p.out_bytes = d_out_bytes;
    p.out_cap = out_cap;
    p.out_recs = d_out_recs;
    p.own = own;
    p.own_bytes = own_bytes;
    p.own_recs = own_recs;
    if ((phases & kPackSizes) && ntiles) {
        const dim3 grid((ntiles + kCountTiles - 1) / kCountTiles);
        if (ch == 1) hipLaunchKernelGGL(pack_count_kernel<1>, grid, dim3(kPackBlock), 0, c->stream, p);
        else hipLaunchKernelGGL(pack_count_kernel<kPackMaxChunks>, grid, dim3(kPackBlock), 0, c->stream, p);
        if (hipGetLastError() != hipSuccess) return -EIO;
    }
    if (phases & kPackSizes) {
        hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(1024), 0, c->stream, p);
        if (hipGetLastError() != hipSuccess) return -EIO;
    }
    if ((phases & kPackScatter) && ntiles) {
        if (ch == 1) hipLaunchKernelGGL(pack_scatter_kernel<1>, dim3(ntiles), dim3(kPackBlock), 0, c->stream, p);
        else hipLaunchKernelGGL(pack_scatter_kernel<kPackMaxChunks>, dim3(ntiles), dim3(kPackBlock), 0, c->stream, p);
        if (hipGetLastError() != hipSuccess) return -EIO;
    }
    return 0;
}

int sr_pack_by_owner(sr_ctx *c, const uint8_t *d_bytes, size_t nbytes, const sr_record *d_recs,
                     const uint64_t *d_n_records, size_t max_records, uint32_t n_owners, uint8_t *d_out_bytes,
                     size_t out_cap, sr_record *d_out_recs, uint64_t *d_owner_counts) {
    if (!c || !d_n_records || !d_owner_counts || n_owners == 0 || n_owners > SR_MAX_OWNERS) return -EINVAL;
    // the packed layout is addressed with u32 offsets: its worst case must fit 32 bits, and the
    // caller's buffer must hold that worst case (the kernels never truncate silently)
    if (max_records > 0xFFFFFFFFull || SR_PACK_CAPACITY((uint64_t)nbytes) > 0xFFFFFFFFull) return -EINVAL;
    if (out_cap < SR_PACK_CAPACITY((uint64_t)nbytes)) return -EINVAL;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    if (max_records && (!d_recs || !d_out_recs || !d_bytes || !d_out_bytes)) return -EINVAL;
    (void)hipSetDevice(c->device);
    PackBatch b{d_bytes, d_recs, d_n_records, (uint32_t)nbytes, (uint32_t)max_records, 0, 0};
    c->own_set = 0;
    c->own_counts = nullptr;
    return pack_launch(c, &b, 1, n_owners, d_out_bytes, out_cap, d_out_recs, d_owner_counts);
}

// The key sr_pack_owner_scatter must match: the batch descriptors (pointers, sizes) and owners of the
// context's last sr_pack_owner_sizes, whose tile bases and split sizes the scatter uses (FNV-1a)
static uint64_t pack_shape(const PackBatch *in, size_t count, uint32_t n_owners) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&h](uint64_t v) {
        for (int i = 0; i < 8; ++i, v >>= 8) h = (h ^ (v & 0xFFu)) * 0x100000001b3ull;
    };
    mix(n_owners);
    mix(count);
    for (size_t j = 0; j < count; ++j) {
        mix((uint64_t)(uintptr_t)in[j].bytes);
        mix((uint64_t)(uintptr_t)in[j].recs);
        mix((uint64_t)(uintptr_t)in[j].n_records);
        mix((uint64_t)in[j].nbytes << 32 | in[j].max_records);
    }
    return h;
}

static int pack_many_args(const sr_batch *batches, size_t count, uint32_t n_owners, PackBatch *in,
                          uint64_t *total_bytes) {
    if (n_owners == 0 || n_owners > SR_MAX_OWNERS) return -EINVAL;
    if (count == 0 || count > SR_MAX_BATCHES_PER_LAUNCH || !batches) return -EINVAL;
    *total_bytes = 0;
    for (size_t j = 0; j < count; ++j) {
        const sr_batch &b = batches[j];
        if (!b.d_n_records || b.max_records > 0xFFFFFFFFull || b.nbytes > 0xFFFFFFF0ull) return -EINVAL;
        if (b.max_records && (!b.d_out || !b.d_bytes)) return -EINVAL;
        *total_bytes += b.nbytes;
        in[j] = PackBatch{b.d_bytes, b.d_out, b.d_n_records, (uint32_t)b.nbytes, (uint32_t)b.max_records, 0, 0};
    }
    return SR_PACK_CAPACITY(*total_bytes) > 0xFFFFFFFFull ? -EINVAL : 0;
}

int sr_pack_many_by_owner(sr_ctx *c, const sr_batch *batches, size_t count, uint32_t n_owners, uint8_t *d_out_bytes,
                          size_t out_cap, sr_record *d_out_recs, uint64_t *d_owner_counts) {
    if (!c || !d_owner_counts) return -EINVAL;
    uint64_t total_bytes = 0;
    PackBatch in[kPackMaxBatches];
    int rc = pack_many_args(batches, count, n_owners, in, &total_bytes);
    if (rc) return rc;
    if (out_cap < SR_PACK_CAPACITY(total_bytes)) return -EINVAL;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    if (!d_out_bytes || !d_out_recs) return -EINVAL;
    (void)hipSetDevice(c->device);
    c->own_set = 0;
    c->own_counts = nullptr;
    return pack_launch(c, in, (uint32_t)count, n_owners, d_out_bytes, out_cap, d_out_recs, d_owner_counts);
}

int sr_pack_owner_sizes(sr_ctx *c, const sr_batch *batches, size_t count, uint32_t n_owners, uint64_t *d_owner_counts) {
    if (!c || !d_owner_counts) return -EINVAL;
    uint64_t total_bytes = 0;
    PackBatch in[kPackMaxBatches];
    int rc = pack_many_args(batches, count, n_owners, in, &total_bytes);
    if (rc) return rc;
    (void)hipSetDevice(c->device);
    c->own_set = 0;
    c->own_counts = d_owner_counts;
    c->own_shape = pack_shape(in, count, n_owners);
    rc = pack_launch(c, in, (uint32_t)count, n_owners, nullptr, 0, nullptr, d_owner_counts, kPackSizes);
    if (rc) c->own_counts = nullptr;
    return rc;
}

int sr_pack_owner_scatter(sr_ctx *c, const sr_batch *batches, size_t count, uint32_t n_owners, int own,
                          uint8_t *d_own_bytes, sr_record *d_own_recs, uint8_t *d_out_bytes, size_t out_cap,
                          sr_record *d_out_recs) {
    if (!c || !c->own_counts || own < -1 || own >= (int)n_owners) return -EINVAL;
    uint64_t total_bytes = 0;
    PackBatch in[kPackMaxBatches];
    int rc = pack_many_args(batches, count, n_owners, in, &total_bytes);
    if (rc) return rc;
    if (pack_shape(in, count, n_owners) != c->own_shape) return -EINVAL;
    if (out_cap < SR_PACK_CAPACITY(total_bytes)) return -EINVAL;
    if (out_cap > 0xFFFFFFFFull) out_cap = 0xFFFFFFFFull;
    if (!d_out_bytes || !d_out_recs) return -EINVAL;
    if (own >= 0 && (!d_own_bytes || !d_own_recs || ((uintptr_t)d_own_bytes & 3u))) return -EINVAL;
    (void)hipSetDevice(c->device);
    // sr_exchange_data finds the own chunk in place and does not copy it
    c->own_set = own >= 0;
    c->own = own;
    c->own_bytes = d_own_bytes;
    c->own_recs = d_own_recs;
    return pack_launch(c, in, (uint32_t)count, n_owners, d_out_bytes, out_cap, d_out_recs, c->own_counts, kPackScatter,
                       own, d_own_bytes, d_own_recs);
}

// Scratch of the packing kernels for one launch (grown, never shrunk; not in stream capture).
static int mtu_reserve(sr_ctx *c, uint32_t tiles, uint32_t chunks, uint32_t nb) {
    const uint32_t nds = c->ds.nds;
    if (tiles > c->mtu_ntiles) {
        free_ptr(c->d_mtu_tiles);
        c->d_mtu_tiles = nullptr;
        c->mtu_ntiles = 0;
        if (hipMalloc(&c->d_mtu_tiles, (size_t)(nds + 1) * tiles * sizeof(uint32_t)) != hipSuccess) return -ENOMEM;
        c->mtu_ntiles = tiles;
    }
    if (!c->d_mtu_keys) {   // keys and closed counts for the most batches a launch can hold
        const size_t words = (size_t)kMtuMaxBatches * (2 * (size_t)nds + 4) + (size_t)kMtuMaxBatches * nds;
        if (hipMalloc(&c->d_mtu_keys, words * sizeof(uint32_t)) != hipSuccess) return -ENOMEM;
    }
    (void)nb;
    if (chunks > c->mtu_chunks) {
        free_ptr(c->d_mtu_chunks);
        free_ptr(c->d_mtu_table);
        free_ptr(c->d_mtu_gp);
        c->d_mtu_chunks = nullptr;
        c->d_mtu_table = nullptr;
        c->d_mtu_gp = nullptr;
        c->mtu_chunks = 0;
        // shard, entry, open, first descriptor per chunk
        if (hipMalloc(&c->d_mtu_chunks, 4 * (size_t)chunks * sizeof(uint32_t)) != hipSuccess) return -ENOMEM;
        // the tables, then next(i) - i of every line of every chunk
        if (hipMalloc(&c->d_mtu_table, (size_t)chunks * (kMtuX * sizeof(uint64_t) + kMtuChunk) + 16) != hipSuccess)
            return -ENOMEM;
        if (hipMalloc(&c->d_mtu_gp, (size_t)chunks * (kMtuChunk * sizeof(uint16_t) + (kMtuP0 + 1) * sizeof(uint32_t))) !=
            hipSuccess)
            return -ENOMEM;
        c->mtu_chunks = chunks;
    }
    return 0;
}

#ifdef SR_MTU_STAMPS
static uint64_t *g_mtu_dbg = nullptr;
static size_t g_mtu_dbg_n = 0;
extern "C" size_t sr_mtu_stamps(uint64_t *dst, size_t max_chunks) {
    const size_t n = g_mtu_dbg_n < max_chunks ? g_mtu_dbg_n : max_chunks;
    if (g_mtu_dbg && n) (void)hipMemcpy(dst, g_mtu_dbg, n * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    return n;
}
#endif

// hist (group mode): the key histograms of the route kernel's tiles for these batches, written by the
// context's last route launch (RouteParams::hist); route_bytes: each batch's bytes in that launch
// (its tiles: ceil(bytes / 16 KiB), numbered in batch order as launch_route numbers them)
static int pack_many_impl(sr_ctx *c, const sr_pack_batch *batches, size_t count, uint32_t *hist,
                          const size_t *route_bytes, bool fused = false, const uint64_t *tile_pd = nullptr) {
    if (!c || !batches || count == 0 || count > (size_t)kMtuMaxBatches) return -EINVAL;
    const uint32_t nds = c->ds.nds;
    if (nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    MtuLaunch L;
    memset(&L, 0, sizeof(L));
    // Chunk size: a shard's chunks are composed one after another (mtu_chain), so few shards with
    // many lines each want long chunks; many shards (short chains) want more, smaller chunks in
    // flight (2048 lines: 16 KiB of LDS per table workgroup, ten per CU instead of five).
    uint64_t all_records = 0;
    for (size_t j = 0; j < count; ++j) all_records += batches[j].max_records;
    uint32_t ch = all_records <= (uint64_t)(nds ? nds : 1) * 32u * kMtuChunk ? (uint32_t)kMtuChunkSmall
                                                                            : (uint32_t)kMtuChunk;
    if (c->mtu_chunk) ch = c->mtu_chunk;   // SR_KNOB_MTU_CHUNK (A/B runs)
    uint32_t tiles = 0, chunks = 0, groups = 0;
    constexpr uint32_t kGroup = 8;   // route tiles per scatter wave (C2: 2048 records, C4: 128)
    for (size_t j = 0; j < count; ++j) {
        const sr_pack_batch &b = batches[j];
        if (!b.d_n_records || !b.d_counts || (nds && !b.d_fill_out) || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if (b.max_records && (!b.d_recs || !b.d_sorted)) return -EINVAL;
        if (b.max_packets && !b.d_packets) return -EINVAL;
        MtuBatchArg &a = L.b[j];
        a.recs = b.d_recs;
        a.n_records = b.d_n_records;
        a.fill_in = b.d_fill_in;
        a.probed_dead = b.d_probed_dead;
        a.sorted = b.d_sorted;
        a.packets = b.d_packets;
        a.counts = b.d_counts;
        a.fill_out = b.d_fill_out;
        a.max_records = (uint32_t)b.max_records;
        a.max_packets = (uint32_t)(b.max_packets > 0xFFFFFFFFull ? 0xFFFFFFFFull : b.max_packets);
        a.tile0 = tiles;
        a.chunk0 = chunks;
        if (hist) {   // the route launch's tiles of this batch
            const uint32_t nt = (uint32_t)((route_bytes[j] + 16383) / 16384);
            a.grp0 = groups;
            groups += (nt + kGroup - 1) / kGroup;
            tiles += nt;
        } else {
            const uint64_t nt = (b.max_records + kMtuTile - 1) / kMtuTile;
            tiles += (uint32_t)(nt ? nt : 1);
        }
        chunks += (uint32_t)((b.max_records + ch - 1) / ch) + nds + 1;
    }
    (void)hipSetDevice(c->device);
    int rc = mtu_reserve(c, hist ? 0u : tiles, chunks, (uint32_t)count);
    if (rc) return rc;
    L.nds = nds;
    L.group = hist ? kGroup : 0u;
    L.groups = groups;
    L.nb = (uint32_t)count;
    L.tiles = tiles;
    L.chunks = chunks;
    L.chunk_lines = ch;
    L.tile_counts = hist ? hist : c->d_mtu_tiles;
    L.keys = c->d_mtu_keys;
    L.closed = c->d_mtu_keys + (size_t)kMtuMaxBatches * (2 * (size_t)nds + 4);
    L.chunk_shard = c->d_mtu_chunks;
    L.chunk_entry = c->d_mtu_chunks + (size_t)chunks;
    L.chunk_open = c->d_mtu_chunks + 2 * (size_t)chunks;
    L.chunk_pk = c->d_mtu_chunks + 3 * (size_t)chunks;
    L.table = c->d_mtu_table;
    L.nx = reinterpret_cast<uint8_t *>(c->d_mtu_table + (((size_t)c->mtu_chunks * kMtuX + 1) & ~(size_t)1));
    L.plen = reinterpret_cast<uint16_t *>(c->d_mtu_gp);
    // group mode after a one-dead-shard launch: mtu_scan ORs the route tiles' probed-dead slots
    L.tile_pd = hist ? tile_pd : nullptr;
    L.pd_words = c->ds.nwords;
    L.gp0 = c->d_mtu_gp + (size_t)c->mtu_chunks * kMtuChunk / 2;
    if (fused) {   // the route launch's deferred probes, run by the counting pass
        if (hist) return -EIO;
        const DeviceState &ds = c->ds;
        L.probe = ProbeArgs{ds.nds, ds.dead, 2u, 0u, ds.magic_n, ds.d_alive, ds.d_magic};
        L.fd_mark = ds.fd_mark;
        L.nwords = ds.nwords;
        for (size_t j = 0; j < count; ++j) L.b[j].dhash = ds.fd_dhash[j];
    }
#ifdef SR_MTU_STAMPS   // developer timeline: 8 stamps per chunk, read back with sr_mtu_stamps
    static uint64_t *d_dbg = nullptr;
    static size_t dbg_cap = 0;
    if (chunks > dbg_cap) {
        if (d_dbg) (void)hipFree(d_dbg);
        dbg_cap = chunks;
        if (hipMalloc(&d_dbg, dbg_cap * 8 * sizeof(uint64_t)) != hipSuccess) return -ENOMEM;
    }
    (void)hipMemsetAsync(d_dbg, 0, (size_t)chunks * 8 * sizeof(uint64_t), c->stream);
    L.dbg = d_dbg;
    g_mtu_dbg = d_dbg;
    g_mtu_dbg_n = chunks;
#else
    L.dbg = nullptr;
#endif
    // the chunk kernels' grid: eight batches or more put each batch's chunks on one XCD
    // (mtu_chunk_slot): eight times the most slots any XCD takes
    uint32_t chunk_grid = chunks;
    L.xcd = (c->mtu_xcd && count >= 8) ? 1u : 0u;   // SR_KNOB_MTU_XCD 0: chunks dealt in launch order
    if (L.xcd) {
        uint32_t per[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx = 0;
        for (size_t j = 0; j < count; ++j) {
            const uint32_t s1 = j + 1 < count ? L.b[j + 1].chunk0 : chunks;
            per[j & 7] += s1 - L.b[j].chunk0;
        }
        for (int x = 0; x < 8; ++x) mx = per[x] > mx ? per[x] : mx;
        chunk_grid = 8 * mx;
    }
    const size_t sort_lds = (size_t)kMtuSortWaves * (nds + 1) * sizeof(uint32_t);
    // up to 4 x 4097 counters: past the 64 KiB default
    ensure_dyn_lds((const void *)mtu_count_kernel<false>, 96 * 1024);
    ensure_dyn_lds((const void *)mtu_count_kernel<true>, 64 * 1024);
    ensure_dyn_lds((const void *)mtu_scatter_kernel, 96 * 1024);
    if (hist) {   // the route kernel counted the keys: scan its tiles' histograms, scatter by groups of tiles
        ensure_dyn_lds((const void *)mtu_scatter_groups_kernel, 96 * 1024);
        const uint32_t gblocks = (groups + kMtuSortWaves - 1) / kMtuSortWaves;
        hipLaunchKernelGGL(mtu_scan_kernel, dim3((uint32_t)count), dim3(1024), 0, c->stream, L);
        if (gblocks)
            hipLaunchKernelGGL(mtu_scatter_groups_kernel, dim3(gblocks), dim3(64 * kMtuSortWaves), sort_lds, c->stream, L);
    } else {
        const uint32_t sort_blocks = (tiles + kMtuSortWaves - 1) / kMtuSortWaves;
        if (fused)
            hipLaunchKernelGGL(mtu_count_kernel<true>, dim3(sort_blocks), dim3(64 * kMtuSortWaves), sort_lds, c->stream, L);
        else
            hipLaunchKernelGGL(mtu_count_kernel<false>, dim3(sort_blocks), dim3(64 * kMtuSortWaves), sort_lds, c->stream, L);
        hipLaunchKernelGGL(mtu_scan_kernel, dim3((uint32_t)count), dim3(1024), 0, c->stream, L);
        hipLaunchKernelGGL(mtu_scatter_kernel, dim3(sort_blocks), dim3(64 * kMtuSortWaves), sort_lds, c->stream, L);
    }
    if (ch == (uint32_t)kMtuChunk)
        hipLaunchKernelGGL(mtu_table_kernel<kMtuChunk>, dim3(chunk_grid), dim3(kMtuTableBlock), 0, c->stream, L);
    else
        hipLaunchKernelGGL(mtu_table_kernel<kMtuChunkSmall>, dim3(chunk_grid), dim3(kMtuTableBlock), 0, c->stream, L);
    // the chain inside the emit kernel (one lane per shard) up to 64 shards, else mtu_chain
    // (a batch's fill_out read as some batch's fill_in would change under the walks: mtu_chain reads
    // every fill_in before the shard's fill_out is written)
    bool walk = c->mtu_walk && nds <= 64;   // SR_KNOB_MTU_WALK 0: mtu_chain
    for (size_t a = 0; walk && a < count; ++a)
        for (size_t b = 0; walk && b < count; ++b) {
            const uint16_t *in = batches[b].d_fill_in, *out = batches[a].d_fill_out;
            if (in && out && in < out + nds && out < in + nds) walk = false;
        }
    if (!walk) hipLaunchKernelGGL(mtu_chain_kernel, dim3((uint32_t)count), dim3(1024), 0, c->stream, L);
    if (ch == (uint32_t)kMtuChunk) {
        if (walk) hipLaunchKernelGGL((mtu_emit_kernel<kMtuChunk, true>), dim3(chunk_grid), dim3(kMtuBlock), 0, c->stream, L);
        else hipLaunchKernelGGL((mtu_emit_kernel<kMtuChunk, false>), dim3(chunk_grid), dim3(kMtuBlock), 0, c->stream, L);
    } else {
        if (walk) hipLaunchKernelGGL((mtu_emit_kernel<kMtuChunkSmall, true>), dim3(chunk_grid), dim3(kMtuBlock), 0, c->stream, L);
        else hipLaunchKernelGGL((mtu_emit_kernel<kMtuChunkSmall, false>), dim3(chunk_grid), dim3(kMtuBlock), 0, c->stream, L);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_pack_packets_many(sr_ctx *c, const sr_pack_batch *batches, size_t count) {
    return pack_many_impl(c, batches, count, nullptr, nullptr);
}

// Route (one launch) and pack. With every shard alive (or exactly one dead: KV_DEAD1) and at most
// kHistKeys - 1 shards the route
// kernel (uniform / segment layouts) also writes each tile's key histogram and the packing skips
// mtu_count, its own pass over the records: C2 packing 0.118-0.120 -> 0.108-0.114 ms, C3 0.075-0.077
// -> 0.069-0.071 per 32 batches. Batches whose record capacity says fewer than 32 lines per 16 KiB
// tile (C4's 1024-byte lines: 16) keep the counting pass, which is cheaper there than scanning
// kHistKeys x 1024 tile counts per batch (C4 packing 0.062-0.066 against 0.071-0.076 ms;
// profiles/r05/pack_hist_ab_r5e.jsonl).
static int route_pack_impl(sr_ctx *c, const sr_batch *route, const sr_pack_batch *pack, size_t count) {
    DeviceState &ds = c->ds;
    bool want = c->hist && ds.dead <= 1 && ds.nds >= 1 && ds.nds < (uint32_t)kHistKeys;
    for (size_t i = 0; want && i < count; ++i)
        want = route[i].max_records * 512 >= route[i].nbytes;
    if (want && !ds.d_hist) {
        const size_t words = (size_t)(ds.max_tiles ? ds.max_tiles : 1) * kHistKeys;
        if (hipMalloc(&ds.d_hist, words * sizeof(uint32_t)) != hipSuccess) ds.d_hist = nullptr;
    }
    RouteParams p = ds.params();
    size_t bytes[kMaxBatches];
    for (size_t i = 0; i < count; ++i) {
        DeviceState::add_batch(p, route[i].d_bytes, route[i].nbytes, route[i].d_out, route[i].max_records,
                               route[i].d_hashes, route[i].d_n_records, route[i].d_probed_dead);
        bytes[i] = route[i].nbytes;
    }
    p.hist = want ? ds.d_hist : nullptr;
    ds.last_hist = false;
    ds.fuse_defer = c->fuse_defer && !want;
    ds.pack_ors_marks = want;
    ds.last_marks_pending = false;
    int rc = launch_variant(ds, p, c->stream);
    ds.fuse_defer = false;
    ds.pack_ors_marks = false;
    if (rc) return rc;
    const bool fused = ds.last_fused;
    ds.last_fused = false;
    const bool marks = ds.last_marks_pending;   // the tiles' probed-dead slots, for mtu_scan to OR
    ds.last_marks_pending = false;
    if (marks && !ds.last_hist) return -EIO;   // (never: such launches ran the KV_HIST1 kernel)
    return pack_many_impl(c, pack, count, ds.last_hist ? ds.d_hist : nullptr, bytes, fused,
                          marks ? ds.d_tile_pd : nullptr);
}

int sr_route_pack_many(sr_ctx *c, const sr_batch *route, const sr_pack_batch *pack, size_t count) {
    if (!c || !route || !pack || count == 0 || count > (size_t)kMaxBatches) return -EINVAL;
    for (size_t i = 0; i < count; ++i) {
        const sr_batch &b = route[i];
        if (!b.d_n_records || (b.nbytes && !b.d_bytes) || b.nbytes > c->ds.max_batch) return -EINVAL;
        if (b.max_records && !b.d_out) return -EINVAL;
        // the packing reads what the route writes
        if (pack[i].d_recs != b.d_out || pack[i].d_n_records != b.d_n_records || pack[i].max_records != b.max_records ||
            pack[i].d_probed_dead != b.d_probed_dead)
            return -EINVAL;
    }
    (void)hipSetDevice(c->device);
    return route_pack_impl(c, route, pack, count);
}

int sr_pack_packets(sr_ctx *c, const sr_record *d_recs, const uint64_t *d_n_records, size_t max_records,
                    const uint16_t *d_fill_in, const uint64_t *d_probed_dead, sr_record *d_sorted,
                    sr_packet *d_packets, size_t max_packets, uint64_t *d_counts, uint16_t *d_fill_out) {
    const sr_pack_batch b{d_recs, d_n_records, max_records, d_fill_in, d_probed_dead,
                          d_sorted, d_packets, max_packets, d_counts, d_fill_out};
    return sr_pack_packets_many(c, &b, 1);
}

// The packets' bytes of packed batches (payload_kernel.hpp): the offsets' scan, the gather (one wave
// per descriptor the batch can have) and, where a batch keeps its pending bytes on the device, the
// pass-through of the downstreams without a descriptor. No scratch: nothing is allocated here.
static int payloads_impl(sr_ctx *c, const sr_payload_batch *batches, size_t count) {
    static_assert(SR_PENDING_STRIDE == kPendStride && SR_PENDING_STRIDE % 16 == 0 &&
                      SR_PENDING_STRIDE >= SR_DOWNSTREAM_BUF_SIZE,
                  "pending slot");
    if (!c || !batches || count == 0 || count > (size_t)kPayMaxBatches) return -EINVAL;
    const uint32_t nds = c->ds.nds;
    if (nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    PayLaunch L;
    memset(&L, 0, sizeof(L));
    uint32_t tiles = 0;
    bool pend = false;
    for (size_t j = 0; j < count; ++j) {
        const sr_payload_batch &b = batches[j];
        if (!b.d_counts || !b.d_offsets || !b.d_total || (nds && !b.d_fill_out)) return -EINVAL;
        if ((b.nbytes && !b.d_bytes) || b.nbytes > 0xFFFFFFF0ull || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if ((b.max_records && !b.d_sorted) || (b.max_packets && !b.d_packets)) return -EINVAL;
        if (b.payload_cap && !b.d_payload) return -EINVAL;
        if (b.d_pend_out && (!b.d_pend_in || b.d_pend_out == b.d_pend_in)) return -EINVAL;
        PayBatchArg &a = L.b[j];
        a.bytes = b.d_bytes;
        a.sorted = b.d_sorted;
        a.packets = b.d_packets;
        a.counts = b.d_counts;
        a.fill_out = b.d_fill_out;
        a.pend_in = b.d_pend_in;
        a.pend_out = b.d_pend_out;
        a.payload = b.d_payload;
        a.offsets = b.d_offsets;
        a.total = b.d_total;
        a.payload_cap = b.payload_cap;
        a.nbytes = (uint32_t)b.nbytes;
        a.max_records = (uint32_t)b.max_records;
        // never more descriptors than SR_MAX_PACKETS of the batch: the gather's grid
        const uint64_t most = SR_MAX_PACKETS((uint64_t)b.nbytes, nds);
        const uint64_t room = b.max_packets < most ? b.max_packets : most;
        a.max_packets = (uint32_t)(b.max_packets > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : b.max_packets);
        a.tile0 = tiles;
        const uint64_t per = (uint64_t)kPayWaves * kPayPerWave;   // packets per workgroup
        const uint64_t t = (room + per - 1) / per;
        if (tiles + t > 0x7FFFFFFFull) return -EINVAL;
        tiles += (uint32_t)t;
        pend = pend || (b.d_pend_out && nds);
    }
    (void)hipSetDevice(c->device);
    L.nb = (uint32_t)count;
    L.nds = nds;
    L.tiles = tiles;
    hipLaunchKernelGGL(payload_offsets_kernel, dim3((uint32_t)count), dim3(1024), 0, c->stream, L);
    if (tiles) hipLaunchKernelGGL(payload_copy_kernel, dim3(tiles), dim3(kPayBlock), 0, c->stream, L);
    if (pend)
        hipLaunchKernelGGL(payload_pending_kernel, dim3((nds + kPayWaves - 1) / kPayWaves, (uint32_t)count),
                           dim3(kPayBlock), 0, c->stream, L);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_pack_payloads_many(sr_ctx *c, const sr_payload_batch *batches, size_t count) {
    return payloads_impl(c, batches, count);
}

int sr_pack_payloads(sr_ctx *c, const sr_payload_batch *batch) { return payloads_impl(c, batch, 1); }

// The three framing launches on the context's stream (frame_kernel.hpp). The scratch is allocated once, at
// its full size, by the first call: later calls allocate nothing and can be captured in a graph.
static int frame_impl(sr_ctx *c, const sr_slot_batch *b) {
    static_assert(SR_MAX_SLOTS == kFrameSpan * kFrameMaxGroups, "one wave scans the workgroup sums");
    static_assert(SR_MAX_SLOT_STRIDE == kFrameMaxStride, "offsets inside a gather run");
    static_assert((uint64_t)SR_MAX_SLOTS * (SR_MAX_DATAGRAM + 1u) <= 0xFFFFFFFFull, "framed offsets fit 32 bits");
    if (!c || !b || !b->d_total) return -EINVAL;
    if (b->stride < SR_DATA_BUF_SIZE || b->stride > kFrameMaxStride || b->count > SR_MAX_SLOTS) return -EINVAL;
    if (b->count && (!b->d_slots || !b->d_lens)) return -EINVAL;
    if (b->cap && !b->d_bytes) return -EINVAL;
    (void)hipSetDevice(c->device);
    if (b->count == 0) return hipMemsetAsync(b->d_total, 0, sizeof(uint64_t), c->stream) == hipSuccess ? 0 : -EIO;
    if (!c->d_frame && hipMalloc(&c->d_frame, (kFrameMaxGroups + (size_t)SR_MAX_SLOTS) * sizeof(uint32_t)) != hipSuccess) {
        c->d_frame = nullptr;
        return -ENOMEM;
    }
    FrameArgs a;
    a.slots = b->d_slots;
    a.stride = b->stride;
    a.lens = b->d_lens;
    a.bytes = b->d_bytes;
    a.cap = b->cap;
    a.ends = b->d_ends;
    a.total = b->d_total;
    a.sums = c->d_frame;
    a.loc = c->d_frame + kFrameMaxGroups;
    a.count = (uint32_t)b->count;
    const uint32_t groups = (a.count + kFrameSpan - 1u) / kFrameSpan;
    const uint32_t per = (uint32_t)(kFrameWaves * kFrameRun);   // datagrams per gather workgroup
    hipLaunchKernelGGL(frame_lens_kernel, dim3(groups), dim3(kFrameSpan), 0, c->stream, a);
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(frame_gather_kernel, dim3((a.count + per - 1u) / per), dim3(kFrameBlock), 0, c->stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_frame_slots(sr_ctx *c, const sr_slot_batch *b) { return frame_impl(c, b); }

// The three formatting launches on the context's stream (log_kernel.hpp). The scratch is allocated once, for a
// batch of max_batch_bytes one-byte lines, by the first call: later calls allocate nothing and can be captured
// in a graph.
static int log_impl(sr_ctx *c, const sr_log_batch *b) {
    static_assert(SR_LOG_MAX_PREFIX == kLogMaxPrefix, "prefix room in LDS");
    if (!c || !b || !b->d_total || !b->d_n_msgs || !b->d_n_records) return -EINVAL;
    if (b->min_level < 0 || b->min_level > 3) return -EINVAL;
    if (b->nbytes > c->ds.max_batch || b->nbytes > kLogMaxBatch || (b->nbytes && !b->d_bytes)) return -EINVAL;
    const size_t rec_room = b->max_records < b->nbytes ? b->max_records : b->nbytes;   // a line has a byte
    if (rec_room && (!b->d_recs || (b->min_level == 0 && !b->d_hashes))) return -EINVAL;
    if (b->d_ends && b->n_datagrams > 0xFFFFFFF0ull) return -EINVAL;
    if (b->prefix_len[0] > kLogMaxPrefix || b->prefix_len[1] > kLogMaxPrefix) return -EINVAL;
    if ((b->prefix_len[0] || b->prefix_len[1]) && !b->d_prefix) return -EINVAL;
    if (b->max_msg && (b->max_msg <= b->prefix_len[0] || b->max_msg <= b->prefix_len[1])) return -EINVAL;
    if (b->text_cap && !b->d_text) return -EINVAL;
    (void)hipSetDevice(c->device);
    const size_t full = c->ds.max_batch < kLogMaxBatch ? c->ds.max_batch : kLogMaxBatch;
    if (!c->d_log && hipMalloc(&c->d_log, 2 * ((full + kLogRecs - 1) / kLogRecs + 1) * sizeof(uint64_t)) != hipSuccess) {
        c->d_log = nullptr;
        return -ENOMEM;
    }
    LogArgs a;
    a.bytes = b->d_bytes;
    a.recs = b->d_recs;
    a.n_records = b->d_n_records;
    a.hashes = b->d_hashes;
    a.ends = b->d_ends;
    a.prefix = b->d_prefix;
    a.text = b->d_text;
    a.offsets = b->d_offsets;
    a.levels = b->d_levels;
    a.total = b->d_total;
    a.n_msgs = b->d_n_msgs;
    a.gsum = c->d_log;
    a.text_cap = b->text_cap;
    a.max_msgs = b->max_msgs;
    a.nbytes = (uint32_t)b->nbytes;
    a.rec_room = (uint32_t)rec_room;
    a.n_ends = b->d_ends ? (uint32_t)b->n_datagrams : 0u;
    a.nds = c->ds.nds;
    a.plen[0] = b->prefix_len[0];
    a.plen[1] = b->prefix_len[1];
    a.max_msg = b->max_msg;
    a.warn_only = b->min_level > 0 ? 1u : 0u;
    const uint32_t groups = (a.rec_room + (uint32_t)kLogRecs - 1u) / (uint32_t)kLogRecs;
    if (groups) hipLaunchKernelGGL(log_lens_kernel, dim3(groups), dim3(kLogRecs), 0, c->stream, a);
    hipLaunchKernelGGL(log_scan_kernel, dim3(1), dim3(1024), 0, c->stream, a);
    if (groups) hipLaunchKernelGGL(log_write_kernel, dim3(groups), dim3(kLogRecs), 0, c->stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_format_log(sr_ctx *c, const sr_log_batch *b) { return log_impl(c, b); }

// ---- name statistics (stats_kernel.hpp, stats_host.hpp) ---------------------------------------------
// One device allocation holds the whole state, so a reset is one memset and a read one copy:
// counters | per-shard lines, bytes | cells | hot keys A, B | hot names | registers (u32 each)
static int stats_open_impl(sr_ctx *c, const sr_stats_config *cfg) {
    if (!c) return -EINVAL;
    StatsState &st = c->stats;
    if (st.open) return -EBUSY;
    sr_stats_config r;
    if (stats_resolve(cfg, c->ds.nds, &r) != 0) return -EINVAL;
    const size_t nds = c->ds.nds, cells = (size_t)r.cms_rows * r.cms_width;
    st.o_shard = kStatsCtrs * sizeof(uint64_t);
    st.o_cells = st.o_shard + 2 * nds * sizeof(uint64_t);
    st.o_ka = st.o_cells + cells * sizeof(uint64_t);
    st.o_kb = st.o_ka + (size_t)r.hot_slots * sizeof(uint64_t);
    st.o_names = st.o_kb + (size_t)r.hot_slots * sizeof(uint64_t);
    st.o_regs = st.o_names + (size_t)r.hot_slots * sizeof(StatsHotName);
    st.bytes = st.o_regs + (nds << r.hll_p) * sizeof(uint32_t);
    (void)hipSetDevice(c->device);
    if (hipMalloc(&st.d_base, st.bytes) != hipSuccess) {
        st.d_base = nullptr;
        (void)hipGetLastError();
        return -ENOMEM;
    }
    if (hipMemsetAsync(st.d_base, 0, st.bytes, c->stream) != hipSuccess) {
        free_ptr(st.d_base);
        st.d_base = nullptr;
        return -EIO;
    }
    // the sketch in LDS next to the per-shard sums can pass the 64 KiB default (set here, not in a capture)
    ensure_dyn_lds((const void *)stats_count_kernel<true>, SR_STATS_MAX_CELLS * 4);
    ensure_dyn_lds((const void *)stats_count_kernel<false>, SR_STATS_MAX_CELLS * 4);
    st.cfg = r;
    st.open = 1;
    return 0;
}

static int stats_update_impl(sr_ctx *c, const sr_stats_batch *batches, size_t count) {
    static_assert(kStatsMaxBatches == (int)SR_MAX_BATCHES_PER_LAUNCH, "launch batch limit");
    if (!c || !c->stats.open || !batches || count == 0 || count > (size_t)kStatsMaxBatches) return -EINVAL;
    const StatsState &st = c->stats;
    StatsArgs a;
    memset(&a, 0, sizeof(a));
    uint64_t tiles = 0;   // the grid's bound only (the kernels number the tiles by the device's counts)
    for (size_t j = 0; j < count; ++j) {
        const sr_stats_batch &b = batches[j];
        if (!b.d_n_records || !b.d_hashes || (b.max_records && !b.d_recs) || (b.nbytes && !b.d_bytes)) return -EINVAL;
        if (b.nbytes > 0xFFFFFFF0ull || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        StatsBatchArg &o = a.b[j];
        o.bytes = b.d_bytes;
        o.recs = b.d_recs;
        o.n_records = b.d_n_records;
        o.hashes = b.d_hashes;
        o.nbytes = (uint32_t)b.nbytes;
        o.max_records = (uint32_t)b.max_records;
        // the host-memory path gives max_records = nbytes (a line has at least a byte): the grid goes by the
        // lines a batch of this size plausibly holds, the kernels by the device's counts
        const uint64_t likely = (uint64_t)b.nbytes / kStatsGridLineBytes + 1u;
        const uint64_t room = b.max_records < likely ? b.max_records : likely;
        tiles += (room + kStatsTile - 1) / kStatsTile;
    }
    if (!tiles) return 0;
    uint8_t *const base = st.d_base;
    a.ctr = (unsigned long long *)base;
    a.shard = (unsigned long long *)(base + st.o_shard);
    a.cells = (unsigned long long *)(base + st.o_cells);
    a.key_a = (unsigned long long *)(base + st.o_ka);
    a.key_b = (unsigned long long *)(base + st.o_kb);
    a.names = (StatsHotName *)(base + st.o_names);
    a.regs = (uint32_t *)(base + st.o_regs);
    a.nb = (uint32_t)count;
    a.nds = c->ds.nds;
    a.p = st.cfg.hll_p;
    a.rows = st.cfg.cms_rows;
    a.width = st.cfg.cms_width;
    a.slots = st.cfg.hot_slots;
    a.hot_div = st.cfg.hot_div;
    a.hot_min = st.cfg.hot_min_lines;
    (void)hipSetDevice(c->device);
    // the grid by the records: a few thousand lines get a few workgroups, never more than kStatsGroups
    const uint64_t want = (tiles + kStatsTilesPerGroup - 1) / kStatsTilesPerGroup;
    const dim3 grid((uint32_t)(want < (uint64_t)kStatsGroups ? want : (uint64_t)kStatsGroups));
    const size_t lds = (size_t)a.rows * a.width * sizeof(uint32_t);
    if (a.nds <= (uint32_t)kStatsLdsShards)
        hipLaunchKernelGGL(stats_count_kernel<true>, grid, dim3(kStatsBlock), lds, c->stream, a);
    else
        hipLaunchKernelGGL(stats_count_kernel<false>, grid, dim3(kStatsBlock), lds, c->stream, a);
    hipLaunchKernelGGL(stats_hot_kernel, grid, dim3(kStatsBlock), 0, c->stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_stats_open(sr_ctx *c, const sr_stats_config *cfg) { return stats_open_impl(c, cfg); }

int sr_stats_update(sr_ctx *c, const sr_stats_batch *batches, size_t count) {
    return stats_update_impl(c, batches, count);
}

int sr_stats_reset(sr_ctx *c) {
    if (!c || !c->stats.open) return -EINVAL;
    (void)hipSetDevice(c->device);
    return hipMemsetAsync(c->stats.d_base, 0, c->stats.bytes, c->stream) == hipSuccess ? 0 : -EIO;
}

int sr_stats_close(sr_ctx *c) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!c->stats.open) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_ptr(c->stats.d_base);
    memset(&c->stats, 0, sizeof(c->stats));
    c->name_stats = 0;
    return 0;
}

int sr_stats_read(sr_ctx *c, sr_stats_snapshot **out) {
    if (out) *out = nullptr;
    if (!c || !out || !c->stats.open) return -EINVAL;
    const StatsState &st = c->stats;
    const uint32_t nds = c->ds.nds;
    (void)hipSetDevice(c->device);
    uint8_t *h = (uint8_t *)malloc(st.bytes);
    sr_stats_snapshot *s = stats_snap_alloc(st.cfg, nds);
    if (!h || !s) {
        free(h);
        free(s);
        return -ENOMEM;
    }
    if (hipMemcpyAsync(h, st.d_base, st.bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        free(h);
        free(s);
        return -EIO;
    }
    const uint64_t *ctr = (const uint64_t *)h;
    for (int v = 0; v < 4; ++v) {
        s->lines[v] = ctr[kStatsCtrLines + v];
        s->bytes[v] = ctr[kStatsCtrBytes + v];
    }
    s->ignored = ctr[kStatsCtrIgnored];
    s->hot_overflow = ctr[kStatsCtrOverflow] ? 1u : 0u;
    memcpy(s->shard_lines, h + st.o_shard, (size_t)nds * sizeof(uint64_t));
    memcpy(s->shard_bytes, h + st.o_shard + (size_t)nds * sizeof(uint64_t), (size_t)nds * sizeof(uint64_t));
    memcpy(s->cells, h + st.o_cells, (size_t)st.cfg.cms_rows * st.cfg.cms_width * sizeof(uint64_t));
    const uint32_t *regs = (const uint32_t *)(h + st.o_regs);
    for (size_t i = 0, n = (size_t)nds << st.cfg.hll_p; i < n; ++i) s->regs[i] = (uint8_t)regs[i];
    const uint64_t *ka = (const uint64_t *)(h + st.o_ka), *kb = (const uint64_t *)(h + st.o_kb);
    const StatsHotName *names = (const StatsHotName *)(h + st.o_names);
    for (uint32_t k = 0; k < st.cfg.hot_slots; ++k) {
        if (!kb[k]) continue;   // B is set last: a slot without it holds nothing
        sr_stats_hot &e = s->hot[s->n_hot++];
        e.hash = (ka[k] >> 32) << 32 | kb[k] >> 32;
        e.name_len = names[k].name_len;
        memcpy(e.name, names[k].name, SR_STATS_NAME_MAX);
    }
    stats_sort_hot(s);
    free(h);
    *out = s;
    return 0;
}

void sr_stats_free(sr_stats_snapshot *snap) { free(snap); }

uint64_t sr_name_hash(const uint8_t *bytes, size_t len) { return (bytes || !len) ? stats_name_hash(bytes, len) : 0; }

uint64_t sr_stats_estimate(const sr_stats_snapshot *snap, uint64_t hash) {
    return stats_snap_ok(snap) ? stats_estimate(snap, hash) : 0;
}

double sr_stats_cardinality(const sr_stats_snapshot *snap, uint32_t shard) {
    if (!stats_snap_ok(snap) || (shard != SR_STATS_ALL && shard >= snap->n_downstreams)) return -1.0;
    return stats_cardinality(snap, shard);
}

int sr_stats_merge(sr_stats_snapshot *into, const sr_stats_snapshot *from) { return stats_merge(into, from); }

int sr_set_name_stats(sr_ctx *c, const sr_stats_config *cfg) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!cfg) {
        c->name_stats = 0;
        return 0;
    }
    if (!c->stats.open) {
        const int rc = stats_open_impl(c, cfg);
        if (rc) return rc;
    }
    c->name_stats = 1;
    return 0;
}

static int grow(void **ptr, size_t *cap, size_t need, size_t elem) {
    if (need <= *cap) return 0;
    free_ptr(*ptr);
    *ptr = nullptr;
    *cap = 0;
    if (hipMalloc(ptr, (need ? need : 1) * elem) != hipSuccess) return -ENOMEM;
    *cap = need;
    return 0;
}

// ---- plain counters coalesced (coalesce_kernel.hpp, coalesce_host.hpp) ------------------------------------
int sr_coalesce_open(sr_ctx *c, const sr_coalesce_config *cfg) {
    if (!c) return -EINVAL;
    CoalesceState &st = c->coalesce;
    if (st.open) return -EBUSY;
    uint32_t slots = 0;
    if (coalesce_resolve(cfg, &slots) != 0) return -EINVAL;
    (void)hipSetDevice(c->device);
    if (hipMalloc(&st.d_table, (size_t)kCoalesceMaxBatches * slots * sizeof(CoalesceSlot)) != hipSuccess) {
        st.d_table = nullptr;
        (void)hipGetLastError();
        return -ENOMEM;
    }
    st.slots = slots;
    st.open = 1;
    return 0;
}

int sr_coalesce_close(sr_ctx *c) {
    if (!c) return -EINVAL;
    CoalesceState &st = c->coalesce;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!st.open) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_ptr(st.d_table);
    free_ptr(st.d_scratch);
    free_ptr(st.d_tiles);
    memset(&st, 0, sizeof(st));
    c->coalesce_on = 0;
    return 0;
}

// The input buffer of the host-memory path for the switches that allocate it again: the batch, then
// SR_SAMPLE_APPEND_CAPACITY(max_batch) of room for the rewritten lines (sr_set_sample), then max_batch of room for the
// merged text (sr_set_coalesce). Grown, never shrunk; every slot is idle.
static int input_reserve(sr_ctx *c, bool sample, bool coalesce) {
    const uint64_t full = c->ds.max_batch;
    const uint64_t arena = sample ? (uint64_t)SR_SAMPLE_APPEND_CAPACITY(full) : 0u;
    const uint64_t total = full + arena + (coalesce ? full : 0u);
    if (total > 0xFFFFFFF0ull || (coalesce && full + arena > SR_COALESCE_MAX_BYTES)) return -EINVAL;
    if (total <= (c->d_in_cap ? c->d_in_cap : full)) return 0;
    (void)hipStreamSynchronize(c->stream);
    uint8_t *in = nullptr;
    if (hipMalloc(&in, total) != hipSuccess) return -ENOMEM;
    free_ptr(c->d_in);
    c->d_in = in;
    c->d_in_cap = total;
    return 0;
}

int sr_set_coalesce(sr_ctx *c, const sr_coalesce_config *cfg) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!cfg) {
        c->coalesce_on = 0;
        return 0;
    }
    const size_t full = c->ds.max_batch;
    if (full > SR_COALESCE_MAX_BYTES || 2 * (uint64_t)full > 0xFFFFFFF0ull) return -EINVAL;
    if (!c->coalesce.open) {
        const int rc = sr_coalesce_open(c, cfg);
        if (rc) return rc;
    }
    (void)hipSetDevice(c->device);
    if (!c->d_ccounts) {   // the first time: the input buffer again, with room for the merged text behind a batch
        const int rc = input_reserve(c, c->d_scounts != nullptr, true);
        if (rc) return rc;
        if (hipMalloc(&c->d_ccounts, 4 * sizeof(uint64_t)) != hipSuccess) {
            c->d_ccounts = nullptr;
            return -ENOMEM;
        }
    }
    c->coalesce_on = 1;
    return 0;
}

int sr_route_pack_coalesced(sr_ctx *c, int slot, const uint8_t **text, size_t *len, uint64_t counts[4]) {
    if (!c || !text || !len || !counts || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.coalesced || !sl.chost) return -EBUSY;
    const uint64_t *hc = (const uint64_t *)(sl.chost + ((sl.ctext_cap + 255) & ~(size_t)255));
    for (int q = 0; q < 4; ++q) counts[q] = hc[q];
    *text = sl.chost;
    *len = (size_t)(hc[3] < sl.ctext_cap ? hc[3] : sl.ctext_cap);
    return hc[3] > sl.ctext_cap ? -ENOSPC : 0;
}

int sr_coalesce(sr_ctx *c, const sr_coalesce_batch *batches, size_t count) {
    static_assert(kCoalesceMaxBatches == (int)SR_MAX_BATCHES_PER_LAUNCH, "launch batch limit");
    if (!c || !c->coalesce.open || !batches || count == 0 || count > (size_t)kCoalesceMaxBatches) return -EINVAL;
    CoalesceState &st = c->coalesce;
    size_t records = 0, tiles = 0;   // the scratch's sizes, by max_records
    uint64_t grid_tiles = 0;         // the grid's bound only (the kernels number the tiles by the device's counts)
    for (size_t j = 0; j < count; ++j) {
        const sr_coalesce_batch &b = batches[j];
        if (!b.d_n_records || !b.d_counts || !b.d_hashes || (b.nbytes && !b.d_bytes)) return -EINVAL;
        if (b.max_records && (!b.d_recs || !b.d_out || b.d_out == b.d_recs)) return -EINVAL;
        if ((const void *)b.d_counts == (const void *)b.d_n_records) return -EINVAL;   // read after the counts are written
        if (b.nbytes > SR_COALESCE_MAX_BYTES || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if (b.append_cap > 0xFFFFFFF0ull || (uint64_t)b.nbytes + b.append_cap > 0xFFFFFFF0ull) return -EINVAL;
        records += b.max_records;
        tiles += (b.max_records + kCoalesceTile - 1) / kCoalesceTile;
        const uint64_t likely = (uint64_t)b.nbytes / kCoalesceGridLineBytes + 1u;
        const uint64_t room = b.max_records < likely ? b.max_records : likely;
        grid_tiles += (room + kCoalesceTile - 1) / kCoalesceTile;
    }
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = grow((void **)&st.d_scratch, &st.scratch_cap, records, sizeof(uint2)))) return rc;
    if ((rc = grow((void **)&st.d_tiles, &st.tiles_cap, tiles, sizeof(uint4)))) return rc;
    CoalesceArgs a;
    memset(&a, 0, sizeof(a));
    size_t at = 0;
    for (size_t j = 0; j < count; ++j) {
        const sr_coalesce_batch &b = batches[j];
        CoalesceBatchArg &o = a.b[j];
        o.bytes = b.d_bytes;
        o.recs = b.d_recs;
        o.n_records = b.d_n_records;
        o.hashes = b.d_hashes;
        o.out = b.d_out;
        o.counts = b.d_counts;
        o.scratch = st.d_scratch + at;
        o.append_cap = b.append_cap;
        o.nbytes = (uint32_t)b.nbytes;
        o.max_records = (uint32_t)b.max_records;
        at += b.max_records;
    }
    a.table = st.d_table;
    a.tiles = st.d_tiles;
    a.nb = (uint32_t)count;
    a.nds = c->ds.nds;
    a.slots = st.slots;
    if (grid_tiles) {
        const uint64_t entries = (uint64_t)count * st.slots;   // at most 2^27
        const uint64_t cg = (entries + kCoalesceBlock - 1) / kCoalesceBlock;
        const dim3 clear_grid((uint32_t)(cg < (uint64_t)kCoalesceGroups ? cg : (uint64_t)kCoalesceGroups));
        const dim3 grid((uint32_t)(grid_tiles < (uint64_t)kCoalesceGroups ? grid_tiles : (uint64_t)kCoalesceGroups));
        hipLaunchKernelGGL(coalesce_clear_kernel, clear_grid, dim3(kCoalesceBlock), 0, c->stream, st.d_table, (uint32_t)entries);
        hipLaunchKernelGGL(coalesce_claim_kernel, grid, dim3(kCoalesceBlock), 0, c->stream, a);
        hipLaunchKernelGGL(coalesce_join_kernel, grid, dim3(kCoalesceBlock), 0, c->stream, a);
        hipLaunchKernelGGL(coalesce_sum_kernel, grid, dim3(kCoalesceBlock), 0, c->stream, a);
        hipLaunchKernelGGL(coalesce_scan_kernel, dim3((uint32_t)count), dim3(kCoalesceScanBlock), 0, c->stream, a);
        hipLaunchKernelGGL(coalesce_emit_kernel, grid, dim3(kCoalesceBlock), 0, c->stream, a);
    } else {   // no batch has room for a record: the counts alone
        hipLaunchKernelGGL(coalesce_scan_kernel, dim3((uint32_t)count), dim3(kCoalesceScanBlock), 0, c->stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_coalesce_parse(const uint8_t *line, size_t len, uint32_t *name_len, int64_t *value) {
    return coalesce_parse_line(line, len, name_len, value);
}

size_t sr_coalesce_format(uint8_t *dst, const uint8_t *name, uint32_t name_len, int64_t sum) {
    if (!dst || (name_len && !name)) return 0;
    return coalesce_format_line(dst, name, name_len, sum);
}

// ---- name rules (rules_kernel.hpp, rules_host.hpp) ----------------------------------------------------------
int sr_rules_open(sr_ctx *c, const sr_rules_config *cfg) {
    if (!c) return -EINVAL;
    RulesState &st = c->rules;
    if (st.open) return -EBUSY;
    (void)hipSetDevice(c->device);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // it allocates and waits: not inside a capture
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return -EINVAL;
    RulesTable *t = (RulesTable *)malloc(sizeof(RulesTable));
    if (!t) return -ENOMEM;
    if (rules_compile(cfg, t) != 0) {
        free(t);
        return -EINVAL;
    }
    (void)hipSetDevice(c->device);
    int rc = 0;
    if (hipMalloc(&st.d_table, sizeof(RulesTable)) != hipSuccess) {
        st.d_table = nullptr;
        rc = -ENOMEM;
    } else if (hipMalloc(&st.d_hits, kRulesHitCells * sizeof(unsigned long long)) != hipSuccess) {
        st.d_hits = nullptr;
        rc = -ENOMEM;
    } else if (hipMemcpyAsync(st.d_table, t, sizeof(RulesTable), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
               hipMemsetAsync(st.d_hits, 0, kRulesHitCells * sizeof(unsigned long long), c->stream) != hipSuccess ||
               hipStreamSynchronize(c->stream) != hipSuccess) {   // t is pageable: the copy is done before it is freed
        rc = -EIO;
    }
    const uint32_t n_rules = t->n_rules;
    free(t);
    if (rc) {
        (void)hipGetLastError();
        free_ptr(st.d_table);
        free_ptr(st.d_hits);
        memset(&st, 0, sizeof(st));
        return rc;
    }
    st.n_rules = n_rules;
    st.open = 1;
    return 0;
}

int sr_rules_close(sr_ctx *c) {
    if (!c) return -EINVAL;
    RulesState &st = c->rules;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!st.open) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_ptr(st.d_table);
    free_ptr(st.d_hits);
    free_ptr(st.d_match);
    free_ptr(st.d_tiles);
    memset(&st, 0, sizeof(st));
    c->rules_on = 0;
    return 0;
}

int sr_rules(sr_ctx *c, const sr_rules_batch *batches, size_t count) {
    static_assert(kRulesMaxBatches == (int)SR_MAX_BATCHES_PER_LAUNCH, "launch batch limit");
    if (!c || !c->rules.open || !batches || count == 0 || count > (size_t)kRulesMaxBatches) return -EINVAL;
    RulesState &st = c->rules;
    size_t records = 0, tiles = 0;   // the scratch's sizes, by max_records
    uint64_t grid_tiles = 0;         // the grid's bound only (the kernels number the tiles by the device's counts)
    for (size_t j = 0; j < count; ++j) {
        const sr_rules_batch &b = batches[j];
        if (!b.d_n_records || !b.d_counts || (b.nbytes && !b.d_bytes)) return -EINVAL;
        if (b.max_records && (!b.d_recs || !b.d_out || b.d_out == b.d_recs)) return -EINVAL;
        if (b.d_hashes && b.d_hashes_out == b.d_hashes) return -EINVAL;
        if ((const void *)b.d_counts == (const void *)b.d_n_records) return -EINVAL;   // read after the counts are written
        if (b.nbytes > 0xFFFFFFF0ull || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if (!b.d_match) records += b.max_records;
        tiles += (b.max_records + kRulesTile - 1) / kRulesTile;
        const uint64_t likely = (uint64_t)b.nbytes / kRulesGridLineBytes + 1u;
        const uint64_t room = b.max_records < likely ? b.max_records : likely;
        grid_tiles += (room + kRulesTile - 1) / kRulesTile;
    }
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = grow((void **)&st.d_match, &st.match_cap, records, sizeof(uint16_t)))) return rc;
    if ((rc = grow((void **)&st.d_tiles, &st.tiles_cap, tiles, sizeof(uint4)))) return rc;
    RulesArgs a;
    memset(&a, 0, sizeof(a));
    size_t at = 0;
    for (size_t j = 0; j < count; ++j) {
        const sr_rules_batch &b = batches[j];
        RulesBatchArg &o = a.b[j];
        const bool hashes = b.d_hashes && b.d_hashes_out;
        o.bytes = b.d_bytes;
        o.recs = b.d_recs;
        o.n_records = b.d_n_records;
        o.hashes = hashes ? b.d_hashes : nullptr;
        o.out = b.d_out;
        o.hashes_out = hashes ? b.d_hashes_out : nullptr;
        o.match = b.d_match ? b.d_match : st.d_match + at;
        o.counts = b.d_counts;
        o.nbytes = (uint32_t)b.nbytes;
        o.max_records = (uint32_t)b.max_records;
        if (!b.d_match) at += b.max_records;
    }
    a.table = st.d_table;
    a.hits = st.d_hits;
    a.tiles = st.d_tiles;
    a.nb = (uint32_t)count;
    a.nds = c->ds.nds;
    if (grid_tiles) {
        const dim3 grid((uint32_t)(grid_tiles < (uint64_t)kRulesGroups ? grid_tiles : (uint64_t)kRulesGroups));
        hipLaunchKernelGGL(rules_match_kernel, grid, dim3(kRulesBlock), 0, c->stream, a);
        hipLaunchKernelGGL(rules_scan_kernel, dim3((uint32_t)count), dim3(kRulesScanBlock), 0, c->stream, a);
        hipLaunchKernelGGL(rules_emit_kernel, grid, dim3(kRulesBlock), 0, c->stream, a);
    } else {   // no batch has room for a record: the counts alone
        hipLaunchKernelGGL(rules_scan_kernel, dim3((uint32_t)count), dim3(kRulesScanBlock), 0, c->stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_rules_read(sr_ctx *c, sr_rule_hits *hits, size_t n) {
    static_assert(sizeof(sr_rule_hits) == 2 * sizeof(unsigned long long), "a hit is two cells");
    if (!c || !c->rules.open || (n && !hits)) return -EINVAL;
    const size_t m = n < (size_t)c->rules.n_rules + 1 ? n : (size_t)c->rules.n_rules + 1;
    (void)hipSetDevice(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -EIO;
    if (m && hipMemcpy(hits, c->rules.d_hits, m * sizeof(sr_rule_hits), hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
    return (int)m;
}

int sr_rules_reset(sr_ctx *c) {
    if (!c || !c->rules.open) return -EINVAL;
    (void)hipSetDevice(c->device);
    return hipMemsetAsync(c->rules.d_hits, 0, kRulesHitCells * sizeof(unsigned long long), c->stream) == hipSuccess ? 0 : -EIO;
}

int sr_rules_check(const sr_rules_config *cfg) {
    RulesTable *t = (RulesTable *)malloc(sizeof(RulesTable));
    if (!t) return -ENOMEM;
    const int rc = rules_compile(cfg, t);
    free(t);
    return rc;
}

int sr_rules_match(const sr_rules_config *cfg, const uint8_t *line, size_t len) {
    if (len && !line) return -EINVAL;
    RulesTable *t = (RulesTable *)malloc(sizeof(RulesTable));
    if (!t) return -ENOMEM;
    int rc = rules_compile(cfg, t);
    if (rc == 0) rc = (int)rules_match(*t, line, len);
    free(t);
    return rc;
}

int sr_rules_parse_text(const char *text, size_t len, sr_rules_config **out, size_t *err_line) {
    return rules_parse_text(text, len, out, err_line);
}

void sr_rules_free(sr_rules_config *cfg) { free(cfg); }

int sr_set_name_rules(sr_ctx *c, const sr_rules_config *cfg) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!cfg) {
        c->rules_on = 0;
        return 0;
    }
    int rc = sr_rules_check(cfg);   // a bad set leaves the stage as it was
    if (rc) return rc;
    if (c->rules.open && (rc = sr_rules_close(c))) return rc;
    if ((rc = sr_rules_open(c, cfg))) return rc;
    (void)hipSetDevice(c->device);
    if (!c->d_rcounts && hipMalloc(&c->d_rcounts, 4 * sizeof(uint64_t)) != hipSuccess) {
        c->d_rcounts = nullptr;
        return -ENOMEM;
    }
    c->rules_on = 1;
    return 0;
}

int sr_route_pack_rules(sr_ctx *c, int slot, uint64_t counts[4]) {
    if (!c || !counts || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.ruled || !sl.rhost) return -EBUSY;
    for (int q = 0; q < 4; ++q) counts[q] = sl.rhost[q];
    return 0;
}

// ---- line grammar (validate_kernel.hpp, validate_host.hpp) --------------------------------------------------
int sr_validate_open(sr_ctx *c, const sr_validate_config *cfg) {
    if (!c) return -EINVAL;
    ValidateStage &st = c->validate;
    if (st.open) return -EBUSY;
    (void)hipSetDevice(c->device);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // it allocates: not inside a capture
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return -EINVAL;
    if (validate_check(cfg) != 0) return -EINVAL;
    int rc = 0;
    if (hipMalloc(&st.d_hits, kValidHitCells * sizeof(unsigned long long)) != hipSuccess) {
        st.d_hits = nullptr;
        rc = -ENOMEM;
    } else if (hipMemsetAsync(st.d_hits, 0, kValidHitCells * sizeof(unsigned long long), c->stream) != hipSuccess) {
        rc = -EIO;
    }
    if (rc) {
        (void)hipGetLastError();
        free_ptr(st.d_hits);
        memset(&st, 0, sizeof(st));
        return rc;
    }
    st.cfg = *cfg;
    st.open = 1;
    return 0;
}

int sr_validate_close(sr_ctx *c) {
    if (!c) return -EINVAL;
    ValidateStage &st = c->validate;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!st.open) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_ptr(st.d_hits);
    free_ptr(st.d_reason);
    free_ptr(st.d_tiles);
    memset(&st, 0, sizeof(st));
    c->validate_on = 0;
    return 0;
}

int sr_validate(sr_ctx *c, const sr_validate_batch *batches, size_t count) {
    static_assert(kValidMaxBatches == (int)SR_MAX_BATCHES_PER_LAUNCH, "launch batch limit");
    if (!c || !c->validate.open || !batches || count == 0 || count > (size_t)kValidMaxBatches) return -EINVAL;
    ValidateStage &st = c->validate;
    size_t records = 0, tiles = 0;   // the scratch's sizes, by max_records
    uint64_t grid_tiles = 0;         // the grid's bound only (the kernels number the tiles by the device's counts)
    for (size_t j = 0; j < count; ++j) {
        const sr_validate_batch &b = batches[j];
        if (!b.d_n_records || !b.d_counts || (b.nbytes && !b.d_bytes)) return -EINVAL;
        if (b.max_records && (!b.d_recs || !b.d_out || b.d_out == b.d_recs)) return -EINVAL;
        if (b.d_hashes && b.d_hashes_out == b.d_hashes) return -EINVAL;
        if ((const void *)b.d_counts == (const void *)b.d_n_records) return -EINVAL;   // read after the counts are written
        if (b.nbytes > 0xFFFFFFF0ull || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if (!b.d_reason) records += b.max_records;
        tiles += (b.max_records + kValidTile - 1) / kValidTile;
        const uint64_t likely = (uint64_t)b.nbytes / kValidGridLineBytes + 1u;
        const uint64_t room = b.max_records < likely ? b.max_records : likely;
        grid_tiles += (room + kValidTile - 1) / kValidTile;
    }
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = grow((void **)&st.d_reason, &st.reason_cap, records, sizeof(uint8_t)))) return rc;
    if ((rc = grow((void **)&st.d_tiles, &st.tiles_cap, tiles, sizeof(uint4)))) return rc;
    ValidateArgs a;
    memset(&a, 0, sizeof(a));
    size_t at = 0;
    for (size_t j = 0; j < count; ++j) {
        const sr_validate_batch &b = batches[j];
        ValidateBatchArg &o = a.b[j];
        const bool hashes = b.d_hashes && b.d_hashes_out;
        o.bytes = b.d_bytes;
        o.recs = b.d_recs;
        o.n_records = b.d_n_records;
        o.hashes = hashes ? b.d_hashes : nullptr;
        o.out = b.d_out;
        o.hashes_out = hashes ? b.d_hashes_out : nullptr;
        o.reason = b.d_reason ? b.d_reason : st.d_reason + at;
        o.counts = b.d_counts;
        o.nbytes = (uint32_t)b.nbytes;
        o.max_records = (uint32_t)b.max_records;
        if (!b.d_reason) at += b.max_records;
    }
    a.hits = st.d_hits;
    a.tiles = st.d_tiles;
    a.nb = (uint32_t)count;
    a.nds = c->ds.nds;
    a.drop_mask = st.cfg.drop_mask;
    a.accept_types = st.cfg.accept_types;
    if (grid_tiles) {
        const dim3 grid((uint32_t)(grid_tiles < (uint64_t)kValidGroups ? grid_tiles : (uint64_t)kValidGroups));
        hipLaunchKernelGGL(validate_check_kernel, grid, dim3(kValidBlock), 0, c->stream, a);
        hipLaunchKernelGGL(validate_scan_kernel, dim3((uint32_t)count), dim3(kValidScanBlock), 0, c->stream, a);
        hipLaunchKernelGGL(validate_emit_kernel, grid, dim3(kValidBlock), 0, c->stream, a);
    } else {   // no batch has room for a record: the counts alone
        hipLaunchKernelGGL(validate_scan_kernel, dim3((uint32_t)count), dim3(kValidScanBlock), 0, c->stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_validate_read(sr_ctx *c, sr_validate_hits *hits, size_t n) {
    static_assert(sizeof(sr_validate_hits) == 2 * sizeof(unsigned long long), "a hit is two cells");
    if (!c || !c->validate.open || (n && !hits)) return -EINVAL;
    const size_t m = n < (size_t)SR_VALID_REASONS ? n : (size_t)SR_VALID_REASONS;
    (void)hipSetDevice(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -EIO;
    if (m && hipMemcpy(hits, c->validate.d_hits, m * sizeof(sr_validate_hits), hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
    return (int)m;
}

int sr_validate_reset(sr_ctx *c) {
    if (!c || !c->validate.open) return -EINVAL;
    (void)hipSetDevice(c->device);
    return hipMemsetAsync(c->validate.d_hits, 0, kValidHitCells * sizeof(unsigned long long), c->stream) == hipSuccess ? 0 : -EIO;
}

int sr_validate_check(const sr_validate_config *cfg) { return validate_check(cfg); }

int sr_validate_line(const sr_validate_config *cfg, const uint8_t *line, size_t len) {
    if (validate_check(cfg) != 0 || !line || len == 0) return -EINVAL;
    return (int)validate_line(line, len, cfg->accept_types);
}

const char *sr_validate_reason_name(uint32_t reason) { return validate_reason_name(reason); }

int sr_validate_parse_spec(const char *text, sr_validate_config *cfg_out) { return validate_parse_spec(text, cfg_out); }

int sr_set_validate(sr_ctx *c, const sr_validate_config *cfg) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!cfg) {
        c->validate_on = 0;
        return 0;
    }
    int rc = validate_check(cfg);   // a bad configuration leaves the stage as it was
    if (rc) return rc;
    if (c->validate.open && (rc = sr_validate_close(c))) return rc;
    if ((rc = sr_validate_open(c, cfg))) return rc;
    (void)hipSetDevice(c->device);
    if (!c->d_vcounts && hipMalloc(&c->d_vcounts, 4 * sizeof(uint64_t)) != hipSuccess) {
        c->d_vcounts = nullptr;
        return -ENOMEM;
    }
    c->validate_on = 1;
    return 0;
}

int sr_route_pack_validate(sr_ctx *c, int slot, uint64_t counts[4]) {
    if (!c || !counts || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.validated || !sl.vhost) return -EBUSY;
    for (int q = 0; q < 4; ++q) counts[q] = sl.vhost[q];
    return 0;
}

// ---- sample rates (sample_kernel.hpp, sample_host.hpp) ------------------------------------------------------
int sr_sample_open(sr_ctx *c, const sr_sample_config *cfg) {
    if (!c) return -EINVAL;
    SampleStage &st = c->sample;
    if (st.open) return -EBUSY;
    (void)hipSetDevice(c->device);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // it allocates: not inside a capture
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return -EINVAL;
    if (sample_check(cfg) != 0) return -EINVAL;
    const uint32_t slots = sample_resolve_slots(cfg->slots);
    int rc = 0;
    if (hipMalloc(&st.d_table, (size_t)kSampleMaxBatches * slots * sizeof(uint32_t)) != hipSuccess) {
        st.d_table = nullptr;
        rc = -ENOMEM;
    } else if (hipMalloc(&st.d_hits, kSampleHitCells * sizeof(unsigned long long)) != hipSuccess) {
        st.d_hits = nullptr;
        rc = -ENOMEM;
    } else if (hipMemsetAsync(st.d_hits, 0, kSampleHitCells * sizeof(unsigned long long), c->stream) != hipSuccess) {
        rc = -EIO;
    }
    if (rc) {
        (void)hipGetLastError();
        free_ptr(st.d_table);
        free_ptr(st.d_hits);
        memset(&st, 0, sizeof(st));
        return rc;
    }
    st.cfg = *cfg;
    st.slots = slots;
    st.open = 1;
    return 0;
}

int sr_sample_close(sr_ctx *c) {
    if (!c) return -EINVAL;
    SampleStage &st = c->sample;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!st.open) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_ptr(st.d_table);
    free_ptr(st.d_hits);
    free_ptr(st.d_scratch);
    free_ptr(st.d_tiles);
    memset(&st, 0, sizeof(st));
    c->sample_on = 0;
    return 0;
}

int sr_sample(sr_ctx *c, const sr_sample_batch *batches, size_t count) {
    static_assert(kSampleMaxBatches == (int)SR_MAX_BATCHES_PER_LAUNCH, "launch batch limit");
    if (!c || !c->sample.open || !batches || count == 0 || count > (size_t)kSampleMaxBatches) return -EINVAL;
    SampleStage &st = c->sample;
    size_t records = 0, tiles = 0;   // the scratch's sizes, by max_records
    uint64_t grid_tiles = 0;         // the grid's bound only (the kernels number the tiles by the device's counts)
    for (size_t j = 0; j < count; ++j) {
        const sr_sample_batch &b = batches[j];
        if (!b.d_n_records || !b.d_counts || !b.d_hashes || ((b.nbytes || b.append_cap) && !b.d_bytes)) return -EINVAL;
        if (b.max_records && (!b.d_recs || !b.d_out || b.d_out == b.d_recs)) return -EINVAL;
        if (b.d_hashes_out == b.d_hashes) return -EINVAL;
        if ((const void *)b.d_counts == (const void *)b.d_n_records) return -EINVAL;   // read after the counts are written
        if (b.nbytes > SR_SAMPLE_MAX_BYTES || b.max_records > 0xFFFFFFF0ull) return -EINVAL;
        if (b.append_cap > 0xFFFFFFF0ull || (uint64_t)b.nbytes + b.append_cap > 0xFFFFFFF0ull) return -EINVAL;
        records += b.max_records;
        tiles += (b.max_records + kSampleTile - 1) / kSampleTile;
        const uint64_t likely = (uint64_t)b.nbytes / kSampleGridLineBytes + 1u;
        const uint64_t room = b.max_records < likely ? b.max_records : likely;
        grid_tiles += (room + kSampleTile - 1) / kSampleTile;
    }
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = grow((void **)&st.d_scratch, &st.scratch_cap, records, sizeof(uint32_t)))) return rc;
    if ((rc = grow((void **)&st.d_tiles, &st.tiles_cap, tiles, sizeof(uint4)))) return rc;
    SampleArgs a;
    memset(&a, 0, sizeof(a));
    size_t at = 0;
    for (size_t j = 0; j < count; ++j) {
        const sr_sample_batch &b = batches[j];
        SampleBatchArg &o = a.b[j];
        o.bytes = b.d_bytes;
        o.recs = b.d_recs;
        o.n_records = b.d_n_records;
        o.hashes = b.d_hashes;
        o.out = b.d_out;
        o.hashes_out = b.d_hashes_out;
        o.step = b.d_step;
        o.counts = b.d_counts;
        o.scratch = st.d_scratch + at;
        o.table = st.d_table + j * (size_t)st.slots;   // back to back: sample_clear_kernel zeroes them as one
        o.append_cap = b.append_cap;
        o.seed = st.cfg.seed + b.seed_add;
        o.nbytes = (uint32_t)b.nbytes;
        o.max_records = (uint32_t)b.max_records;
        at += b.max_records;
    }
    a.hits = st.d_hits;
    a.tiles = st.d_tiles;
    a.nb = (uint32_t)count;
    a.nds = c->ds.nds;
    a.slots = st.slots;
    a.limit = st.cfg.limit;
    a.types = st.cfg.types;
    if (grid_tiles) {
        const dim3 grid((uint32_t)(grid_tiles < (uint64_t)kSampleGroups ? grid_tiles : (uint64_t)kSampleGroups));
        const uint64_t clear = ((uint64_t)count * st.slots / 4u + kSampleBlock - 1) / kSampleBlock;
        hipLaunchKernelGGL(sample_clear_kernel, dim3((uint32_t)(clear < (uint64_t)kSampleGroups ? clear : (uint64_t)kSampleGroups)),
                           dim3(kSampleBlock), 0, c->stream, a);
        hipLaunchKernelGGL(sample_count_kernel, grid, dim3(kSampleBlock), 0, c->stream, a);
        hipLaunchKernelGGL(sample_sum_kernel, grid, dim3(kSampleBlock), 0, c->stream, a);
        hipLaunchKernelGGL(sample_scan_kernel, dim3((uint32_t)count), dim3(kSampleScanBlock), 0, c->stream, a);
        hipLaunchKernelGGL(sample_emit_kernel, grid, dim3(kSampleBlock), 0, c->stream, a);
    } else {   // no batch has room for a record: the counts alone
        hipLaunchKernelGGL(sample_scan_kernel, dim3((uint32_t)count), dim3(kSampleScanBlock), 0, c->stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

int sr_sample_read(sr_ctx *c, sr_sample_hits *hits, size_t n) {
    static_assert(sizeof(sr_sample_hits) == 2 * sizeof(unsigned long long), "a hit is two cells");
    if (!c || !c->sample.open || (n && !hits)) return -EINVAL;
    const size_t m = n < (size_t)SR_SAMPLE_STEPS ? n : (size_t)SR_SAMPLE_STEPS;
    (void)hipSetDevice(c->device);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -EIO;
    if (m && hipMemcpy(hits, c->sample.d_hits, m * sizeof(sr_sample_hits), hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
    return (int)m;
}

int sr_sample_reset(sr_ctx *c) {
    if (!c || !c->sample.open) return -EINVAL;
    (void)hipSetDevice(c->device);
    return hipMemsetAsync(c->sample.d_hits, 0, kSampleHitCells * sizeof(unsigned long long), c->stream) == hipSuccess ? 0 : -EIO;
}

int sr_sample_check(const sr_sample_config *cfg) { return sample_check(cfg); }

int sr_sample_parse(const uint8_t *line, size_t len, uint32_t types, uint32_t *ins, uint32_t *type_bit) {
    if (!line) return -EINVAL;
    return sample_parse(line, len, types, ins, type_bit);
}

uint32_t sr_sample_step(uint32_t limit, uint64_t count) { return sample_step(limit, count); }

int sr_sample_keep(uint64_t hash, uint64_t seed, uint64_t index, uint32_t step) {
    if (step >= SR_SAMPLE_STEPS) return -EINVAL;
    return (int)sample_keep(hash, seed, index, step);
}

const char *sr_sample_rate_text(uint32_t step) { return sample_rate_text(step); }

size_t sr_sample_rewrite(uint8_t *dst, const uint8_t *line, size_t len, uint32_t ins, uint32_t step) {
    return sample_rewrite(dst, line, len, ins, step);
}

int sr_sample_parse_spec(const char *text, sr_sample_config *cfg_out) { return sample_parse_spec(text, cfg_out); }

int sr_set_sample(sr_ctx *c, const sr_sample_config *cfg) {
    if (!c) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (!cfg) {
        c->sample_on = 0;
        return 0;
    }
    int rc = sample_check(cfg);   // a bad configuration leaves the stage as it was
    if (rc) return rc;
    if (c->ds.max_batch > SR_SAMPLE_MAX_BYTES) return -EINVAL;
    (void)hipSetDevice(c->device);
    if ((rc = input_reserve(c, true, c->d_ccounts != nullptr))) return rc;
    if (c->sample.open && (rc = sr_sample_close(c))) return rc;
    if ((rc = sr_sample_open(c, cfg))) return rc;
    if (!c->d_scounts && hipMalloc(&c->d_scounts, 4 * sizeof(uint64_t)) != hipSuccess) {
        c->d_scounts = nullptr;
        return -ENOMEM;
    }
    c->sample_subs = 0;
    c->sample_on = 1;
    return 0;
}

int sr_route_pack_sample(sr_ctx *c, int slot, const uint8_t **text, size_t *len, uint64_t counts[4], uint64_t *seed) {
    if (!c || !text || !len || !counts || !seed || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.sampled || !sl.shost) return -EBUSY;
    const uint64_t *hc = (const uint64_t *)(sl.shost + ((sl.stext_cap + 255) & ~(size_t)255));
    for (int q = 0; q < 4; ++q) counts[q] = hc[q];
    *text = sl.shost;
    *len = (size_t)(hc[3] < sl.stext_cap ? hc[3] : sl.stext_cap);
    *seed = sl.sseed;
    return hc[3] > sl.stext_cap ? -ENOSPC : 0;
}

// Host outputs of a slot for batches of up to nbytes (grown, never shrunk; the slot is idle).
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int slot_reserve(sr_ctx *c, int k, size_t nbytes) {
    sr_ctx::Slot &sl = c->slot[k];
    const size_t nds = c->ds.nds, nw = c->ds.nwords ? c->ds.nwords : 1;
    const size_t rec = nbytes, pk = (size_t)SR_MAX_PACKETS(nbytes, c->ds.nds);
    if (!sl.done && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) {
        sl.done = nullptr;
        return -ENOMEM;
    }
    if (sl.host && rec <= sl.rec_cap && pk <= sl.pk_cap) return 0;
    if (sl.host) (void)hipHostFree(sl.host);
    sl.host = sl.dev = nullptr;
    sl.rec_cap = sl.pk_cap = 0;
    const size_t o_pk = up256(rec * sizeof(sr_record)), o_fill = o_pk + up256(pk * sizeof(sr_packet));
    const size_t o_pr = o_fill + up256(nds * sizeof(uint16_t) + 2), o_cnt = o_pr + up256(nw * sizeof(uint64_t));
    const size_t o_fin = o_cnt + 256, o_lens = o_fin + up256(nds * sizeof(uint16_t) + 2);
    const size_t total = o_lens + up256((size_t)SR_MAX_SLOTS * sizeof(uint16_t));
    void *h = nullptr;
    if (hipHostMalloc(&h, total, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.host = (uint8_t *)h;
    sl.dev = (uint8_t *)d;
    sl.rec_cap = rec;
    sl.pk_cap = pk;
    sl.sorted = (sr_record *)sl.host;
    sl.packets = (sr_packet *)(sl.host + o_pk);
    sl.fill = (uint16_t *)(sl.host + o_fill);
    sl.probed = (uint64_t *)(sl.host + o_pr);
    sl.counts = (uint64_t *)(sl.host + o_cnt);
    sl.fill_in = (uint16_t *)(sl.host + o_fin);
    sl.lens_in = (uint16_t *)(sl.host + o_lens);
    return 0;
}

// sr_set_trace: the slot's input-order records and hashes (grown, never shrunk; the slot is idle)
static int slot_trace_reserve(sr_ctx *c, int k, size_t nbytes) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.thost && nbytes <= sl.trec_cap) return 0;
    if (sl.thost) (void)hipHostFree(sl.thost);
    sl.thost = sl.tdev = nullptr;
    sl.trec_cap = 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, up256(nbytes * sizeof(sr_record)) + nbytes * sizeof(uint64_t) + 8, hipHostMallocMapped) !=
        hipSuccess)
        return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.thost = (uint8_t *)h;
    sl.tdev = (uint8_t *)d;
    sl.trec_cap = nbytes;
    return 0;
}

// sr_set_payloads: the slot's arena, offsets and total (grown, never shrunk; the slot is idle):
// arena | offsets (descriptors + 1) | total
static int slot_payload_reserve(sr_ctx *c, int k, size_t nbytes) {
    sr_ctx::Slot &sl = c->slot[k];
    const size_t cap = (size_t)SR_PAYLOAD_CAPACITY(nbytes, c->ds.nds), pk = (size_t)SR_MAX_PACKETS(nbytes, c->ds.nds);
    if (sl.phost && cap <= sl.pay_cap && pk <= sl.poff_cap) return 0;
    if (sl.phost) (void)hipHostFree(sl.phost);
    sl.phost = sl.pdev = nullptr;
    sl.pay_cap = sl.poff_cap = 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, up256(cap) + up256((pk + 1) * sizeof(uint32_t)) + 256, hipHostMallocMapped) != hipSuccess)
        return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.phost = (uint8_t *)h;
    sl.pdev = (uint8_t *)d;
    sl.pay_cap = cap;
    sl.poff_cap = pk;
    return 0;
}

// sr_set_coalesce: the slot's merged text and counts (grown, never shrunk; the slot is idle): text | 5 u64
static int slot_coalesce_reserve(sr_ctx *c, int k, size_t nbytes) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.chost && nbytes <= sl.ctext_cap) return 0;
    if (sl.chost) (void)hipHostFree(sl.chost);
    sl.chost = sl.cdev = nullptr;
    sl.ctext_cap = 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, up256(nbytes) + 256, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.chost = (uint8_t *)h;
    sl.cdev = (uint8_t *)d;
    sl.ctext_cap = nbytes;
    return 0;
}

// sr_set_name_rules: the slot's counts (the slot is idle): 4 counts and the input's record count
static int slot_rules_reserve(sr_ctx *c, int k) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.rhost) return 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.rhost = (uint64_t *)h;
    sl.rdev = (uint64_t *)d;
    return 0;
}

// sr_set_validate: the slot's counts (the slot is idle): 4 counts and the input's record count
static int slot_validate_reserve(sr_ctx *c, int k) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.vhost) return 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.vhost = (uint64_t *)h;
    sl.vdev = (uint64_t *)d;
    return 0;
}

// sr_set_sample: the slot's rewritten text and counts (grown, never shrunk; the slot is idle): text | 5 u64
static int slot_sample_reserve(sr_ctx *c, int k, size_t text_bytes) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.shost && text_bytes <= sl.stext_cap) return 0;
    if (sl.shost) (void)hipHostFree(sl.shost);
    sl.shost = sl.sdev = nullptr;
    sl.stext_cap = 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, up256(text_bytes) + 256, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.shost = (uint8_t *)h;
    sl.sdev = (uint8_t *)d;
    sl.stext_cap = text_bytes;
    return 0;
}

// sr_set_logtext: the slot's text arena, index, totals and the staging of prefixes and ends (sized by the
// switch, which only changes while every slot is idle)
struct LogLayout {
    size_t o_off, o_lv, o_tot, o_pfx, o_ends, total;
};
static LogLayout log_layout(size_t text_cap, size_t msgs) {
    LogLayout l;
    l.o_off = up256(text_cap);
    l.o_lv = l.o_off + up256((msgs + 1) * sizeof(uint32_t));
    l.o_tot = l.o_lv + up256(msgs);
    l.o_pfx = l.o_tot + 256;
    l.o_ends = l.o_pfx + up256(2 * (size_t)kLogMaxPrefix);
    l.total = l.o_ends + up256((size_t)SR_MAX_SLOTS * sizeof(uint32_t));
    return l;
}
static int slot_log_reserve(sr_ctx *c, int k) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.lhost && sl.ltext_cap == c->log_cap && sl.lmsg_cap == c->log_msgs) return 0;
    if (sl.lhost) (void)hipHostFree(sl.lhost);
    sl.lhost = sl.ldev = nullptr;
    sl.ltext_cap = sl.lmsg_cap = 0;
    sl.stage_plen[0] = sl.stage_plen[1] = 0;
    sl.stage_ends = 0;
    sl.logged = 0;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, log_layout(c->log_cap, c->log_msgs).total, hipHostMallocMapped) != hipSuccess) return -ENOMEM;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return -EIO;
    }
    sl.lhost = (uint8_t *)h;
    sl.ldev = (uint8_t *)d;
    sl.ltext_cap = c->log_cap;
    sl.lmsg_cap = c->log_msgs;
    return 0;
}

// The datagrams of a slot submission (sr_route_pack_submit_slots): framed on the device into c->d_in.
struct SlotSource {
    const uint8_t *d_slots;   // the device address of the caller's page-locked slots
    size_t stride;
    const uint16_t *lens;
    size_t count;
};

// src == nullptr: `bytes` is a framed batch in host memory. Otherwise nbytes is the framed size of src's
// datagrams (sr_frame_slots_size, > 0) and `bytes` is unused.
static int pack_submit(sr_ctx *c, int k, const uint8_t *bytes, size_t nbytes, const uint16_t *fill,
                       const SlotSource *src = nullptr) {
    sr_ctx::Slot &sl = c->slot[k];
    if (sl.busy) return -EBUSY;
    if ((nbytes && !bytes && !src) || nbytes > c->ds.max_batch) return -EINVAL;
    if (c->ds.nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    if (!src && nbytes && bytes[nbytes - 1] != '\n') return -EINVAL;
    if (c->logtext && c->log_max_msg && sl.lhost &&
        (c->log_max_msg <= sl.stage_plen[0] || c->log_max_msg <= sl.stage_plen[1]))
        return -EINVAL;   // sr_format_log would refuse it after the route was enqueued
    (void)hipSetDevice(c->device);
    const size_t nds = c->ds.nds, nw = c->ds.nwords;
    int rc;
    // every buffer is sized for the context's largest batch at the first submission (an empty one
    // pre-allocates): growing page-locked memory or freeing device memory mid-stream would stall the
    // data thread while its socket fills
    // (with the sample rates on a kept line may be up to 8 bytes longer: the thinned batch has at most
    // SR_SAMPLE_APPEND_CAPACITY(nbytes) bytes, which then sizes the packets and the payloads)
    const bool sample = c->sample_on != 0;
    const size_t full = c->ds.max_batch, fulls = sample ? (size_t)SR_SAMPLE_APPEND_CAPACITY(full) : full;
    const size_t fullp = (size_t)SR_MAX_PACKETS(fulls, nds);
    if ((rc = slot_reserve(c, k, fulls))) return rc;
    if (c->trace && (rc = slot_trace_reserve(c, k, full))) return rc;
    if (c->payloads && (rc = slot_payload_reserve(c, k, fulls))) return rc;
    if (sample && (rc = slot_sample_reserve(c, k, (size_t)SR_SAMPLE_APPEND_CAPACITY(full)))) return rc;
    if (c->logtext && (rc = slot_log_reserve(c, k))) return rc;
    const bool coalesce = c->coalesce_on != 0;
    if (coalesce && (rc = slot_coalesce_reserve(c, k, full))) return rc;
    const bool rules = c->rules_on != 0;
    if (rules && (rc = slot_rules_reserve(c, k))) return rc;
    const bool validate = c->validate_on != 0;
    if (validate && (rc = slot_validate_reserve(c, k))) return rc;
    const bool log_trace = c->logtext && c->log_level == 0;   // the formatter needs hashes and datagram ends
    if (log_trace && src && !c->d_ends && hipMalloc(&c->d_ends, (size_t)SR_MAX_SLOTS * sizeof(uint32_t)) != hipSuccess) {
        c->d_ends = nullptr;
        return -ENOMEM;
    }
    const size_t cap = nbytes ? nbytes : 1;   // never more lines than bytes
    const size_t arena = sample ? (size_t)SR_SAMPLE_APPEND_CAPACITY(nbytes) : 0;   // behind the batch in d_in
    const size_t pcap = (size_t)SR_MAX_PACKETS(sample ? (size_t)SR_SAMPLE_APPEND_CAPACITY(cap) : cap, nds);
    const uint64_t seed_add = c->sample_subs;
    if ((rc = grow((void **)&c->d_out, &c->d_out_cap, full, sizeof(sr_record)))) return rc;
    if ((rc = grow((void **)&c->d_sorted, &c->d_sorted_cap, full, sizeof(sr_record)))) return rc;
    if ((rc = grow((void **)&c->d_packets, &c->d_packets_cap, fullp, sizeof(sr_packet)))) return rc;
    if (!c->d_fill) {
        if (hipMalloc(&c->d_fill, (3 * nds + 2) * sizeof(uint16_t)) != hipSuccess) {
            c->d_fill = nullptr;
            return -ENOMEM;
        }
        if (hipMemsetAsync(c->d_fill, 0, (3 * nds + 2) * sizeof(uint16_t), c->stream) != hipSuccess) return -EIO;
        c->fill_cur = 0;
    }
    if (!c->d_mcounts && hipMalloc(&c->d_mcounts, 4 * sizeof(uint64_t)) != hipSuccess) return -ENOMEM;
    uint16_t *const f_in = fill ? c->d_fill + 2 * nds : c->d_fill + (size_t)c->fill_cur * nds;
    uint16_t *const f_out = c->d_fill + (size_t)(c->fill_cur ^ 1) * nds;
    if (fill && nds) {   // staged in the slot's page-locked memory: the caller's array is free on return
        memcpy(sl.fill_in, fill, nds * sizeof(uint16_t));
        if (hipMemcpyAsync(f_in, sl.fill_in, nds * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return -EIO;
    }
    if (nbytes == 0) {   // no lines: the fills carry over, nothing is probed
        if (nds && hipMemcpyAsync(f_out, f_in, nds * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            return -EIO;
        if (hipMemsetAsync(c->d_mcounts, 0, 4 * sizeof(uint64_t), c->stream) != hipSuccess) return -EIO;
    } else {
        if (src) {   // the lengths staged like the fill; the datagrams read in place, no bulk copy
            memcpy(sl.lens_in, src->lens, src->count * sizeof(uint16_t));
            const sr_slot_batch fb{src->d_slots, src->stride, (const uint16_t *)(sl.dev + ((uint8_t *)sl.lens_in - sl.host)),
                                   src->count, c->d_in, c->ds.max_batch, log_trace ? c->d_ends : nullptr,
                                   (uint64_t *)(sl.dev + ((uint8_t *)(sl.counts + 3) - sl.host))};
            if ((rc = frame_impl(c, &fb))) return rc;
        } else if (hipMemcpyAsync(c->d_in, bytes, nbytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            return -EIO;
        }
        // over 1024 shards with some dead the route kernel also writes the hashes: the probed-dead
        // replay then reads 8 bytes per line instead of re-hashing the names (probed_dead_kernel);
        // up to 1024 the probes note the dead shards themselves
        // TRACE (sr_set_trace) needs every line's hash too (sr-main.c:91), and so do the name statistics
        uint64_t *hashes = nullptr;
        if (c->trace || log_trace || c->name_stats || coalesce || sample || c->ds.replay_wants_hashes()) {
            if ((rc = grow((void **)&c->d_hash, &c->d_hash_cap, full, sizeof(uint64_t)))) return rc;
            hashes = c->d_hash;
        }
        const sr_batch rb{c->d_in, nbytes, c->d_out, cap, hashes, c->d_count, c->d_probed};
        if (rules || validate || sample) {   // route, validate, rules, sample, coalesce, pack: each stage that is on
                                             // reads the one before's records, count and (for the sample rates and
                                             // the coalescing) hashes
            const bool later_hs = coalesce || sample;   // a later stage takes the hashes
            if (coalesce && !c->d_cout && hipMalloc(&c->d_cout, full * sizeof(sr_record)) != hipSuccess) {
                c->d_cout = nullptr;
                return -ENOMEM;
            }
            RouteParams p = c->ds.params();
            DeviceState::add_batch(p, rb.d_bytes, rb.nbytes, rb.d_out, rb.max_records, rb.d_hashes, rb.d_n_records,
                                   rb.d_probed_dead);
            if ((rc = launch_variant(c->ds, p, c->stream))) return rc;
            const sr_record *recs = c->d_out;
            const uint64_t *cnt = c->d_count, *hs = later_hs ? c->d_hash : nullptr;
            if (validate) {
                if ((rc = grow((void **)&c->d_vout, &c->d_vout_cap, full, sizeof(sr_record)))) return rc;
                if (later_hs && (rc = grow((void **)&c->d_vhash, &c->d_vhash_cap, full, sizeof(uint64_t)))) return rc;
                const sr_validate_batch vb{c->d_in, nbytes, recs, cnt, cap, c->d_vout, hs, later_hs ? c->d_vhash : nullptr,
                                           nullptr, c->d_vcounts};
                if ((rc = sr_validate(c, &vb, 1))) return rc;
                recs = c->d_vout;
                cnt = c->d_vcounts;
                hs = later_hs ? c->d_vhash : nullptr;
            }
            if (rules) {
                if ((rc = grow((void **)&c->d_rout, &c->d_rout_cap, full, sizeof(sr_record)))) return rc;
                if (later_hs && (rc = grow((void **)&c->d_rhash, &c->d_rhash_cap, full, sizeof(uint64_t)))) return rc;
                const sr_rules_batch ub{c->d_in, nbytes, recs, cnt, cap, c->d_rout, hs, later_hs ? c->d_rhash : nullptr,
                                        nullptr, c->d_rcounts};
                if ((rc = sr_rules(c, &ub, 1))) return rc;
                recs = c->d_rout;
                cnt = c->d_rcounts;
                hs = later_hs ? c->d_rhash : nullptr;
            }
            if (sample) {   // the rewritten lines go behind the batch; the coalescing takes both as its batch
                if ((rc = grow((void **)&c->d_sout, &c->d_sout_cap, full, sizeof(sr_record)))) return rc;
                if (coalesce && (rc = grow((void **)&c->d_shash, &c->d_shash_cap, full, sizeof(uint64_t)))) return rc;
                const sr_sample_batch mb{c->d_in, nbytes, arena, recs, cnt, cap, hs, c->d_sout, coalesce ? c->d_shash : nullptr,
                                         nullptr, c->d_scounts, seed_add};
                if ((rc = sr_sample(c, &mb, 1))) return rc;
                recs = c->d_sout;
                cnt = c->d_scounts;
                hs = coalesce ? c->d_shash : nullptr;
            }
            if (coalesce) {
                const sr_coalesce_batch cb{c->d_in, nbytes + arena, nbytes, recs, cnt, cap, hs, c->d_cout, c->d_ccounts};
                if ((rc = sr_coalesce(c, &cb, 1))) return rc;
                recs = c->d_cout;
                cnt = c->d_ccounts;
            }
            const sr_pack_batch pb{recs, cnt, cap, f_in, c->d_probed, c->d_sorted, c->d_packets, pcap, c->d_mcounts, f_out};
            if ((rc = pack_many_impl(c, &pb, 1, nullptr, nullptr))) return rc;
        } else if (!coalesce) {
            const sr_pack_batch pb{c->d_out, c->d_count, cap, f_in, c->d_probed, c->d_sorted, c->d_packets, pcap,
                                   c->d_mcounts, f_out};
            if ((rc = route_pack_impl(c, &rb, &pb, 1))) return rc;
        } else {   // route, coalesce, pack: the packing reads the coalesced records and their count
            if (!c->d_cout && hipMalloc(&c->d_cout, full * sizeof(sr_record)) != hipSuccess) {
                c->d_cout = nullptr;
                return -ENOMEM;
            }
            RouteParams p = c->ds.params();
            DeviceState::add_batch(p, rb.d_bytes, rb.nbytes, rb.d_out, rb.max_records, rb.d_hashes, rb.d_n_records,
                                   rb.d_probed_dead);
            if ((rc = launch_variant(c->ds, p, c->stream))) return rc;
            const sr_coalesce_batch cb{c->d_in, nbytes, nbytes, c->d_out, c->d_count, cap, c->d_hash, c->d_cout, c->d_ccounts};
            if ((rc = sr_coalesce(c, &cb, 1))) return rc;
            const sr_pack_batch pb{c->d_cout, c->d_ccounts, cap, f_in, c->d_probed, c->d_sorted, c->d_packets, pcap,
                                   c->d_mcounts, f_out};
            if ((rc = pack_many_impl(c, &pb, 1, nullptr, nullptr))) return rc;
        }
    }
    c->fill_cur ^= 1;
    PackOut o;
    o.sorted = c->d_sorted;
    o.packets = c->d_packets;
    o.fill = f_out;
    o.probed = (nbytes && c->ds.dead) ? c->d_probed : nullptr;
    o.counts = c->d_mcounts;
    o.rec_cap = sl.rec_cap;
    o.pk_cap = sl.pk_cap;
    o.nds = (uint32_t)nds;
    o.nwords = (uint32_t)nw;
    o.h_sorted = (sr_record *)(sl.dev + ((uint8_t *)sl.sorted - sl.host));
    o.h_packets = (sr_packet *)(sl.dev + ((uint8_t *)sl.packets - sl.host));
    o.h_fill = (uint16_t *)(sl.dev + ((uint8_t *)sl.fill - sl.host));
    o.h_probed = (uint64_t *)(sl.dev + ((uint8_t *)sl.probed - sl.host));
    o.h_counts = (uint64_t *)(sl.dev + ((uint8_t *)sl.counts - sl.host));
    sl.framed = src != nullptr;
    sl.frame_bytes = nbytes;
    sl.traced = c->trace;
    // input order, and the hashes (sr_route_pack_trace); with the coalescing on coalesce_out_kernel copies them,
    // by the input's count
    // (with the name rules on rules_out_kernel does, unless the coalescing is on too)
    // (and with the line grammar on validate_out_kernel does, unless one of those two is on too)
    // (and with the sample rates on sample_out_kernel does, unless one of those three is on too)
    o.recs = (c->trace && nbytes && !coalesce && !rules && !validate && !sample) ? c->d_out : nullptr;
    o.hashes = (c->trace && nbytes && !coalesce && !rules && !validate && !sample) ? c->d_hash : nullptr;
    o.h_recs = c->trace ? (sr_record *)sl.tdev : nullptr;
    o.h_hashes = c->trace ? (uint64_t *)(sl.tdev + up256(sl.trec_cap * sizeof(sr_record))) : nullptr;
    // one workgroup per 512 records (two per thread), at most 1024 workgroups (grid-stride beyond)
    const uint64_t want = (cap + 511) / 512;
    hipLaunchKernelGGL(pack_out_kernel, dim3((uint32_t)(want < 1024 ? (want ? want : 1) : 1024)), dim3(256), 0,
                       c->stream, o);
    if (hipGetLastError() != hipSuccess) return -EIO;
    sl.coalesced = coalesce;
    if (coalesce) {   // the merged text, the counts and the input's record count into the slot's page-locked memory
        uint64_t *const hc = (uint64_t *)(sl.chost + up256(sl.ctext_cap));
        if (nbytes == 0) {
            for (int q = 0; q < 5; ++q) hc[q] = 0;   // the slot is idle: nothing is in flight that writes here
        } else {
            CoalesceOut co;
            co.text = c->d_in + nbytes + arena;
            co.counts = c->d_ccounts;
            co.n_records = c->d_count;
            co.text_cap = nbytes < sl.ctext_cap ? nbytes : sl.ctext_cap;
            co.rec_cap = c->trace ? sl.trec_cap : 0;
            co.h_text = sl.cdev;
            co.h_counts = (uint64_t *)(sl.cdev + up256(sl.ctext_cap));
            co.recs = c->trace ? c->d_out : nullptr;
            co.hashes = c->trace ? c->d_hash : nullptr;
            co.h_recs = c->trace ? (sr_record *)sl.tdev : nullptr;
            co.h_hashes = c->trace ? (uint64_t *)(sl.tdev + up256(sl.trec_cap * sizeof(sr_record))) : nullptr;
            hipLaunchKernelGGL(coalesce_out_kernel, dim3((uint32_t)(want < 1024 ? (want ? want : 1) : 1024)),
                               dim3(kCoalesceBlock), 0, c->stream, co);
            if (hipGetLastError() != hipSuccess) return -EIO;
        }
    }
    sl.ruled = rules;
    if (rules) {   // the stage's counts and the input's record count into the slot's page-locked memory
        if (nbytes == 0) {
            for (int q = 0; q < 5; ++q) sl.rhost[q] = 0;   // the slot is idle: nothing is in flight that writes here
        } else {
            const bool tr = c->trace && !coalesce;
            RulesOut ro;
            ro.counts = c->d_rcounts;
            ro.n_records = c->d_count;
            ro.rec_cap = tr ? sl.trec_cap : 0;
            ro.h_counts = sl.rdev;
            ro.recs = tr ? c->d_out : nullptr;
            ro.hashes = tr ? c->d_hash : nullptr;
            ro.h_recs = tr ? (sr_record *)sl.tdev : nullptr;
            ro.h_hashes = tr ? (uint64_t *)(sl.tdev + up256(sl.trec_cap * sizeof(sr_record))) : nullptr;
            hipLaunchKernelGGL(rules_out_kernel, dim3((uint32_t)(!tr ? 1 : want < 1024 ? (want ? want : 1) : 1024)),
                               dim3(kRulesBlock), 0, c->stream, ro);
            if (hipGetLastError() != hipSuccess) return -EIO;
        }
    }
    sl.validated = validate;
    if (validate) {   // the stage's counts and the input's record count into the slot's page-locked memory
        if (nbytes == 0) {
            for (int q = 0; q < 5; ++q) sl.vhost[q] = 0;   // the slot is idle: nothing is in flight that writes here
        } else {
            const bool tr = c->trace && !coalesce && !rules;
            ValidateOut vo;
            vo.counts = c->d_vcounts;
            vo.n_records = c->d_count;
            vo.rec_cap = tr ? sl.trec_cap : 0;
            vo.h_counts = sl.vdev;
            vo.recs = tr ? c->d_out : nullptr;
            vo.hashes = tr ? c->d_hash : nullptr;
            vo.h_recs = tr ? (sr_record *)sl.tdev : nullptr;
            vo.h_hashes = tr ? (uint64_t *)(sl.tdev + up256(sl.trec_cap * sizeof(sr_record))) : nullptr;
            hipLaunchKernelGGL(validate_out_kernel, dim3((uint32_t)(!tr ? 1 : want < 1024 ? (want ? want : 1) : 1024)),
                               dim3(kValidBlock), 0, c->stream, vo);
            if (hipGetLastError() != hipSuccess) return -EIO;
        }
    }
    sl.sampled = sample;
    if (sample) {   // the rewritten text, the counts and the input's record count into the slot's page-locked memory
        uint64_t *const hc = (uint64_t *)(sl.shost + up256(sl.stext_cap));
        sl.sseed = c->sample.cfg.seed + seed_add;
        if (nbytes == 0) {
            for (int q = 0; q < 5; ++q) hc[q] = 0;   // the slot is idle: nothing is in flight that writes here
        } else {
            const bool tr = c->trace && !coalesce && !rules && !validate;
            SampleOut so;
            so.text = c->d_in + nbytes;
            so.counts = c->d_scounts;
            so.n_records = c->d_count;
            so.text_cap = arena < sl.stext_cap ? arena : sl.stext_cap;
            so.rec_cap = tr ? sl.trec_cap : 0;
            so.h_text = sl.sdev;
            so.h_counts = (uint64_t *)(sl.sdev + up256(sl.stext_cap));
            so.recs = tr ? c->d_out : nullptr;
            so.hashes = tr ? c->d_hash : nullptr;
            so.h_recs = tr ? (sr_record *)sl.tdev : nullptr;
            so.h_hashes = tr ? (uint64_t *)(sl.tdev + up256(sl.trec_cap * sizeof(sr_record))) : nullptr;
            hipLaunchKernelGGL(sample_out_kernel, dim3((uint32_t)(want < 1024 ? (want ? want : 1) : 1024)),
                               dim3(kSampleBlock), 0, c->stream, so);
            if (hipGetLastError() != hipSuccess) return -EIO;
        }
    }
    sl.payloaded = c->payloads;
    if (c->payloads) {   // the packets' bytes straight into the slot's page-locked memory; the host holds the carries
        const size_t o_off = up256(sl.pay_cap), o_tot = o_off + up256((sl.poff_cap + 1) * sizeof(uint32_t));
        const sr_payload_batch yb{c->d_in, nbytes + arena + (coalesce ? nbytes : 0), c->d_sorted, nbytes ? cap : 0, c->d_packets, pcap < sl.poff_cap ? pcap : sl.poff_cap,
                                  c->d_mcounts, f_out, nullptr, nullptr, sl.pdev, sl.pay_cap,
                                  (uint32_t *)(sl.pdev + o_off), (uint64_t *)(sl.pdev + o_tot)};
        if ((rc = payloads_impl(c, &yb, 1))) return rc;
    }
    sl.logged = 0;
    if (c->logtext) {   // the batch's log text straight into the slot's page-locked memory (log_kernel.hpp)
        const LogLayout l = log_layout(sl.ltext_cap, sl.lmsg_cap);
        const uint32_t *ends = nullptr;
        size_t n_ends = 0;
        if (log_trace && nbytes) {
            if (src) {
                ends = c->d_ends;
                n_ends = src->count;
            } else if (sl.stage_ends) {
                ends = (const uint32_t *)(sl.ldev + l.o_ends);
                n_ends = sl.stage_ends;
            }
        }
        const sr_log_batch lb{c->d_in, nbytes, c->d_out, c->d_count, nbytes ? cap : 0, log_trace && nbytes ? c->d_hash : nullptr,
                              ends, n_ends, c->log_level, sl.ldev + l.o_pfx, {sl.stage_plen[0], sl.stage_plen[1]},
                              c->log_max_msg, sl.ldev, sl.ltext_cap, (uint32_t *)(sl.ldev + l.o_off), sl.ldev + l.o_lv,
                              sl.lmsg_cap, (uint64_t *)(sl.ldev + l.o_tot), (uint64_t *)(sl.ldev + l.o_tot) + 1};
        if ((rc = log_impl(c, &lb))) return rc;
        sl.logged = 1;
        sl.stage_plen[0] = sl.stage_plen[1] = 0;   // staged for one submission
        sl.stage_ends = 0;
    }
    if (c->name_stats && nbytes) {   // the input-order records and the hashes never leave the device
        const sr_stats_batch sb{c->d_in, nbytes, c->d_out, c->d_count, cap, c->d_hash};
        if ((rc = stats_update_impl(c, &sb, 1))) return rc;
    }
    if (hipEventRecord(sl.done, c->stream) != hipSuccess) return -EIO;
    sl.busy = 1;
    if (sample) ++c->sample_subs;
    return 0;
}

static int pack_result(sr_ctx *c, int k, sr_pack_result *res) {
    sr_ctx::Slot &sl = c->slot[k];
    if (!sl.busy) return -EBUSY;
    sl.busy = 0;
    (void)hipSetDevice(c->device);
    if (hipEventSynchronize(sl.done) != hipSuccess) return -EIO;
    const uint64_t np = sl.counts[0], nv = sl.counts[1], nr = sl.counts[2];
    res->sorted = sl.sorted;
    res->packets = sl.packets;
    res->fill = sl.fill;
    res->probed_dead = sl.probed;
    res->n_records = (size_t)(nr < sl.rec_cap ? nr : sl.rec_cap);
    res->n_valid = (size_t)(nv < res->n_records ? nv : res->n_records);
    res->n_packets = (size_t)(np < sl.pk_cap ? np : sl.pk_cap);
    // a slot submission: the device framed what the host sized, unless the datagrams changed in flight
    if (sl.framed && sl.counts[3] != sl.frame_bytes) return -EIO;
    return (nr > sl.rec_cap || np > sl.pk_cap) ? -ENOSPC : 0;
}

int sr_route_pack_trace(sr_ctx *c, int slot, const sr_record **records, const uint64_t **hashes, size_t *n) {
    if (!c || !records || !hashes || !n || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.traced || !sl.thost || !sl.counts) return -EBUSY;
    // the input's records: with the coalescing on counts[2] is the coalesced batch's
    // (and with the name rules on the kept lines')
    const uint64_t nr = (sl.coalesced && sl.chost) ? ((const uint64_t *)(sl.chost + up256(sl.ctext_cap)))[4]
                        : (sl.ruled && sl.rhost)   ? sl.rhost[4]
                        : (sl.validated && sl.vhost) ? sl.vhost[4]
                        : (sl.sampled && sl.shost) ? ((const uint64_t *)(sl.shost + up256(sl.stext_cap)))[4]
                                                   : sl.counts[2];
    *n = (size_t)(nr < sl.trec_cap ? nr : sl.trec_cap);
    *records = (const sr_record *)sl.thost;
    *hashes = (const uint64_t *)(sl.thost + up256(sl.trec_cap * sizeof(sr_record)));
    return 0;
}

int sr_route_pack_payloads(sr_ctx *c, int slot, const uint8_t **payload, const uint32_t **offsets, size_t *n) {
    if (!c || !payload || !offsets || !n || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.payloaded || !sl.phost || !sl.counts) return -EBUSY;
    const uint64_t np = sl.counts[0];
    const size_t room = sl.pk_cap < sl.poff_cap ? sl.pk_cap : sl.poff_cap;
    *n = (size_t)(np < room ? np : room);
    *payload = sl.phost;
    *offsets = (const uint32_t *)(sl.phost + up256(sl.pay_cap));
    return 0;
}

int sr_set_logtext(sr_ctx *c, int min_level_or_off, size_t text_cap, uint32_t max_msg) {
    if (!c || min_level_or_off > 3) return -EINVAL;
    for (int k = 0; k < 3; ++k)
        if (c->slot[k].busy) return -EBUSY;
    if (min_level_or_off < 0) {
        c->logtext = 0;
        return 0;
    }
    if (c->ds.max_batch > kLogMaxBatch) return -EINVAL;
    const size_t cap = text_cap ? text_cap : (size_t)SR_LOG_DEFAULT_TEXT_CAP(c->ds.max_batch);
    // a message is at least its header (24 bytes or more) or max_msg bytes, and its '\n': a text that fits
    // the arena has no more messages than this, so its index fits too
    const size_t least = (max_msg && max_msg < 24u ? max_msg : 24u) + 1u;
    const uint64_t most = SR_LOG_MAX_MSGS(c->ds.max_batch, SR_MAX_SLOTS);
    const uint64_t msgs = (uint64_t)cap / least + 1u;
    c->logtext = 1;
    c->log_level = min_level_or_off;
    c->log_cap = cap;
    c->log_msgs = (size_t)(msgs < most ? msgs : most);
    c->log_max_msg = max_msg;
    return 0;
}

int sr_route_pack_set_prefix(sr_ctx *c, int slot, const uint8_t *trace, size_t tlen, const uint8_t *warn, size_t wlen) {
    if (!c || slot < 0 || slot > 2 || !c->logtext) return -EINVAL;
    if (tlen > kLogMaxPrefix || wlen > kLogMaxPrefix || (tlen && !trace) || (wlen && !warn)) return -EINVAL;
    sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy) return -EBUSY;
    (void)hipSetDevice(c->device);
    int rc = slot_log_reserve(c, slot);
    if (rc) return rc;
    uint8_t *const p = sl.lhost + log_layout(sl.ltext_cap, sl.lmsg_cap).o_pfx;
    if (tlen) memcpy(p, trace, tlen);
    if (wlen) memcpy(p + tlen, warn, wlen);
    sl.stage_plen[0] = (uint32_t)tlen;
    sl.stage_plen[1] = (uint32_t)wlen;
    return 0;
}

int sr_route_pack_set_ends(sr_ctx *c, int slot, const uint32_t *ends, size_t n) {
    if (!c || slot < 0 || slot > 2 || !c->logtext || n > SR_MAX_SLOTS || (n && !ends)) return -EINVAL;
    sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy) return -EBUSY;
    (void)hipSetDevice(c->device);
    int rc = slot_log_reserve(c, slot);
    if (rc) return rc;
    if (n) memcpy(sl.lhost + log_layout(sl.ltext_cap, sl.lmsg_cap).o_ends, ends, n * sizeof(uint32_t));
    sl.stage_ends = n;
    return 0;
}

int sr_route_pack_logtext(sr_ctx *c, int slot, const uint8_t **text, uint64_t *total, const uint32_t **offsets,
                          const uint8_t **levels, size_t *n_msgs) {
    if (!c || !text || !total || !offsets || !levels || !n_msgs || slot < 0 || slot > 2) return -EINVAL;
    const sr_ctx::Slot &sl = c->slot[slot];
    if (sl.busy || !sl.logged || !sl.lhost) return -EBUSY;
    const LogLayout l = log_layout(sl.ltext_cap, sl.lmsg_cap);
    const uint64_t *tot = (const uint64_t *)(sl.lhost + l.o_tot);
    *text = sl.lhost;
    *total = tot[0];
    *offsets = (const uint32_t *)(sl.lhost + l.o_off);
    *levels = sl.lhost + l.o_lv;
    *n_msgs = (size_t)(tot[1] < sl.lmsg_cap ? tot[1] : sl.lmsg_cap);
    return (tot[0] > sl.ltext_cap || tot[1] > sl.lmsg_cap) ? -ENOSPC : 0;
}

int sr_route_pack_submit(sr_ctx *c, int slot, const uint8_t *bytes, size_t nbytes, const uint16_t *fill) {
    if (!c || slot < 0 || slot > 1) return -EINVAL;
    return pack_submit(c, slot, bytes, nbytes, fill);
}

int sr_route_pack_submit_slots(sr_ctx *c, int slot, const uint8_t *slots, size_t stride, const uint16_t *lens,
                               size_t count, const uint16_t *fill) {
    if (!c || slot < 0 || slot > 1) return -EINVAL;
    if (stride < SR_DATA_BUF_SIZE || stride > kFrameMaxStride || count > SR_MAX_SLOTS) return -EINVAL;
    if (count && (!slots || !lens)) return -EINVAL;
    if (c->slot[slot].busy) return -EBUSY;
    const size_t nbytes = frame_slots_size(slots, stride, lens, count, nullptr);
    if (nbytes > c->ds.max_batch) return -EINVAL;
    if (nbytes == 0) return pack_submit(c, slot, nullptr, 0, fill);
    (void)hipSetDevice(c->device);
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, (void *)slots, 0) != hipSuccess || !d) {   // not page-locked: no guess
        (void)hipGetLastError();
        return -EINVAL;
    }
    const SlotSource src{(const uint8_t *)d, stride, lens, count};
    return pack_submit(c, slot, nullptr, nbytes, fill, &src);
}

int sr_route_pack_result(sr_ctx *c, int slot, sr_pack_result *res) {
    if (!c || !res || slot < 0 || slot > 1) return -EINVAL;
    return pack_result(c, slot, res);
}

int sr_route_pack_batch(sr_ctx *c, const uint8_t *bytes, size_t nbytes, uint16_t *fill, sr_record *sorted,
                        size_t max_records, size_t *n_records, size_t *n_valid, sr_packet *packets,
                        size_t max_packets, size_t *n_packets, uint64_t *probed_dead) {
    if (!c || !n_records || !n_valid || !n_packets || (nbytes && !bytes) || nbytes > c->ds.max_batch) return -EINVAL;
    if ((c->ds.nds && !fill) || (max_records && !sorted) || (max_packets && !packets)) return -EINVAL;
    if (c->ds.nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    *n_records = *n_valid = *n_packets = 0;
    const uint32_t nw = c->ds.nwords;
    if (nbytes == 0) {
        if (probed_dead && nw) memset(probed_dead, 0, nw * sizeof(uint64_t));
        return 0;
    }
    int rc = pack_submit(c, 2, bytes, nbytes, fill);
    if (rc) return rc;
    sr_pack_result r;
    rc = pack_result(c, 2, &r);
    if (rc && rc != -ENOSPC) return rc;
    const size_t cr = r.n_records < max_records ? r.n_records : max_records;
    const size_t cp = r.n_packets < max_packets ? r.n_packets : max_packets;
    if (cr) memcpy(sorted, r.sorted, cr * sizeof(sr_record));
    if (cp) memcpy(packets, r.packets, cp * sizeof(sr_packet));
    if (c->ds.nds) memcpy(fill, r.fill, c->ds.nds * sizeof(uint16_t));
    if (probed_dead && nw) memcpy(probed_dead, r.probed_dead, nw * sizeof(uint64_t));
    *n_records = r.n_records;
    *n_valid = r.n_valid;
    *n_packets = r.n_packets;
    return (rc || r.n_records > max_records || r.n_packets > max_packets) ? -ENOSPC : 0;
}

int sr_route_batch(sr_ctx *c, const uint8_t *bytes, size_t nbytes, sr_record *out, size_t max_records,
                   size_t *n_records, uint64_t *hashes) {
    if (!c || !n_records || (nbytes && !bytes) || nbytes > c->ds.max_batch) return -EINVAL;
    if (max_records && !out) return -EINVAL;
    *n_records = 0;
    if (nbytes == 0) {
        if (c->ds.nwords) memset(c->h_probed, 0, c->ds.nwords * sizeof(uint64_t));
        return 0;
    }
    if (bytes[nbytes - 1] != '\n') return -EINVAL;
    // every shard alive: nothing can be probed dead (the device bitmap is skipped)
    if (c->ds.nwords) memset(c->h_probed, 0, c->ds.nwords * sizeof(uint64_t));
    (void)hipSetDevice(c->device);
    // device record capacity: never more lines than bytes
    const size_t cap = max_records < nbytes ? max_records : nbytes;
    if (cap > c->d_out_cap) {
        (void)hipFree(c->d_out);
        c->d_out = nullptr;
        c->d_out_cap = 0;
        if (hipMalloc(&c->d_out, cap * sizeof(sr_record)) != hipSuccess) return -ENOMEM;
        c->d_out_cap = cap;
    }
    // hashes: asked for, or for the probed-dead replay (probed_dead_kernel; over 1024 shards)
    const bool want_hash = hashes || c->ds.replay_wants_hashes();
    if (want_hash && cap > c->d_hash_cap) {
        (void)hipFree(c->d_hash);
        c->d_hash = nullptr;
        c->d_hash_cap = 0;
        if (hipMalloc(&c->d_hash, cap * sizeof(uint64_t)) != hipSuccess) return -ENOMEM;
        c->d_hash_cap = cap;
    }
    if (hipMemcpyAsync(c->d_in, bytes, nbytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return -EIO;
    RouteParams p = c->ds.params();
    DeviceState::add_batch(p, c->d_in, nbytes, c->d_out, cap, want_hash ? c->d_hash : nullptr, c->d_count, c->d_probed);
    int rc = launch_variant(c->ds, p, c->stream);
    if (rc) return rc;
    if (c->ds.dead && c->ds.nwords &&
        hipMemcpyAsync(c->h_probed, c->d_probed, c->ds.nwords * sizeof(uint64_t), hipMemcpyDeviceToHost,
                       c->stream) != hipSuccess)
        return -EIO;
    uint64_t n = 0;
    if (hipMemcpyAsync(&n, c->d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return -EIO;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -EIO;
    const size_t ncopy = n < cap ? (size_t)n : cap;
    if (ncopy) {
        if (hipMemcpyAsync(out, c->d_out, ncopy * sizeof(sr_record), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return -EIO;
        if (hashes &&
            hipMemcpyAsync(hashes, c->d_hash, ncopy * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return -EIO;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return -EIO;
    }
    *n_records = (size_t)n;
    return n > max_records ? -ENOSPC : 0;
}

}  // extern "C"

// ---- multi-GPU exchange (exchange.hpp, local_comm.hpp) -------------------------------------------
// A communicator is a small table of collectives behind one handle: the RCCL entry points are one
// instance (sr_comm_open), the in-process board the other (sr_comm_open_local). Everything above the
// table (the sizes publish and spin, exchange_run, regroup_run, exchange_dead_rows, the own-chunk-in-
// place test) is one code path for both.
struct CommBackend {
    int (*all_to_all)(sr_comm *c, const uint64_t *send, uint64_t *recv, size_t count, hipStream_t stream);
    int (*send)(sr_comm *c, const void *buf, size_t bytes, int peer, int tag, hipStream_t stream);
    int (*recv)(sr_comm *c, void *buf, size_t bytes, int peer, int tag, hipStream_t stream);
    int (*group_start)(sr_comm *c, hipStream_t stream);
    int (*group_end)(sr_comm *c, hipStream_t stream);
    void (*close)(sr_comm *c);
};

// what the communicator's sr_transport callbacks get (sr_comm_transport: owned by the comm)
struct CommTransport {
    sr_comm *comm;
    hipStream_t stream;
    sr_ctx *ctx;
};

struct sr_comm_group : LocalGroup {
    using LocalGroup::LocalGroup;
};

struct sr_comm {
    const CommBackend *be = nullptr;
    RcclApi *r = nullptr;   // RCCL backend
    void *nccl = nullptr;
    LocalComm local;        // in-process backend
    int world = 0, rank = 0, device = 0;
    uint64_t *h_sizes = nullptr;   // pinned, mapped, coherent: [2][world][2] sent, received, then the sequence word
    uint64_t *d_sizes = nullptr;   // its device address (nullptr: copies and a stream synchronisation instead)
    uint64_t seq = 0;
    uint32_t timeout_ms = 0;       // sr_comm_set_timeout: 0 = no deadline
    int broken = 0;                // a deadline ran out on this comm
    CommTransport tuser{};         // sr_comm_transport's `user`
};

// -EPIPE once a deadline ran out on the comm or its group broke
static int comm_usable(sr_comm *c) {
    if (c->broken || (c->local.group && c->local.group->board.broken())) return -EPIPE;
    return 0;
}
static void comm_break(sr_comm *c) {
    c->broken = 1;
    if (c->local.group) c->local.group->board.break_all();
}

// RCCL
static int rccl_be_all_to_all(sr_comm *c, const uint64_t *send, uint64_t *recv, size_t count, hipStream_t s) {
    return c->r->all_to_all(send, recv, count, kNcclUint64, c->nccl, s) == 0 ? 0 : -EIO;
}
static int rccl_be_send(sr_comm *c, const void *buf, size_t bytes, int peer, int, hipStream_t s) {
    return c->r->send(buf, bytes, kNcclUint8, peer, c->nccl, s) == 0 ? 0 : -EIO;
}
static int rccl_be_recv(sr_comm *c, void *buf, size_t bytes, int peer, int, hipStream_t s) {
    return c->r->recv(buf, bytes, kNcclUint8, peer, c->nccl, s) == 0 ? 0 : -EIO;
}
static int rccl_be_group_start(sr_comm *c, hipStream_t) { return c->r->group_start() == 0 ? 0 : -EIO; }
static int rccl_be_group_end(sr_comm *c, hipStream_t) { return c->r->group_end() == 0 ? 0 : -EIO; }
static void rccl_be_close(sr_comm *c) {
    if (c->nccl) (void)c->r->comm_destroy(c->nccl);
}
static const CommBackend kRcclBackend{rccl_be_all_to_all, rccl_be_send,      rccl_be_recv,
                                      rccl_be_group_start, rccl_be_group_end, rccl_be_close};

// In process: the operations of a group are collected and run on the board at group_end, on the calling
// rank's thread and stream (local_board.hpp: run_group).
static int local_be_run(sr_comm *c, const BoardSeg *own, size_t n_own, hipStream_t s) {
    LocalDev dev{&c->local, s};
    const int rc = c->local.group->board.run_group(c->rank, c->local.ops, own, n_own, dev, c->timeout_ms);
    c->local.ops.clear();
    if (rc == -ETIMEDOUT) c->broken = 1;
    return rc;
}
static int local_be_group_start(sr_comm *c, hipStream_t s) {
    if (c->local.in_group) return -EINVAL;
    int rc = comm_usable(c);
    if (!rc) rc = local_stream_ok(s);
    if (rc) return rc;
    c->local.ops.clear();
    c->local.in_group = true;
    return 0;
}
static int local_be_post(sr_comm *c, bool is_send, void *buf, size_t bytes, int peer, int tag) {
    if (!c->local.in_group || !buf || peer < 0 || peer >= c->world || peer == c->rank || tag < 0 ||
        tag >= kBoardA2ATag)
        return -EINVAL;
    if (bytes) c->local.ops.push_back(BoardOp{is_send, peer, tag, buf, bytes});
    return 0;
}
static int local_be_send(sr_comm *c, const void *buf, size_t bytes, int peer, int tag, hipStream_t) {
    return local_be_post(c, true, const_cast<void *>(buf), bytes, peer, tag);
}
static int local_be_recv(sr_comm *c, void *buf, size_t bytes, int peer, int tag, hipStream_t) {
    return local_be_post(c, false, buf, bytes, peer, tag);
}
static int local_be_group_end(sr_comm *c, hipStream_t s) {
    if (!c->local.in_group) return -EINVAL;
    c->local.in_group = false;
    return local_be_run(c, nullptr, 0, s);
}
// count elements per peer: world - 1 sends, world - 1 receives, the own element one more segment of the pull
static int local_be_all_to_all(sr_comm *c, const uint64_t *send, uint64_t *recv, size_t count, hipStream_t s) {
    if (c->local.in_group || !send || !recv || !count) return -EINVAL;
    int rc = comm_usable(c);
    if (!rc) rc = local_stream_ok(s);
    if (rc) return rc;
    const size_t bytes = count * sizeof(uint64_t);
    c->local.ops.clear();
    for (int q = 0; q < c->world; ++q) {
        if (q == c->rank) continue;
        c->local.ops.push_back(BoardOp{true, q, kBoardA2ATag, const_cast<uint64_t *>(send) + (size_t)q * count, bytes});
        c->local.ops.push_back(BoardOp{false, q, kBoardA2ATag, recv + (size_t)q * count, bytes});
    }
    const BoardSeg own{send + (size_t)c->rank * count, recv + (size_t)c->rank * count, bytes};
    return local_be_run(c, &own, 1, s);
}
static void local_be_close(sr_comm *c) {
    local_events_retire(c->local);
    c->local.group->board.release_rank(c->rank);
}
static const CommBackend kLocalBackend{local_be_all_to_all, local_be_send,      local_be_recv,
                                       local_be_group_start, local_be_group_end, local_be_close};

// the sizes' page-locked landing place (both backends)
static int comm_sizes_alloc(sr_comm *c) {
    if (hipHostMalloc((void **)&c->h_sizes, (4 * (size_t)c->world + 1) * sizeof(uint64_t),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return -ENOMEM;
    memset(c->h_sizes, 0, (4 * (size_t)c->world + 1) * sizeof(uint64_t));
    if (hipHostGetDevicePointer((void **)&c->d_sizes, c->h_sizes, 0) != hipSuccess) c->d_sizes = nullptr;
    return 0;
}

extern "C" {

int sr_comm_id(uint8_t id[SR_COMM_ID_BYTES]) {
    RcclApi *r = rccl_api();
    if (!id) return -EINVAL;
    if (!r) return -ENOSYS;
    return r->get_unique_id(id) == 0 ? 0 : -EIO;
}

int sr_comm_open(sr_comm **out, const uint8_t id[SR_COMM_ID_BYTES], int world, int rank, int device) {
    if (!out || !id || world < 1 || world > (int)kMaxOwners || rank < 0 || rank >= world) return -EINVAL;
    *out = nullptr;
    RcclApi *r = rccl_api();
    if (!r) return -ENOSYS;
    if (hipSetDevice(device) != hipSuccess) return -ENODEV;
    sr_comm *c = new (std::nothrow) sr_comm;
    if (!c) return -ENOMEM;
    c->be = &kRcclBackend, c->r = r, c->world = world, c->rank = rank, c->device = device;
    if (comm_sizes_alloc(c)) {
        delete c;
        return -ENOMEM;
    }
    CommId cid;
    memcpy(cid.b, id, sizeof(cid.b));
    if (((InitRankFn)r->comm_init_rank)(&c->nccl, world, cid, rank) != 0) {
        (void)hipHostFree(c->h_sizes);
        delete c;
        return -EIO;
    }
    *out = c;
    return 0;
}

int sr_comm_group_open(sr_comm_group **g, int world) {
    if (!g) return -EINVAL;
    *g = nullptr;
    if (world < 1 || world > (int)kMaxOwners) return -EINVAL;
    *g = new (std::nothrow) sr_comm_group(world);
    return *g ? 0 : -ENOMEM;
}

int sr_comm_group_close(sr_comm_group *g) {
    if (!g) return -EINVAL;
    if (g->board.open_ranks() > 0) return -EBUSY;
    for (hipEvent_t e : g->retired) (void)hipEventDestroy(e);
    delete g;
    return 0;
}

int sr_comm_open_local(sr_comm **out, sr_comm_group *g, int rank, int device) {
    if (!out) return -EINVAL;
    *out = nullptr;
    if (!g || rank < 0 || rank >= g->board.world()) return -EINVAL;
    if (device < 0 || hipSetDevice(device) != hipSuccess) return -ENODEV;
    sr_comm *c = new (std::nothrow) sr_comm;
    if (!c) return -ENOMEM;
    c->be = &kLocalBackend, c->world = g->board.world(), c->rank = rank, c->device = device;
    int rc = g->board.take_rank(rank, device);
    if (rc) {
        delete c;
        return rc;
    }
    // Ranks on another device: the pull reads the peer's memory, so access is enabled both ways at open.
    // The slot is taken BEFORE the peers are scanned: of two ranks that open at the same time, the one
    // whose take_rank comes second sees the first (both run under the board's lock), so every pair on
    // two devices is enabled before the later rank's open returns, and no message of a pair moves
    // before both of its ranks are open.
    // (Not run on a one-GPU machine: unverified)
    for (int q = 0; q < g->board.world(); ++q) {
        const int pd = g->board.device_of(q);
        if (q == rank || pd < 0 || pd == device) continue;
        int a = 0, b = 0;
        if (hipDeviceCanAccessPeer(&a, device, pd) != hipSuccess || hipDeviceCanAccessPeer(&b, pd, device) != hipSuccess ||
            !a || !b) {
            (void)hipGetLastError();
            g->board.release_rank(rank);
            delete c;
            return -ENOTSUP;
        }
        (void)hipDeviceEnablePeerAccess(pd, 0);   // (hipErrorPeerAccessAlreadyEnabled is fine)
        (void)hipSetDevice(pd);
        (void)hipDeviceEnablePeerAccess(device, 0);
        (void)hipSetDevice(device);
        (void)hipGetLastError();
    }
    c->local.group = g, c->local.rank = rank;
    if ((rc = local_events_create(c->local)) || (rc = comm_sizes_alloc(c))) {
        local_be_close(c);
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

int sr_comm_set_timeout(sr_comm *c, uint32_t ms) {
    if (!c) return -EINVAL;
    c->timeout_ms = ms;
    return 0;
}

void sr_comm_close(sr_comm *c) {
    if (!c) return;
    (void)hipHostFree(c->h_sizes);
    c->be->close(c);
    delete c;
}

int sr_exchange_sizes(sr_ctx *ctx, sr_comm *comm, const uint64_t *d_owner_counts, uint64_t *d_recv_counts,
                      uint64_t *h_sent, uint64_t *h_received) {
    if (!ctx || !comm || !d_owner_counts || !d_recv_counts || !h_sent || !h_received) return -EINVAL;
    int rc = comm_usable(comm);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    const size_t w2 = 2 * (size_t)comm->world;
    // one deadline for the whole call: the board's waits inside all_to_all start their own `ms` no
    // earlier than this, and what follows them (the spin, or the fallback's drain) ends at this one
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(comm->timeout_ms);
    if (comm->d_sizes) {
        // one rank: nothing to exchange (the received sizes are the sent ones, written by the publish
        // kernel); then the host spins on the sequence word, checking the stream now and then for errors
        // and, with sr_comm_set_timeout, the clock
        if (comm->world > 1 && (rc = comm->be->all_to_all(comm, d_owner_counts, d_recv_counts, 2, ctx->stream)))
            return rc;
        const uint64_t seq = ++comm->seq;
        hipLaunchKernelGGL(sizes_publish_kernel, dim3(1), dim3(256), 0, ctx->stream, d_owner_counts,
                           comm->world > 1 ? d_recv_counts : nullptr, d_recv_counts, comm->d_sizes,
                           (uint32_t)w2, seq);
        if (hipGetLastError() != hipSuccess) return -EIO;
        volatile const uint64_t *hs = comm->h_sizes;
        for (uint32_t k = 1; hs[2 * w2] != seq; ++k) {
            if ((k & 255u) == 0) {
                const hipError_t q = hipStreamQuery(ctx->stream);
                if (q == hipSuccess) {
                    if (hs[2 * w2] == seq) break;
                    return -EIO;
                }
                if (q != hipErrorNotReady) return -EIO;
                if (comm->timeout_ms && std::chrono::steady_clock::now() >= deadline) {
                    comm_break(comm);   // the sizes may still land later: the comm is not used again
                    return -ETIMEDOUT;
                }
            }
            __builtin_ia32_pause();
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        for (size_t i = 0; i < w2; ++i) {
            h_sent[i] = hs[i];
            h_received[i] = hs[w2 + i];
        }
        return 0;
    }
    if ((rc = comm->be->all_to_all(comm, d_owner_counts, d_recv_counts, 2, ctx->stream))) return rc;
    if (hipMemcpyAsync(comm->h_sizes, d_owner_counts, w2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipMemcpyAsync(comm->h_sizes + w2, d_recv_counts, w2 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                       ctx->stream) != hipSuccess)
        return -EIO;
    if (!comm->timeout_ms) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return -EIO;
    } else {   // the same wait under the deadline
        for (hipError_t q; (q = hipStreamQuery(ctx->stream)) != hipSuccess;) {
            if (q != hipErrorNotReady) return -EIO;
            if (std::chrono::steady_clock::now() >= deadline) {
                comm_break(comm);
                return -ETIMEDOUT;
            }
            std::this_thread::yield();
        }
    }
    memcpy(h_sent, comm->h_sizes, w2 * sizeof(uint64_t));
    memcpy(h_received, comm->h_sizes + w2, w2 * sizeof(uint64_t));
    return 0;
}

static int rebase_launch(hipStream_t stream, sr_record *d_recs, const sr_exchange_peer *peers, int world) {
    RebaseArgs a;
    int rc = rebase_args(peers, world, a);
    if (rc) return rc;
    if (a.n_lines > a.first) {   // (one source, or every source before the first that moves: nothing to add)
        hipLaunchKernelGGL(exchange_rebase_kernel, dim3((a.n_lines - a.first + 255u) / 256u), dim3(256), 0, stream, d_recs, a);
        if (hipGetLastError() != hipSuccess) return -EIO;
    }
    return 0;
}

// The communicator as an sr_transport: every call on the backend with the context's stream. Both chunk
// kinds travel as bytes (the record chunk is 8 bytes per line on both sides of a pair).
static int comm_group_start(void *u) {
    CommTransport *t = (CommTransport *)u;
    return t->comm->be->group_start(t->comm, t->stream);
}
static int comm_group_end(void *u) {
    CommTransport *t = (CommTransport *)u;
    return t->comm->be->group_end(t->comm, t->stream);
}
static int comm_send(void *u, const void *buf, size_t bytes, int peer, int tag) {
    CommTransport *t = (CommTransport *)u;
    return t->comm->be->send(t->comm, buf, bytes, peer, tag, t->stream);
}
static int comm_recv(void *u, void *buf, size_t bytes, int peer, int tag) {
    CommTransport *t = (CommTransport *)u;
    return t->comm->be->recv(t->comm, buf, bytes, peer, tag, t->stream);
}
static int comm_copy(void *u, void *dst, const void *src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ((CommTransport *)u)->stream) == hipSuccess
               ? 0 : -EIO;
}
static int comm_rebase(void *u, sr_record *recs, const sr_exchange_peer *peers, int world, uint64_t) {
    return rebase_launch(((CommTransport *)u)->stream, recs, peers, world);
}
static sr_transport comm_transport(CommTransport *user) {
    return sr_transport{user, comm_group_start, comm_group_end, comm_send, comm_recv, comm_copy, comm_rebase};
}

int sr_comm_transport(sr_comm *comm, sr_ctx *ctx, sr_transport *out) {
    if (!comm || !ctx || !out) return -EINVAL;
    comm->tuser = CommTransport{comm, ctx->stream, ctx};
    *out = comm_transport(&comm->tuser);
    return 0;
}

int sr_exchange_data(sr_ctx *ctx, sr_comm *comm, const uint8_t *d_packed, const sr_record *d_packed_recs,
                     const uint64_t *h_sent, const uint64_t *h_received, uint8_t *d_recv_bytes,
                     sr_record *d_recv_recs) {
    if (!ctx || !comm || !h_sent || !h_received) return -EINVAL;
    const int usable = comm_usable(comm);
    if (usable) return usable;
    (void)hipSetDevice(ctx->device);
    CommTransport ct{comm, ctx->stream, ctx};
    const sr_transport t = comm_transport(&ct);
    // the own chunk already in its place (sr_pack_owner_scatter into these receive buffers): no copy
    bool in_place = false;
    if (ctx->own_set && ctx->own == comm->rank) {
        sr_exchange_peer peers[kMaxOwners];
        uint64_t tot[4];
        if (exchange_plan(comm->world, comm->rank, h_sent, h_received, peers, tot) == 0) {
            const sr_exchange_peer &e = peers[comm->rank];
            in_place = ctx->own_bytes == d_recv_bytes + e.recv_byte0 && ctx->own_recs == d_recv_recs + e.recv_line0;
        }
    }
    ctx->own_set = 0;
    return exchange_run(t, comm->world, comm->rank, h_sent, h_received, d_packed, d_packed_recs, d_recv_bytes,
                        d_recv_recs, in_place);
}

// One route launch's regroup on any transport (sr_regroup_run): the split sizes, the size exchange
// (the one host round trip), the plan, the scatter with the rank's own chunk written straight into its
// place in the receive buffers, then the exchange without the own chunk's copy and the rebase.
// sr_regroup_launch is this on a communicator (RCCL or in process): all run this one sequence.
static int regroup_run(sr_ctx *ctx, const sr_transport &t, sr_sizes_fn sizes, int world, int rank,
                       const sr_batch *batches, size_t count, uint64_t *d_owner_counts, uint64_t *d_recv_counts,
                       uint8_t *d_packed, size_t packed_cap, sr_record *d_packed_recs, uint8_t *d_recv_bytes,
                       size_t recv_bytes_cap, sr_record *d_recv_recs, size_t recv_recs_cap, uint64_t *h_sent,
                       uint64_t *h_received) {
    if (!ctx || !sizes || !d_owner_counts || !d_recv_counts || !d_recv_bytes || !d_recv_recs || !h_sent ||
        !h_received || world < 1 || world > (int)kMaxOwners || rank < 0 || rank >= world)
        return -EINVAL;
    int rc = sr_pack_owner_sizes(ctx, batches, count, (uint32_t)world, d_owner_counts);
    if (rc) return rc;
    if ((rc = sizes(t.user, d_owner_counts, d_recv_counts, h_sent, h_received))) return rc;
    sr_exchange_peer peers[kMaxOwners];
    uint64_t tot[4];
    if ((rc = exchange_plan(world, rank, h_sent, h_received, peers, tot))) return rc;
    if (tot[2] > recv_recs_cap || tot[3] > recv_bytes_cap) return -ENOSPC;
    const sr_exchange_peer &e = peers[rank];
    rc = sr_pack_owner_scatter(ctx, batches, count, (uint32_t)world, rank, d_recv_bytes + e.recv_byte0,
                               d_recv_recs + e.recv_line0, d_packed, packed_cap, d_packed_recs);
    ctx->own_set = 0;   // consumed here: the exchange below is told the own chunk is in place
    if (rc) return rc;
    return exchange_run(t, world, rank, h_sent, h_received, d_packed, d_packed_recs, d_recv_bytes, d_recv_recs,
                        true);
}

static int comm_sizes(void *u, const uint64_t *d_owner_counts, uint64_t *d_recv_counts, uint64_t *h_sent,
                      uint64_t *h_received) {
    CommTransport *t = (CommTransport *)u;
    return sr_exchange_sizes(t->ctx, t->comm, d_owner_counts, d_recv_counts, h_sent, h_received);
}

int sr_regroup_launch(sr_ctx *ctx, sr_comm *comm, const sr_batch *batches, size_t count,
                      uint64_t *d_owner_counts, uint64_t *d_recv_counts, uint8_t *d_packed, size_t packed_cap,
                      sr_record *d_packed_recs, uint8_t *d_recv_bytes, size_t recv_bytes_cap,
                      sr_record *d_recv_recs, size_t recv_recs_cap, uint64_t *h_sent, uint64_t *h_received) {
    if (!ctx || !comm) return -EINVAL;
    const int usable = comm_usable(comm);
    if (usable) return usable;
    (void)hipSetDevice(ctx->device);
    CommTransport ct{comm, ctx->stream, ctx};
    const sr_transport t = comm_transport(&ct);
    return regroup_run(ctx, t, comm_sizes, comm->world, comm->rank, batches, count, d_owner_counts, d_recv_counts,
                       d_packed, packed_cap, d_packed_recs, d_recv_bytes, recv_bytes_cap, d_recv_recs, recv_recs_cap,
                       h_sent, h_received);
}

int sr_regroup_run(sr_ctx *ctx, const sr_transport *t, sr_sizes_fn sizes, int world, int rank,
                   const sr_batch *batches, size_t count, uint64_t *d_owner_counts, uint64_t *d_recv_counts,
                   uint8_t *d_packed, size_t packed_cap, sr_record *d_packed_recs, uint8_t *d_recv_bytes,
                   size_t recv_bytes_cap, sr_record *d_recv_recs, size_t recv_recs_cap, uint64_t *h_sent,
                   uint64_t *h_received) {
    if (!ctx || !t) return -EINVAL;
    (void)hipSetDevice(ctx->device);
    return regroup_run(ctx, *t, sizes, world, rank, batches, count, d_owner_counts, d_recv_counts, d_packed,
                       packed_cap, d_packed_recs, d_recv_bytes, recv_bytes_cap, d_recv_recs, recv_recs_cap, h_sent,
                       h_received);
}

int sr_exchange_plan(int world, int rank, const uint64_t *h_sent, const uint64_t *h_received,
                     sr_exchange_peer *peers, uint64_t *totals) {
    uint64_t tot[4];
    const int rc = exchange_plan(world, rank, h_sent, h_received, peers, tot);
    if (!rc && totals) memcpy(totals, tot, sizeof(tot));
    return rc;
}

int sr_exchange_run(const sr_transport *t, int world, int rank, const uint64_t *h_sent, const uint64_t *h_received,
                    const uint8_t *packed, const sr_record *packed_recs, uint8_t *recv_bytes, sr_record *recv_recs) {
    if (!t) return -EINVAL;
    return exchange_run(*t, world, rank, h_sent, h_received, packed, packed_recs, recv_bytes, recv_recs);
}

int sr_exchange_rebase(sr_ctx *ctx, sr_record *d_recv_recs, const sr_exchange_peer *peers, int world) {
    if (!ctx || !peers) return -EINVAL;
    RebaseArgs a;
    int rc = rebase_args(peers, world, a);
    if (rc) return rc;
    if (a.n_lines && !d_recv_recs) return -EINVAL;
    (void)hipSetDevice(ctx->device);
    return rebase_launch(ctx->stream, d_recv_recs, peers, world);
}

// ---- owner side (owner_kernel.hpp) -----------------------------------------------------------------
static uint32_t dead_words(const sr_ctx *c) { return c->ds.nds ? (c->ds.nds + 63u) / 64u : 1u; }

// The launch's bitmaps ORed into row `rank` (one kernel), then the rows over the transport.
static int exchange_dead_impl(sr_ctx *ctx, const sr_transport &t, int world, int rank, const sr_batch *batches,
                              size_t count, uint64_t *d_all_dead) {
    DeadOrArgs a;
    memset(&a, 0, sizeof(a));
    for (size_t j = 0; j < count; ++j) a.pd[j] = batches[j].d_probed_dead;
    a.count = (uint32_t)count;
    a.nwords = dead_words(ctx);
    a.row = d_all_dead + (size_t)rank * a.nwords;
    (void)hipSetDevice(ctx->device);
    hipLaunchKernelGGL(owner_dead_or_kernel, dim3((a.nwords + 63u) / 64u), dim3(64), 0, ctx->stream, a);
    if (hipGetLastError() != hipSuccess) return -EIO;
    return exchange_dead_rows(t, world, rank, d_all_dead, a.nwords);
}

static bool exchange_dead_args_ok(const sr_ctx *ctx, int world, int rank, const sr_batch *batches, size_t count,
                                  const uint64_t *d_all_dead) {
    return ctx && d_all_dead && world >= 1 && world <= (int)kMaxOwners && rank >= 0 && rank < world &&
           count <= SR_MAX_BATCHES_PER_LAUNCH && (count == 0 || batches);
}

int sr_exchange_dead_run(sr_ctx *ctx, const sr_transport *t, int world, int rank, const sr_batch *batches,
                         size_t count, uint64_t *d_all_dead) {
    if (!t || !exchange_dead_args_ok(ctx, world, rank, batches, count, d_all_dead)) return -EINVAL;
    if (world > 1 && (!t->group_start || !t->group_end || !t->send || !t->recv)) return -EINVAL;
    return exchange_dead_impl(ctx, *t, world, rank, batches, count, d_all_dead);
}

int sr_exchange_dead(sr_ctx *ctx, sr_comm *comm, const sr_batch *batches, size_t count, uint64_t *d_all_dead) {
    if (!comm || !exchange_dead_args_ok(ctx, comm->world, comm->rank, batches, count, d_all_dead)) return -EINVAL;
    const int usable = comm_usable(comm);
    if (usable) return usable;
    CommTransport ct{comm, ctx->stream, ctx};
    const sr_transport t = comm_transport(&ct);
    return exchange_dead_impl(ctx, t, comm->world, comm->rank, batches, count, d_all_dead);
}

// The fold, then the packing and the gather as sr_pack_packets / sr_pack_payloads run them: every argument
// is checked before the first launch, so that -EINVAL leaves nothing enqueued.
int sr_owner_pack(sr_ctx *c, const sr_owner_batch *b) {
    if (!c || !b || !b->d_recv_counts || b->world < 1 || b->world > (int)kMaxOwners) return -EINVAL;
    const uint32_t nds = c->ds.nds;
    if (nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    if (!b->d_counts || (nds && !b->d_fill_out) || b->max_records > 0xFFFFFFF0ull) return -EINVAL;
    if (b->max_records && (!b->d_recv_recs || !b->d_sorted)) return -EINVAL;
    if (b->max_packets && !b->d_packets) return -EINVAL;
    if (b->d_payload) {   // sr_pack_payloads' rules
        if (!b->d_offsets || !b->d_total) return -EINVAL;
        if ((b->recv_nbytes && !b->d_recv_bytes) || b->recv_nbytes > 0xFFFFFFF0ull) return -EINVAL;
        if (b->d_pend_out && (!b->d_pend_in || b->d_pend_out == b->d_pend_in)) return -EINVAL;
    }
    (void)hipSetDevice(c->device);
    if (!c->d_owner_n && hipMalloc(&c->d_owner_n, sizeof(uint64_t)) != hipSuccess) return -ENOMEM;
    if (!c->d_owner_fill && hipMalloc(&c->d_owner_fill, (nds ? nds : 1) * sizeof(uint16_t)) != hipSuccess)
        return -ENOMEM;
    const OwnerFoldArgs f{b->d_recv_counts, b->d_all_dead, b->d_fill_in, c->d_owner_n, c->d_owner_fill,
                          (uint32_t)b->world, nds, dead_words(c)};
    hipLaunchKernelGGL(owner_fold_kernel, dim3(1), dim3(kOwnerBlock), 0, c->stream, f);
    if (hipGetLastError() != hipSuccess) return -EIO;
    const sr_pack_batch pb{b->d_recv_recs, c->d_owner_n, b->max_records, c->d_owner_fill, nullptr,
                           b->d_sorted, b->d_packets, b->max_packets, b->d_counts, b->d_fill_out};
    int rc = pack_many_impl(c, &pb, 1, nullptr, nullptr);
    if (rc || !b->d_payload) return rc;
    const sr_payload_batch yb{b->d_recv_bytes, b->recv_nbytes, b->d_sorted, b->max_records, b->d_packets,
                              b->max_packets, b->d_counts, b->d_fill_out, b->d_pend_in, b->d_pend_out,
                              b->d_payload, b->payload_cap, b->d_offsets, b->d_total};
    return payloads_impl(c, &yb, 1);
}

int sr_flush_pending(sr_ctx *c, uint16_t *d_fill, const uint8_t *d_pend, sr_packet *d_packets, size_t max_packets,
                     uint64_t *d_counts, uint8_t *d_payload, size_t payload_cap, uint32_t *d_offsets,
                     uint64_t *d_total) {
    if (!c || !d_counts || !d_offsets || !d_total) return -EINVAL;
    const uint32_t nds = c->ds.nds;
    if (nds > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    if ((nds && (!d_fill || !d_pend)) || (max_packets && !d_packets) || (payload_cap && !d_payload)) return -EINVAL;
    const uint32_t room = (uint32_t)(max_packets < nds ? max_packets : nds);   // never more descriptors than slots
    const FlushArgs a{d_fill, d_pend, d_packets, d_counts, d_payload, d_offsets, d_total, payload_cap, nds, room};
    (void)hipSetDevice(c->device);
    hipLaunchKernelGGL(flush_scan_kernel, dim3(1), dim3(kOwnerBlock), 0, c->stream, a);
    if (room)
        hipLaunchKernelGGL(flush_copy_kernel, dim3((room + kPayWaves - 1) / kPayWaves), dim3(kPayBlock), 0,
                           c->stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // extern "C"
