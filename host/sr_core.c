/*
 * sr_core.c — one data thread of the MI355X statsd-router (include/sr_router.h).
 *
 * Per batch of framed datagrams the GPU does the per-line work and the per-downstream packing
 * (sr_route_pack_batch: tokenise, length / ':' verdict, sdbm hash, shard pick, greedy 1450-byte
 * packets); this file keeps the reference's host-side state and side effects:
 *   - the pending (active) buffer of every downstream and its traffic / packet counters
 *     (downstream_s, sr-types.h:36-63);
 *   - the flush of a packet: counters, then the bytes to the emit callback (ds_schedule_flush,
 *     sr-main.c:49-71; the send itself, ds_flush_cb :21-46, is the caller's);
 *   - the drop of a probed dead downstream's pending buffer (find_downstream, sr-main.c:106);
 *   - the WARN lines with the reference's texts (sr-main.c:115,142,184) and, at log_level 0, the
 *     TRACE lines (sr-main.c:91,102,174) in input order, from the GPU's per-line hashes;
 *   - the flush timer (ds_flush_timer_cb, :194-204) and the self-metrics (ping_cb, :206-235), whose
 *     few lines are routed on the GPU too and appended here with push_to_downstream's rule (:73-83).
 * There is no CPU routing path: the shard of every line, data or ping, comes from the GPU.
 */
#include "../include/sr_router.h"
#include "sr_slots.h"

#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct ds_state {
    uint8_t pending[SR_DOWNSTREAM_BUF_SIZE]; /* active buffer (sr-types.h:40-41) */
    uint32_t fill;                           /* active_buffer_length            */
    int32_t traffic, packets;                /* sr-types.h:52,54                */
    char conn_metric[SR_METRIC_SIZE];        /* per_downstream_counter_metric   */
    int conn_len;
    char traffic_metric[SR_METRIC_SIZE];
    char packet_metric[SR_METRIC_SIZE];
} ds_state;

struct sr_core {
    sr_ctx *ctx;
    uint32_t n, nwords;
    int log_level;
    ds_state *ds;
    uint64_t *alive;
    char alive_metric[SR_METRIC_SIZE];
    sr_core_emit_fn emit;
    sr_core_log_fn log;
    sr_core_flush_fn flush;
    void *user;
    /* per-batch buffers (page-locked) */
    size_t max_batch;
    uint8_t *in[2];                          /* the two slots' framed datagrams                 */
    const uint8_t *in_flight_bytes;          /* the framed bytes of the batch in flight          */
    size_t in_flight_len;
    int in_flight;                           /* slot whose batch is on the GPU, or -1            */
    unsigned fail_submit, submits;           /* fault injection (sr_core_inject_faults, tests)   */
    unsigned fail_finish, finishes;
    int trace;                               /* log_level TRACE: per-line hashes from the GPU     */
    uint32_t *dg_ends[2];                    /* TRACE: datagram ends of the batch in each slot    */
    size_t dg_n[2], dg_cap[2];
    /* sr_core_submit_slots: the batch in a slot is datagrams left in 4096-byte slots of its buffer */
    uint16_t *slot_lens[2];                  /* their lengths as received                          */
    uint32_t *slot_ends[2];                  /* framed end offset after each (sr_slots.h)          */
    size_t slot_n[2];                        /* slots of the batch; 0: the buffer holds framed bytes */
    uint64_t *ping_hash;                     /* TRACE: the ping names' hashes                      */
    int payloads;                            /* sr_core_set_payloads: packets from the slot's arena */
    int devlog;                              /* sr_core_set_device_log: batches' log text from the GPU */
    sr_core_log_prefix_fn log_prefix;        /* block mode: the prefixes, asked at submission      */
    sr_core_log_block_fn log_block;          /* block mode: a batch's whole text in one call       */
    int log_host[2];                         /* the slot's batch could not be staged: the host formats it */
    uint64_t log_device_n, log_host_n;       /* sr_core_device_log_stats                            */
    int coalesce;                            /* sr_core_set_coalesce: plain counters coalesced on the GPU */
    const uint8_t *co_text[2];               /* the merged text of the batch being completed in a slot ... */
    size_t co_base[2];                       /* ... which holds the framed bytes from this offset on       */
    uint64_t co_totals[4];                   /* sr_core_coalesce_counts                                     */
    int sample;                              /* sr_core_set_sample: hot names thinned on the GPU            */
    const uint8_t *sa_text[2];               /* the rewritten lines of the batch being completed in a slot ... */
    size_t sa_base[2];                       /* ... which holds the framed bytes from this offset on        */
    int host_fills;                          /* the host changed pending buffers since the last  */
                                             /* submission: upload them with the next one         */
    uint16_t *fill16;
    sr_record *sorted;                       /* the ping names' records (sr_route_batch)         */
    size_t sorted_cap;
    uint64_t *probed;
    struct iovec *iov;
    char *msg;
    size_t msg_cap;
    uint8_t *ping;                           /* the ping names routed by sr_core_ping */
    size_t ping_cap;
};

static void core_log(sr_core *c, int level, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static void core_log(sr_core *c, int level, const char *fmt, ...) {
    if (level < c->log_level || !c->log) return;
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(c->msg, c->msg_cap, fmt, ap);
    va_end(ap);
    if (n < 0) return;
    if ((size_t)n >= c->msg_cap) n = (int)c->msg_cap - 1;
    c->log(c->user, level, c->msg, (size_t)n);
}

/* ds_schedule_flush (sr-main.c:49-71): count the packet, hand the pending buffer over, start a new one */
static void schedule_flush(sr_core *c, uint32_t s) {
    ds_state *d = &c->ds[s];
    d->packets += 1;                                               /* :61 */
    d->traffic = (int32_t)((uint32_t)d->traffic + d->fill);        /* :62 */
    struct iovec v = {d->pending, d->fill};
    c->emit(c->user, s, &v, 1, d->fill);
    d->fill = 0;                                                   /* :65 */
}

/* push_to_downstream (sr-main.c:73-83) for the host-side lines (ping) */
static void push(sr_core *c, uint32_t s, const char *line, size_t len) {
    ds_state *d = &c->ds[s];
    if (d->fill + len > SR_DOWNSTREAM_BUF_SIZE) schedule_flush(c, s); /* :75-78 */
    memcpy(d->pending + d->fill, line, len);                         /* :80    */
    d->fill += (uint32_t)len;                                        /* :82    */
}

static int alive_bit(const sr_core *c, uint32_t k) { return (int)((c->alive[k >> 6] >> (k & 63)) & 1u); }

static void build_names(sr_core *c, const sr_core_config *cfg) {
    /* sr-init.c:57: "%s.%s-%d.%s" prefix, hostname, data_port + thread, "healthy_downstreams" */
    snprintf(c->alive_metric, SR_METRIC_SIZE, "%s.%s-%d.%s", cfg->ping_prefix, cfg->hostname, cfg->data_port,
             "healthy_downstreams");
    /* sr-init.c:90-96: the host with '.' -> '_' written over ONE buffer shared by all downstreams and
     * never terminated, so a shorter host keeps the tail of a longer previous one (the reference's
     * buffer starts as stack garbage; zeros here) */
    char mh[SR_METRIC_SIZE];
    memset(mh, 0, sizeof(mh));
    for (uint32_t i = 0; i < c->n; i++) {
        const char *h = cfg->ds_hosts[i], *port = cfg->ds_data_ports[i];
        for (size_t j = 0; h[j] && j < SR_METRIC_SIZE - 1; j++) mh[j] = h[j] == '.' ? '_' : h[j];
        ds_state *d = &c->ds[i];
        /* sr-init.c:112-118 */
        d->conn_len = snprintf(d->conn_metric, SR_METRIC_SIZE, "%s.%s-%d-%s-%s.%s\n%s.%s-%s.%s\n", cfg->ping_prefix,
                               cfg->hostname, cfg->data_port, mh, port, "connections:1|c", cfg->ping_prefix, mh, port,
                               "connections:1|c");
        if (d->conn_len >= (int)SR_METRIC_SIZE) d->conn_len = SR_METRIC_SIZE - 1;
        snprintf(d->packet_metric, SR_METRIC_SIZE, "%s.%s-%s.%s", cfg->ping_prefix, mh, port, "packets");
        snprintf(d->traffic_metric, SR_METRIC_SIZE, "%s.%s-%s.%s", cfg->ping_prefix, mh, port, "traffic");
    }
}

void sr_core_close(sr_core *c) {
    if (!c) return;
    if (c->ctx) sr_close(c->ctx);
    sr_free_host(c->in[0]);
    sr_free_host(c->in[1]);
    sr_free_host(c->sorted);
    free(c->fill16);
    free(c->probed);
    free(c->iov);
    free(c->msg);
    free(c->ping);
    free(c->ping_hash);
    free(c->dg_ends[0]);
    free(c->dg_ends[1]);
    for (int k = 0; k < 2; k++) {
        free(c->slot_lens[k]);
        free(c->slot_ends[k]);
    }
    free(c->alive);
    free(c->ds);
    free(c);
}

int sr_core_open(sr_core **out, const sr_core_config *cfg, sr_core_emit_fn emit, sr_core_log_fn log,
                 sr_core_flush_fn flush, void *user) {
    if (!out || !cfg || !emit || cfg->max_batch_bytes == 0) return -EINVAL;
    if (cfg->n_downstreams == 0 || cfg->n_downstreams > SR_MAX_PACK_DOWNSTREAMS) return -EINVAL;
    if (!cfg->ds_hosts || !cfg->ds_data_ports || !cfg->ping_prefix || !cfg->hostname) return -EINVAL;
    *out = NULL;
    sr_core *c = calloc(1, sizeof(*c));
    if (!c) return -ENOMEM;
    c->n = cfg->n_downstreams;
    c->nwords = (c->n + 63) / 64;
    c->log_level = cfg->log_level;
    c->emit = emit;
    c->log = log;
    c->flush = flush;
    c->user = user;
    c->max_batch = cfg->max_batch_bytes;
    int rc = sr_open(&c->ctx, cfg->device, cfg->max_batch_bytes, c->n);
    if (rc) {
        sr_core_close(c);
        return rc;
    }
    c->in_flight = -1;
    c->host_fills = 1;
    /* TRACE (sr-init.c:252 default): every line's hash from the route kernel, records in input order */
    c->trace = c->log_level <= SR_TRACE && c->log != NULL;
    if (c->trace && (rc = sr_set_trace(c->ctx, 1))) {
        sr_core_close(c);
        return rc;
    }
    c->msg_cap = 3 * SR_DATA_BUF_SIZE;
    c->ds = calloc(c->n, sizeof(ds_state));
    c->alive = calloc(c->nwords, sizeof(uint64_t));
    c->fill16 = calloc(c->n, sizeof(uint16_t));
    c->probed = calloc(c->nwords, sizeof(uint64_t));
    c->iov = calloc(SR_DOWNSTREAM_BUF_SIZE + 2, sizeof(struct iovec));
    c->msg = malloc(c->msg_cap);
    c->ping_cap = ((size_t)c->n + 1) * (SR_METRIC_SIZE + 8);
    c->ping = malloc(c->ping_cap);
    c->sorted_cap = (size_t)c->n + 1;   /* the ping batch: one line per name */
    c->in[0] = sr_alloc_host(cfg->max_batch_bytes);
    c->in[1] = sr_alloc_host(cfg->max_batch_bytes);
    c->sorted = sr_alloc_host(c->sorted_cap * sizeof(sr_record));
    c->ping_hash = calloc(c->sorted_cap, sizeof(uint64_t));
    if (!c->ds || !c->alive || !c->fill16 || !c->probed || !c->iov || !c->msg || !c->ping || !c->in[0] ||
        !c->in[1] || !c->sorted || !c->ping_hash) {
        sr_core_close(c);
        return -ENOMEM;
    }
    /* every health client starts dead (sr-init.c:85) */
    if ((rc = sr_set_alive(c->ctx, c->alive))) {
        sr_core_close(c);
        return rc;
    }
    /* both slots' buffers allocated now (an empty batch each), not while the socket fills */
    for (int k = 0; k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, c->fill16)) || (rc = sr_route_pack_result(c->ctx, k, &r))) {
            sr_core_close(c);
            return rc;
        }
    }
    build_names(c, cfg);
    *out = c;
    return 0;
}

int sr_core_set_alive(sr_core *c, const uint64_t *alive) {
    if (!c || !alive) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    memcpy(c->alive, alive, c->nwords * sizeof(uint64_t));
    if (c->n & 63) c->alive[c->nwords - 1] &= (1ull << (c->n & 63)) - 1;
    return sr_set_alive(c->ctx, c->alive);
}

uint8_t *sr_core_batch_buffer(sr_core *c, size_t *cap) { return sr_core_slot_buffer(c, 0, cap); }

uint8_t *sr_core_slot_buffer(sr_core *c, int slot, size_t *cap) {
    if (!c || slot < 0 || slot > 1) return NULL;
    if (cap) *cap = c->max_batch;
    return c->in[slot];
}

static void drop_probed(sr_core *c) {
    /* find_downstream zeroes the active buffer of each dead downstream it probes (sr-main.c:106) */
    for (uint32_t w = 0; w < c->nwords; w++)
        for (uint64_t m = c->probed[w]; m; m &= m - 1) c->ds[w * 64 + (uint32_t)__builtin_ctzll(m)].fill = 0;
}

/* Where framed byte `off` of the batch in `slot` lies: in the framed bytes, or, for a slot batch, in its
 * datagram's slot (the datagram there is its framed form: sr_core_submit_slots wrote the missing '\n').
 * A line, and a datagram, is one run of bytes either way. With sr_core_set_sample a record in the
 * SR_SAMPLE_APPEND_CAPACITY(nbytes) bytes past the batch's is a rewritten line: it lies in the slot's sample text.
 * With sr_core_set_coalesce a record past that (past the batch's bytes, without the sampling) is a merged line: it
 * lies in the slot's merged text. */
static const uint8_t *batch_at(const sr_core *c, int slot, const uint8_t *framed, uint32_t off) {
    if (c->co_text[slot] && off >= c->co_base[slot]) return c->co_text[slot] + (off - c->co_base[slot]);
    if (c->sa_text[slot] && off >= c->sa_base[slot]) return c->sa_text[slot] + (off - c->sa_base[slot]);
    if (!c->slot_n[slot]) return framed + off;
    return sr_slot_addr(c->in[slot], SR_DATA_BUF_SIZE, c->slot_ends[slot], c->slot_n[slot], off);
}

/* The WARN line of an unrouted record, with the reference's text. */
static void warn_line(sr_core *c, int slot, const uint8_t *framed, const sr_record *r) {
    const char *line = (const char *)batch_at(c, slot, framed, r->offset);
    const int len = r->length;
    if (r->route == SR_ROUTE_INVALID_LENGTH) {
        /* sr-main.c:184 */
        core_log(c, SR_WARN, "%s: invalid length %d of metric %.*s", "udp_read_cb", len, len, line);
    } else if (r->route == SR_ROUTE_INVALID_FORMAT) {
        /* sr-main.c:141-142: the '\n' becomes NUL and the line is printed with %s */
        core_log(c, SR_WARN, "%s: invalid metric %.*s", "process_data_line", len - 1, line);
    } else {
        core_log(c, SR_WARN, "%s: all downstreams are dead", "find_downstream"); /* sr-main.c:115 */
    }
}

/* find_downstream's TRACE lines for a line that passed the length and ':' tests (sr-main.c:91,102):
 * its hash, then its first live pick, or the WARN when every downstream is dead (:115). */
static void trace_line(sr_core *c, const char *line, int len, uint64_t h, uint32_t route) {
    core_log(c, SR_TRACE, "%s: hash = %lx, length = %d, line = %.*s", "find_downstream", (unsigned long)h, len, len,
             line);
    if (route < c->n) core_log(c, SR_TRACE, "%s: pushing to downstream %d", "find_downstream", (int)route);
    else core_log(c, SR_WARN, "%s: all downstreams are dead", "find_downstream");
}

/* TRACE: every message of udp_read_cb for the batch in slot `slot`, in input order: per datagram
 * "got packet" (sr-main.c:174), then per line its WARN (:142,184) or its find_downstream lines. */
static int trace_batch(sr_core *c, int slot, const uint8_t *framed, size_t nbytes) {
    const sr_record *rec;
    const uint64_t *hs;
    size_t n = 0, i = 0, d0 = 0;
    int rc = sr_route_pack_trace(c->ctx, slot, &rec, &hs, &n);
    if (rc) {
        core_log(c, SR_ERROR, "%s: sr_route_pack_trace() failed %s", "udp_read_cb", strerror(-rc));
        c->dg_n[slot] = 0;
        return rc;
    }
    /* a slot batch brings its own boundaries: one per slot, an empty datagram repeating the one before
     * (the reference logs nothing for it, sr-main.c:170) */
    const size_t nd = c->slot_n[slot] ? c->slot_n[slot] : c->dg_n[slot];
    const uint32_t *ends = c->slot_n[slot] ? c->slot_ends[slot] : c->dg_ends[slot];
    for (size_t g = 0; g <= nd; g++) {   /* the datagrams, then whatever no boundary covers */
        const size_t end = g < nd ? ends[g] : nbytes;
        if (g < nd && (end > d0 || !c->slot_n[slot]))
            core_log(c, SR_TRACE, "%s: got packet %.*s", "udp_read_cb", (int)(end - d0),
                     (const char *)batch_at(c, slot, framed, (uint32_t)d0));
        for (; i < n && (g == nd || rec[i].offset < end); i++) {
            if (rec[i].route == SR_ROUTE_INVALID_LENGTH || rec[i].route == SR_ROUTE_INVALID_FORMAT)
                warn_line(c, slot, framed, &rec[i]);
            else
                trace_line(c, (const char *)batch_at(c, slot, framed, rec[i].offset), rec[i].length, hs[i],
                           rec[i].route);
        }
        d0 = end;
    }
    c->dg_n[slot] = 0;
    return 0;
}

/* sr_core_set_device_log: the batch's messages as the GPU wrote them into the slot (sr_route_pack_logtext),
 * to the block callback in one call or to the log callback one by one. Not 0: the text or its index did not
 * fit, or the slot has none; the caller formats the batch on the host. */
static int device_log(sr_core *c, int slot) {
    const uint8_t *text;
    const uint32_t *offs;
    const uint8_t *lv;
    uint64_t total = 0;
    size_t n = 0;
    int rc = c->log_host[slot] ? -ENOSPC : sr_route_pack_logtext(c->ctx, slot, &text, &total, &offs, &lv, &n);
    if (rc) {
        c->log_host_n++;
        return rc;
    }
    c->log_device_n++;
    if (c->log_block) {
        if (n) c->log_block(c->user, (const char *)text, (size_t)total, n);
    } else {
        for (size_t i = 0; i < n; i++)
            c->log(c->user, lv[i], (const char *)text + offs[i], (size_t)(offs[i + 1] - offs[i]) - 1);
    }
    c->dg_n[slot] = 0;
    return 0;
}

/* The host's half of a batch (udp_read_cb's per-line side effects, sr-main.c:175-189, for a whole
 * batch): drop probed dead buffers, the log lines in input order, then the packets per downstream. */
static void complete(sr_core *c, int slot, const uint8_t *framed, size_t nbytes, const sr_pack_result *r) {
    memcpy(c->probed, r->probed_dead, c->nwords * sizeof(uint64_t));
    drop_probed(c);
    c->co_text[slot] = NULL;
    c->sa_text[slot] = NULL;
    size_t sa_room = 0;  /* the sample text's room in the device's batch, between the batch and the merged text */
    if (c->sample) {     /* the rewritten lines' bytes, behind the batch's own */
        const uint8_t *text = NULL;
        size_t len = 0;
        uint64_t counts[4], seed = 0;
        const int rc = sr_route_pack_sample(c->ctx, slot, &text, &len, counts, &seed);
        if (rc) {   /* (the text of a routed batch always fits: nothing of this batch can be sent) */
            core_log(c, SR_ERROR, "%s: sr_route_pack_sample() failed %s", "udp_read_cb", strerror(-rc));
            c->host_fills = 1;
            c->dg_n[slot] = 0;
            return;
        }
        c->sa_text[slot] = text;
        c->sa_base[slot] = nbytes;
        sa_room = SR_SAMPLE_APPEND_CAPACITY(nbytes);
    }
    if (c->coalesce) {   /* the merged lines' bytes, behind the batch's own and the sample text's room */
        const uint8_t *text = NULL;
        size_t len = 0;
        uint64_t counts[4];
        const int rc = sr_route_pack_coalesced(c->ctx, slot, &text, &len, counts);
        if (rc) {   /* (the text of a routed batch always fits: nothing of this batch can be sent) */
            core_log(c, SR_ERROR, "%s: sr_route_pack_coalesced() failed %s", "udp_read_cb", strerror(-rc));
            c->host_fills = 1;
            c->dg_n[slot] = 0;
            return;
        }
        c->co_text[slot] = text;
        c->co_base[slot] = nbytes + sa_room;
        for (int q = 0; q < 4; q++) c->co_totals[q] += counts[q];
    }
    /* without the TRACE inputs (the slot was not traced) the WARN lines still come, from the sorted
     * records' unrouted tail, in input order */
    if (c->devlog && device_log(c, slot) == 0) {
        /* logged */
    } else if ((!c->trace || trace_batch(c, slot, framed, nbytes) != 0) && c->log_level <= SR_WARN)
        for (size_t i = r->n_valid; i < r->n_records; i++) warn_line(c, slot, framed, &r->sorted[i]);
    /* sr_core_set_payloads: the packets' lines laid end to end by the GPU, packet q at
     * arena[offs[q] + carry, offs[q + 1]) (the carry's room is unwritten: the host holds those bytes) */
    const uint8_t *arena = NULL;
    const uint32_t *offs = NULL;
    size_t n_arena = 0;
    if (c->payloads && (sr_route_pack_payloads(c->ctx, slot, &arena, &offs, &n_arena) != 0 || n_arena != r->n_packets)) {
        core_log(c, SR_ERROR, "%s: sr_route_pack_payloads() failed", "udp_read_cb");
        arena = NULL;   /* the line list below serves the batch */
    }
    for (size_t q = 0; q < r->n_packets; q++) {
        const sr_packet *p = &r->packets[q];
        ds_state *d = &c->ds[p->shard];
        const sr_record *rec = r->sorted + p->first;
        if (arena) {
            const uint8_t *lines = arena + offs[q] + p->carry;
            if (p->open) {   /* the carried bytes are in place already */
                memcpy(d->pending + p->carry, lines, p->length);
                d->fill = (uint32_t)p->carry + p->length;
                continue;
            }
            int iv = 0;
            if (p->carry) c->iov[iv++] = (struct iovec){d->pending, p->carry};
            if (p->length) c->iov[iv++] = (struct iovec){(void *)lines, p->length};
            const uint32_t bytes = (uint32_t)p->carry + p->length;
            d->packets += 1;
            d->traffic = (int32_t)((uint32_t)d->traffic + bytes);
            c->emit(c->user, p->shard, c->iov, iv, bytes);
            d->fill = 0;
            continue;
        }
        if (p->open) {
            /* the new active buffer: the carried bytes (already in place) + this batch's lines */
            uint32_t f = p->carry;
            for (uint32_t k = 0; k < p->nlines; k++) {
                memcpy(d->pending + f, batch_at(c, slot, framed, rec[k].offset), rec[k].length);
                f += rec[k].length;
            }
            d->fill = f;
            continue;
        }
        int iv = 0;
        if (p->carry) c->iov[iv++] = (struct iovec){d->pending, p->carry};
        for (uint32_t k = 0; k < p->nlines; k++)
            c->iov[iv++] = (struct iovec){(void *)batch_at(c, slot, framed, rec[k].offset), rec[k].length};
        const uint32_t bytes = (uint32_t)p->carry + p->length;
        d->packets += 1;
        d->traffic = (int32_t)((uint32_t)d->traffic + bytes);
        c->emit(c->user, p->shard, c->iov, iv, bytes);
        d->fill = 0;
    }
    if (c->flush) c->flush(c->user);
}

/* Start a batch on the GPU; the pending bytes are the device's own unless the host changed them. */
static int submit(sr_core *c, int slot, const uint8_t *framed, size_t nbytes) {
    const uint16_t *fill = NULL;
    if (c->host_fills) {   /* nothing is in flight here: the host's fills are current */
        for (uint32_t s = 0; s < c->n; s++) c->fill16[s] = (uint16_t)c->ds[s].fill;
        fill = c->fill16;
    }
    if (c->devlog) {   /* staged for this submission only */
        /* A batch that cannot be staged (more datagram ends than the slot's staging holds, or a staging
         * error) is still routed: the host formats its log, as for a text that did not fit. */
        int rc = 0;
        c->log_host[slot] = 0;
        if (c->log_block) {
            char pfx[2 * SR_LOG_MAX_PREFIX];
            size_t tl = c->trace ? c->log_prefix(c->user, SR_TRACE, pfx, SR_LOG_MAX_PREFIX) : 0;
            if (tl > SR_LOG_MAX_PREFIX) tl = SR_LOG_MAX_PREFIX;
            size_t wl = c->log_prefix(c->user, SR_WARN, pfx + tl, SR_LOG_MAX_PREFIX);
            if (wl > SR_LOG_MAX_PREFIX) wl = SR_LOG_MAX_PREFIX;
            rc = sr_route_pack_set_prefix(c->ctx, slot, (const uint8_t *)pfx, tl, (const uint8_t *)pfx + tl, wl);
        }
        if (!rc && c->trace && !c->slot_n[slot]) {
            if (c->dg_n[slot] > SR_MAX_SLOTS) rc = -ENOSPC;
            else rc = sr_route_pack_set_ends(c->ctx, slot, c->dg_ends[slot], c->dg_n[slot]);
        }
        if (rc) c->log_host[slot] = 1;
    }
    int rc = c->slot_n[slot] ? sr_route_pack_submit_slots(c->ctx, slot, c->in[slot], SR_DATA_BUF_SIZE, c->slot_lens[slot],
                                                          c->slot_n[slot], fill)
                             : sr_route_pack_submit(c->ctx, slot, framed, nbytes, fill);
    if (rc) return rc;
    c->host_fills = 0;
    return 0;
}

static int finish(sr_core *c, int slot, const uint8_t *framed, size_t nbytes) {
    sr_pack_result r;
    int rc = sr_route_pack_result(c->ctx, slot, &r);
    if (!rc && c->fail_finish && ++c->finishes == c->fail_finish) rc = -EIO;   /* fault injection */
    if (rc) {
        c->host_fills = 1;   /* the device's chain is no longer what the host holds */
        c->dg_n[slot] = 0;
        return rc;
    }
    complete(c, slot, framed, nbytes, &r);
    return 0;
}

int sr_core_drain(sr_core *c) {
    if (!c) return -EINVAL;
    if (c->in_flight < 0) return 0;
    const int slot = c->in_flight;
    c->in_flight = -1;
    return finish(c, slot, c->in_flight_bytes, c->in_flight_len);
}

/* TRACE: the datagram ends of the batch about to go into `slot` (copied) */
static int note_datagrams(sr_core *c, int slot, const uint32_t *ends, size_t n) {
    c->dg_n[slot] = 0;
    if (!c->trace || !n) return 0;
    if (!ends) return -EINVAL;
    if (n > c->dg_cap[slot]) {
        uint32_t *p = realloc(c->dg_ends[slot], n * sizeof(uint32_t));
        if (!p) return -ENOMEM;
        c->dg_ends[slot] = p;
        c->dg_cap[slot] = n;
    }
    memcpy(c->dg_ends[slot], ends, n * sizeof(uint32_t));
    c->dg_n[slot] = n;
    return 0;
}

/* Start the batch prepared in `slot` (framed bytes, or slots when slot_n[slot] != 0) and complete the other
 * slot's batch: the common half of sr_core_submit_datagrams and sr_core_submit_slots. */
static int submit_slot(sr_core *c, int slot, size_t nbytes) {
    int rc;
    if ((rc = submit(c, slot, c->in[slot], nbytes))) {
        c->dg_n[slot] = 0;
        c->slot_n[slot] = 0;
        return rc;   /* nothing submitted: sr_core_in_flight() is not `slot` */
    }
    const int prev = c->in_flight;
    const uint8_t *prev_bytes = c->in_flight_bytes;
    const size_t prev_len = c->in_flight_len;
    c->in_flight = slot;
    c->in_flight_bytes = c->in[slot];
    c->in_flight_len = nbytes;
    if (prev < 0) return 0;
    if ((rc = finish(c, prev, prev_bytes, prev_len)) == 0) return 0;
    /* The previous batch failed, so its packets never reached the pending buffers the new batch's
     * device-chained fills assume: take the new batch back and route it again from the host's fills
     * (finish() set host_fills), so that host and device agree on every pending buffer. */
    sr_pack_result r;
    const int rc_back = sr_route_pack_result(c->ctx, slot, &r);
    if (rc_back && rc_back != -ENOSPC)
        core_log(c, SR_ERROR, "%s: taking back the batch after a failed one failed %s", "udp_read_cb",
                 strerror(-rc_back));
    c->in_flight = -1;
    if (submit(c, slot, c->in[slot], nbytes) == 0) c->in_flight = slot;   /* (its datagram ends kept) */
    else c->dg_n[slot] = c->slot_n[slot] = 0;
    return rc;
}

int sr_core_submit_datagrams(sr_core *c, int slot, size_t nbytes, const uint32_t *ends, size_t n_datagrams) {
    if (!c || slot < 0 || slot > 1 || nbytes > c->max_batch) return -EINVAL;
    if (c->in_flight == slot) return -EBUSY;
    if (nbytes == 0) return 0;
    if (c->fail_submit && ++c->submits == c->fail_submit) return -EIO;   /* as a failed sr_route_pack_submit */
    c->slot_n[slot] = 0;
    int rc = note_datagrams(c, slot, ends, n_datagrams);
    if (rc) return rc;
    return submit_slot(c, slot, nbytes);
}

int sr_core_submit_slots(sr_core *c, int slot, const uint16_t *lens, size_t n_slots) {
    if (!c || slot < 0 || slot > 1 || (n_slots && !lens)) return -EINVAL;
    const size_t room = c->max_batch / SR_DATA_BUF_SIZE;
    if (n_slots > room || n_slots > SR_MAX_SLOTS) return -EINVAL;
    if (c->in_flight == slot) return -EBUSY;
    if (!c->slot_lens[slot]) {   /* once per slot, for the whole arena */
        uint16_t *l = malloc((room ? room : 1) * sizeof(uint16_t));
        uint32_t *e = malloc((room ? room : 1) * sizeof(uint32_t));
        if (!l || !e) {
            free(l);
            free(e);
            return -ENOMEM;
        }
        c->slot_lens[slot] = l;
        c->slot_ends[slot] = e;
    }
    /* udp_read_cb's framing in place (sr-main.c:163-173): the cap, and the missing '\n' written behind the
     * datagram, so that the slot holds its framed form for the host's own reads; the device frames the same
     * bytes from the lengths as received */
    uint32_t pos = 0;
    for (size_t j = 0; j < n_slots; j++) {
        uint8_t *d = c->in[slot] + j * SR_DATA_BUF_SIZE;
        const uint32_t n = lens[j] < SR_MAX_DATAGRAM ? lens[j] : SR_MAX_DATAGRAM;
        if (n) {
            pos += n;
            if (d[n - 1] != '\n') {
                d[n] = '\n';
                pos += 1;
            }
        }
        c->slot_lens[slot][j] = lens[j];
        c->slot_ends[slot][j] = pos;
    }
    if (pos == 0) return 0;
    if (c->fail_submit && ++c->submits == c->fail_submit) return -EIO;   /* as a failed sr_route_pack_submit */
    c->dg_n[slot] = 0;
    c->slot_n[slot] = n_slots;
    return submit_slot(c, slot, pos);
}

int sr_core_submit(sr_core *c, int slot, size_t nbytes) { return sr_core_submit_datagrams(c, slot, nbytes, NULL, 0); }

int sr_core_in_flight(const sr_core *c) { return c ? c->in_flight : -EINVAL; }

int sr_core_route_datagrams(sr_core *c, const uint8_t *framed, size_t nbytes, const uint32_t *ends,
                            size_t n_datagrams) {
    if (!c || (nbytes && !framed) || nbytes > c->max_batch) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    if (nbytes == 0) return 0;
    c->slot_n[0] = 0;
    if ((rc = note_datagrams(c, 0, ends, n_datagrams))) return rc;
    if ((rc = submit(c, 0, framed, nbytes))) {
        c->dg_n[0] = 0;
        return rc;
    }
    return finish(c, 0, framed, nbytes);
}

int sr_core_route(sr_core *c, const uint8_t *framed, size_t nbytes) {
    return sr_core_route_datagrams(c, framed, nbytes, NULL, 0);
}

sr_ctx *sr_core_context(sr_core *c) { return c ? c->ctx : NULL; }

int sr_core_set_payloads(sr_core *c, int on) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    int rc = sr_set_payloads(c->ctx, on);
    if (rc) return rc;
    c->payloads = on ? 1 : 0;
    /* both slots' arenas allocated now (an empty batch each; the device's pending bytes carry over) */
    for (int k = 0; on && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return 0;
}

int sr_core_set_device_log(sr_core *c, int on, size_t text_cap, sr_core_log_prefix_fn prefix, sr_core_log_block_fn block) {
    if (!c || (on && block && !prefix)) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    /* a core that logs nothing of a batch (log_level above WARN, or no callback at all) has nothing to format */
    const int wanted = on && c->log_level <= SR_WARN && (block || c->log);
    int rc = sr_set_logtext(c->ctx, wanted ? (c->log_level <= SR_TRACE ? SR_TRACE : SR_WARN) : -1, text_cap,
                            wanted ? (block ? SR_CORE_LOG_MAX_MSG : (uint32_t)c->msg_cap - 1) : 0);   /* core_log's cut */
    if (rc) return rc;
    c->devlog = wanted ? 1 : 0;
    c->log_prefix = wanted ? prefix : NULL;
    c->log_block = wanted ? block : NULL;
    /* both slots' arenas allocated now (an empty batch each; the device's pending bytes carry over) */
    for (int k = 0; wanted && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return 0;
}

int sr_core_device_log_stats(const sr_core *c, uint64_t *device_batches, uint64_t *host_batches) {
    if (!c) return -EINVAL;
    if (device_batches) *device_batches = c->log_device_n;
    if (host_batches) *host_batches = c->log_host_n;
    return 0;
}

int sr_core_set_name_stats(sr_core *c, const sr_stats_config *cfg) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    return sr_set_name_stats(c->ctx, cfg);
}

int sr_core_set_coalesce(sr_core *c, const sr_coalesce_config *cfg) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    int rc = sr_set_coalesce(c->ctx, cfg);
    if (rc) return rc;
    c->coalesce = cfg ? 1 : 0;
    c->co_text[0] = c->co_text[1] = NULL;
    /* both slots' text buffers allocated now (an empty batch each; the device's pending bytes carry over) */
    for (int k = 0; cfg && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return 0;
}

int sr_core_set_name_rules(sr_core *c, const sr_rules_config *cfg) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    int rc = sr_set_name_rules(c->ctx, cfg);
    if (rc) return rc;
    /* both slots' counts allocated now (an empty batch each; the device's pending bytes carry over) */
    for (int k = 0; cfg && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return 0;
}

int sr_core_name_rule_hits(sr_core *c, sr_rule_hits *hits, size_t n, int reset) {
    if (!c || (n && !hits)) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    const int got = sr_rules_read(c->ctx, hits, n);
    if (got < 0) return got;
    if (reset && (rc = sr_rules_reset(c->ctx))) return rc;
    return got;
}

int sr_core_set_validate(sr_core *c, const sr_validate_config *cfg) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    int rc = sr_set_validate(c->ctx, cfg);
    if (rc) return rc;
    /* both slots' counts allocated now (an empty batch each; the device's pending bytes carry over) */
    for (int k = 0; cfg && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return 0;
}

int sr_core_validate_hits(sr_core *c, sr_validate_hits *hits, size_t n, int reset) {
    if (!c || (n && !hits)) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    const int got = sr_validate_read(c->ctx, hits, n);
    if (got < 0) return got;
    if (reset && (rc = sr_validate_reset(c->ctx))) return rc;
    return got;
}

int sr_core_set_sample(sr_core *c, const sr_sample_config *cfg) {
    if (!c) return -EINVAL;
    if (c->in_flight >= 0) return -EBUSY;
    int rc = sr_set_sample(c->ctx, cfg);
    if (rc) return rc;
    c->sample = cfg ? 1 : 0;
    c->sa_text[0] = c->sa_text[1] = NULL;
    /* both slots' text buffers allocated now (an empty batch each; the device's pending bytes carry over); then
     * the switch once more, so that the first batch of lines is thinned under the configuration's own seed */
    for (int k = 0; cfg && k < 2; k++) {
        sr_pack_result r;
        if ((rc = sr_route_pack_submit(c->ctx, k, NULL, 0, NULL)) || (rc = sr_route_pack_result(c->ctx, k, &r))) return rc;
    }
    return cfg ? sr_set_sample(c->ctx, cfg) : 0;
}

int sr_core_sample_hits(sr_core *c, sr_sample_hits *hits, size_t n, int reset) {
    if (!c || (n && !hits)) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    const int got = sr_sample_read(c->ctx, hits, n);
    if (got < 0) return got;
    if (reset && (rc = sr_sample_reset(c->ctx))) return rc;
    return got;
}

int sr_core_coalesce_counts(sr_core *c, uint64_t totals[4], int reset) {
    if (!c || !totals) return -EINVAL;
    memcpy(totals, c->co_totals, sizeof(c->co_totals));
    if (reset) memset(c->co_totals, 0, sizeof(c->co_totals));
    return 0;
}

int sr_core_name_stats(sr_core *c, sr_stats_snapshot **out, int reset) {
    if (out) *out = NULL;
    if (!c || !out) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    if ((rc = sr_stats_read(c->ctx, out))) return rc;
    return reset ? sr_stats_reset(c->ctx) : 0;
}

int sr_core_inject_faults(sr_core *c, unsigned fail_submit, unsigned fail_finish) {
    if (!c) return -EINVAL;
    c->fail_submit = fail_submit;
    c->fail_finish = fail_finish;
    c->submits = c->finishes = 0;
    return 0;
}

int sr_core_flush_timer(sr_core *c) {
    if (!c) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    c->host_fills = 1;
    for (uint32_t s = 0; s < c->n; s++)
        if (c->ds[s].fill > 0) schedule_flush(c, s); /* sr-main.c:199-203 */
    if (c->flush) c->flush(c->user);
    return 0;
}

int sr_core_ping(sr_core *c) {
    if (!c) return -EINVAL;
    int rc = sr_core_drain(c);
    if (rc) return rc;
    c->host_fills = 1;
    /* The shard of a ping line depends only on its name (the bytes before ':') and the alive bits,
     * so the n + 1 names are routed on the GPU in one batch first; the texts, whose counters change
     * as earlier lines are pushed, are formatted afterwards in the reference's order. */
    size_t pos = 0;
    uint8_t *b = c->ping;
    for (uint32_t i = 0; i <= c->n; i++) {
        const char *name = i < c->n ? c->ds[i].traffic_metric : c->alive_metric;
        int k = snprintf((char *)b + pos, c->ping_cap - pos, "%s:0|%c\n", name, i < c->n ? 'c' : 'g');
        if (k < 0 || pos + (size_t)k >= c->ping_cap) return -ENOSPC;
        pos += (size_t)k;
    }
    if (pos > c->max_batch) return -ENOSPC;
    size_t nr = 0;
    rc = sr_route_batch(c->ctx, b, pos, c->sorted, c->sorted_cap, &nr, c->trace ? c->ping_hash : NULL);
    if (rc) return rc;
    if (nr != c->n + 1) return -EIO;
    if ((rc = sr_last_probed_dead(c->ctx, c->probed))) return rc;
    drop_probed(c); /* only dead downstreams: none of them receives a ping line */
    char buf[2 * SR_METRIC_SIZE + 64];
    int count = 0;
    for (uint32_t i = 0; i < c->n; i++) {
        ds_state *d = &c->ds[i];
        if (alive_bit(c, i)) { /* sr-main.c:220-223 */
            push(c, i, d->conn_metric, (size_t)d->conn_len);
            count++;
        }
        const int32_t traffic = d->traffic, packets = d->packets; /* :224-227 */
        d->traffic = 0;
        d->packets = 0;
        const int n = snprintf(buf, sizeof(buf), "%s:%d|c\n%s:%d|c\n", d->traffic_metric, traffic, d->packet_metric,
                               packets);
        const uint16_t route = c->sorted[i].route; /* process_data_line, :231 */
        if (c->trace) trace_line(c, buf, n, c->ping_hash[i], route);
        else if (route >= c->n) core_log(c, SR_WARN, "%s: all downstreams are dead", "find_downstream");
        if (route < c->n) push(c, route, buf, (size_t)n);
    }
    const int n = snprintf(buf, sizeof(buf), "%s:%d|g\n", c->alive_metric, count); /* :233-234 */
    const uint16_t route = c->sorted[c->n].route;
    if (c->trace) trace_line(c, buf, n, c->ping_hash[c->n], route);
    else if (route >= c->n) core_log(c, SR_WARN, "%s: all downstreams are dead", "find_downstream");
    if (route < c->n) push(c, route, buf, (size_t)n);
    if (c->flush) c->flush(c->user);
    return 0;
}

int sr_core_state(const sr_core *c, uint32_t s, const uint8_t **pending, size_t *len, int32_t *traffic,
                  int32_t *packets) {
    if (!c || s >= c->n) return -EINVAL;
    if (pending) *pending = c->ds[s].pending;
    if (len) *len = c->ds[s].fill;
    if (traffic) *traffic = c->ds[s].traffic;
    if (packets) *packets = c->ds[s].packets;
    return 0;
}

const char *sr_core_metric_name(const sr_core *c, uint32_t s, int which) {
    if (!c) return NULL;
    if (which == 3) return c->alive_metric;
    if (s >= c->n) return NULL;
    return which == 0 ? c->ds[s].conn_metric : which == 1 ? c->ds[s].traffic_metric : c->ds[s].packet_metric;
}
