/*
 * sr_router.h — one data thread of the MI355X statsd-router, on top of the C ABI in sr_route.h.
 *
 * The reference runs one libev loop per data thread (data_pipe_thread, sr-main.c:237-308), each
 * with its own copy of the downstream array (sr-main.c:249): a 1450-byte active buffer per
 * downstream that lines are appended to (push_to_downstream, sr-main.c:73-83) and that is
 * flushed when the next line would not fit or on the flush timer (ds_schedule_flush /
 * ds_flush_timer_cb, sr-main.c:49-71,194-204), plus per-downstream traffic / packet counters and
 * the self-metrics of ping_cb (sr-main.c:206-235).
 *
 * sr_core is that per-thread state with the per-line work moved to the GPU: a batch of framed
 * datagrams is classified, hashed, shard-picked AND packed into per-downstream packets on the
 * device (sr_route_pack_batch); the host only walks the packet descriptors (one iovec per line),
 * drops the pending buffers of probed dead downstreams (sr-main.c:106) and formats the WARN
 * lines of invalid lines with the reference's exact texts (sr-main.c:115,142,184). Timers (flush,
 * ping) run on the host between batches, exactly as libev runs them between read callbacks.
 *
 * Conventions: 0 or a negative errno; not thread-safe (one sr_core per data thread).
 */
#ifndef SR_ROUTER_H
#define SR_ROUTER_H

#include <stddef.h>
#include <stdint.h>
#include <sys/uio.h>

#include "sr_route.h"

#ifdef __cplusplus
extern "C" {
#endif

/* log levels of the reference logger (sr-util.h:15-21) */
enum sr_log_level { SR_TRACE = 0, SR_DEBUG = 1, SR_INFO = 2, SR_WARN = 3, SR_ERROR = 4 };

#define SR_METRIC_SIZE 256u  /* sr-types.h:32: buffers of the ping metric names */

typedef struct sr_core_config {
    int device;                        /* HIP device of the thread's context                    */
    size_t max_batch_bytes;            /* framed bytes per sr_core_route call                    */
    uint32_t n_downstreams;            /* the `downstream=` list of statsd-router.conf           */
    const char *const *ds_hosts;       /* each downstream's host, as written in the config        */
    const char *const *ds_data_ports;  /* each downstream's data port, as written                 */
    const char *ping_prefix;           /* ping_prefix=                                             */
    const char *hostname;              /* gethostname() of the router (sr-init.c:298)             */
    int data_port;                     /* data_port + thread index: the names of sr-init.c:57,113 */
    int log_level;                     /* messages below this level are not even formatted        */
} sr_core_config;

/* A flushed packet for downstream ds: iov[0..iovcnt) concatenated, `bytes` in total (<= 1450).
 * The iovecs point into core-owned and caller-owned memory that later calls overwrite: the
 * callback must consume them (send or copy) before it returns. */
typedef void (*sr_core_emit_fn)(void *user, uint32_t ds, const struct iovec *iov, int iovcnt, size_t bytes);
/* A log message (no trailing newline, no timestamp: the text the reference passes to log_msg). */
typedef void (*sr_core_log_fn)(void *user, int level, const char *msg, size_t len);
/* Called once at the end of every call that may have emitted packets (e.g. to sendmmsg them). */
typedef void (*sr_core_flush_fn)(void *user);

typedef struct sr_core sr_core;
int sr_core_open(sr_core **core, const sr_core_config *cfg, sr_core_emit_fn emit, sr_core_log_fn log,
                 sr_core_flush_fn flush, void *user);

/* The health checker's alive bits (sr-types.h:25): ceil(n/64) words. All start DEAD, as in the
 * reference (sr-init.c:85). */
int sr_core_set_alive(sr_core *core, const uint64_t *alive);

/* A page-locked buffer of max_batch_bytes the caller may frame datagrams into (optional; it is slot
 * 0's buffer of the double-buffered calls below). */
uint8_t *sr_core_batch_buffer(sr_core *core, size_t *capacity);

/* Route one batch of framed datagrams (sr_frame_datagram output, back to back): what the
 * reference does in udp_read_cb for each datagram in turn (sr-main.c:149-191). */
int sr_core_route(sr_core *core, const uint8_t *framed, size_t nbytes);

/* Double-buffered routing: the host's work on one batch (walking its packets, the emit and log
 * callbacks, receiving the next datagrams) overlaps the GPU's work on the next (sr_route_pack_submit).
 * The core owns two page-locked batch buffers, slots 0 and 1 (sr_core_slot_buffer). sr_core_submit
 * starts routing slot `slot`'s first nbytes, then completes the OTHER slot's batch if one is in
 * flight (its packets are emitted, its WARN lines logged, the flush callback called), so when it
 * returns at most `slot` is in flight and the other slot's buffer may be refilled. sr_core_drain
 * completes the batch in flight, if any. Batches complete in submission order, with exactly the
 * packets, pending buffers, counters and log lines that sr_core_route would produce for them one
 * after another; pending bytes chain on the device between batches. sr_core_route,
 * sr_core_flush_timer, sr_core_ping and sr_core_set_alive drain first. Returns 0, -EBUSY (the slot is
 * in flight), -EINVAL or an sr_route_pack_* error. */
uint8_t *sr_core_slot_buffer(sr_core *core, int slot, size_t *capacity);
int sr_core_submit(sr_core *core, int slot, size_t nbytes);
int sr_core_drain(sr_core *core);

/* The same two calls with the batch's datagram boundaries: ends[i] is the end offset (exclusive) of
 * framed datagram i in the batch, ascending, the last = nbytes (empty datagrams have no entry: the
 * reference logs nothing for them, sr-main.c:170). Only a core opened at log_level SR_TRACE reads
 * them: it logs, in input order, "udp_read_cb: got packet ..." per datagram (sr-main.c:174) and, per
 * line that reaches find_downstream, its hash and first live pick (sr-main.c:91,102) between the WARN
 * lines, from the GPU's per-line hashes (sr_set_trace). Without boundaries (the calls above) a TRACE
 * core logs the per-line messages only. The array is copied; it may be reused on return. */
int sr_core_route_datagrams(sr_core *core, const uint8_t *framed, size_t nbytes, const uint32_t *ends,
                            size_t n_datagrams);
int sr_core_submit_datagrams(sr_core *core, int slot, size_t nbytes, const uint32_t *ends, size_t n_datagrams);

/* sr_core_submit for datagrams that stay where recvmmsg left them: slot `slot`'s buffer
 * (sr_core_slot_buffer) is read as an arena of capacity / SR_DATA_BUF_SIZE slots of SR_DATA_BUF_SIZE bytes,
 * datagram j in the first lens[j] bytes of slot j (lengths above SR_MAX_DATAGRAM are capped, as recv()
 * caps them). Nothing is moved: the datagrams are framed on the device (sr_route_pack_submit_slots). The
 * core computes the framed ends itself and writes a missing final '\n' into the byte behind a datagram
 * (slot j's byte lens[j], always inside the slot), so that WARN and TRACE texts, "got packet" lines, the
 * packets' iovecs and the new pending buffers are read from the slots. lens is copied. Everything else is
 * sr_core_submit's: the other slot's batch is completed, batches complete in submission order with the
 * packets, counters and log lines sr_core_route would produce for the same datagrams framed, sr_core_drain,
 * sr_core_set_payloads and the fault injection apply unchanged, and a TRACE core needs no boundaries
 * argument (every slot is a datagram). The slot's buffer must stay unchanged until the batch completes.
 * Returns 0, -EBUSY, -EINVAL (n_slots over the arena or SR_MAX_SLOTS), -ENOMEM or an sr_route_pack_* error. */
int sr_core_submit_slots(sr_core *core, int slot, const uint16_t *lens, size_t n_slots);

/* The core's device context (sr_route.h), e.g. for sr_set_layout or sr_set_knob (developer A/B runs).
 * Owned by the core. */
sr_ctx *sr_core_context(sr_core *core);

/* Packets from the device's arena. With sr_core_set_payloads(core, 1) every later batch also has its
 * packets' bytes gathered on the GPU (sr_set_payloads, sr_route.h), and a flushed packet reaches the emit
 * callback as at most two pieces: the bytes pending before the batch (when it has any), then its lines
 * as one run of the slot's arena, valid until the emit callback and the flush callback after it have
 * returned; the downstream's new pending buffer is one copy out of the arena. Packets, counters, log
 * lines and their order are the same either way. Off by default. Returns 0, -EINVAL, -EBUSY (a batch is
 * in flight: drain first). */
int sr_core_set_payloads(sr_core *core, int on);

/* Log text from the device. With sr_core_set_device_log(core, 1, ...) every later batch also has its log
 * messages written on the GPU (sr_set_logtext, sr_route.h: "got packet" per datagram, the WARN of every dropped
 * line, and at log_level SR_TRACE the two find_downstream messages per routed line), at the core's log_level,
 * into page-locked memory of the slot of text_cap bytes (0: SR_CORE_LOG_DEFAULT_TEXT_CAP of max_batch_bytes).
 *   block == NULL: when the batch completes its messages go one by one to the log callback, as (level, text)
 *     without prefix or newline, each cut like the host formatter's (12287 bytes): the sequence the host
 *     formatter produces. One corner differs: for a datagram end that repeats the one before it in
 *     sr_core_submit_datagrams' ends (an empty datagram, which by that call's contract has no entry) the host
 *     formatter logs an empty "got packet" and the device logs none, as the reference does (sr-main.c:170).
 *   block != NULL: prefix(user, level, dst, cap) is asked for the SR_TRACE (a TRACE core only) and the SR_WARN
 *     prefix when the batch is submitted (it writes at most cap = SR_LOG_MAX_PREFIX bytes to dst and returns
 *     their count); every message is prefix[level] + text cut to SR_CORE_LOG_MAX_MSG bytes (log_msg's
 *     2048-byte buffer, sr-util.c:14-27) + '\n', and the batch's whole text goes to block(user, text, len,
 *     n_msgs) in ONE call where its first message would have gone: after the dead downstreams' drop, before
 *     the packets. A batch without messages makes no call.
 * A batch whose text or index did not fit the arena, or that could not be staged (more than SR_MAX_SLOTS
 * datagram ends in a sr_core_submit_datagrams / sr_core_route_datagrams batch), is routed as always and
 * formatted by the host as without the switch (in block mode through the log callback), so no line is lost at
 * any capacity or datagram count; a TRACE core keeps sr_set_trace on for that. sr_core_device_log_stats counts
 * the completed batches whose log came from the device and those the host formatted since the core was opened
 * (either pointer may be NULL): a host count that keeps growing says the arena is too small for the traffic. Ping lines, ERROR lines and the fault-injection paths stay host-formatted, and a batch that is taken
 * back is formatted once, when it completes. Packets, counters and their order are the same either way. Off
 * by default. Returns 0, -EINVAL, -EBUSY (a batch is in flight: drain first), -ENOMEM. */
#define SR_CORE_LOG_MAX_MSG 2047u
#define SR_CORE_LOG_DEFAULT_TEXT_CAP(max_batch_bytes) SR_LOG_DEFAULT_TEXT_CAP(max_batch_bytes)
typedef size_t (*sr_core_log_prefix_fn)(void *user, int level, char *dst, size_t cap);
typedef void (*sr_core_log_block_fn)(void *user, const char *text, size_t len, size_t n_msgs);
int sr_core_set_device_log(sr_core *core, int on, size_t text_cap, sr_core_log_prefix_fn prefix,
                           sr_core_log_block_fn block);
int sr_core_device_log_stats(const sr_core *core, uint64_t *device_batches, uint64_t *host_batches);

/* Name statistics. With sr_core_set_name_stats(core, cfg) (cfg as sr_stats_open takes it, sr_route.h: all zero
 * selects the defaults) every later batch of sr_core_route*, sr_core_submit* and sr_core_submit_slots is also
 * counted on the GPU (sr_set_name_stats): lines and bytes per verdict and shard, distinct names per shard, and
 * the names that carry the most lines. Nothing more crosses PCIe per batch, and packets, counters, log lines
 * and their order are the same with the switch on. NULL turns the switch off; the statistics stay readable.
 * sr_core_name_stats drains first, then returns the snapshot (sr_stats_read; free it with sr_stats_free) and,
 * with reset != 0, starts the statistics again from zero (sr_stats_reset).
 * What is counted: the lines of data batches. Ping lines are not (sr_core_ping routes them outside the submit
 * path). A batch that is taken back after a failed one and routed again is counted twice: the statistics see
 * every route launch, not every completed batch.
 * Return 0, -EINVAL (also: sr_core_name_stats before the switch was ever on), -EBUSY (set: a batch is in
 * flight, drain first), -ENOMEM, -EIO. */
int sr_core_set_name_stats(sr_core *core, const sr_stats_config *cfg_or_null);
int sr_core_name_stats(sr_core *core, sr_stats_snapshot **out, int reset);

/* Plain counters coalesced. With sr_core_set_coalesce(core, cfg) (cfg as sr_coalesce_open takes it, sr_route.h:
 * slots = 0 selects the default) every later batch of sr_core_route*, sr_core_submit* and sr_core_submit_slots is
 * coalesced on the GPU between the route and the packing (sr_set_coalesce): lines `<name>:<n>|c` of one name in
 * one batch leave as one line with the sum, at the place of the first of them. Other lines, their order per
 * downstream, the log lines and the name statistics are those of the switch being off; packets, traffic counters
 * and pending bytes describe the coalesced lines. Ping lines are not coalesced (sr_core_ping routes them outside
 * the submit path). NULL turns the switch off.
 * sr_core_coalesce_counts: the sums over the batches completed since the core was opened or the last reset of
 * {lines out, lines dropped, groups merged, merged text bytes}; reset != 0 starts them again from zero.
 * Return 0, -EINVAL, -EBUSY (set: a batch is in flight, drain first), -ENOMEM. */
int sr_core_set_coalesce(sr_core *core, const sr_coalesce_config *cfg_or_null);
int sr_core_coalesce_counts(sr_core *core, uint64_t totals[4], int reset);

/* Name rules. With sr_core_set_name_rules(core, cfg) (cfg as sr_rules_open takes it, sr_route.h) every later batch
 * of sr_core_route*, sr_core_submit* and sr_core_submit_slots has the lines that the set drops taken out on the
 * GPU between the route and the packing, before the coalescing when that switch is on too (sr_set_name_rules).
 * The kept lines, their order per downstream, the log lines and the name statistics are those of the switch being
 * off (a muted name stays visible among the hot names); packets, traffic counters and pending bytes describe the
 * kept lines. Ping lines are not subject to the rules (sr_core_ping routes them outside the submit path). NULL
 * turns the switch off. A new set replaces the old one and starts the hits again from zero.
 * sr_core_name_rule_hits: drains first, then copies the first min(n, n_rules + 1) pairs {lines, bytes} per rule
 * (the default's is the last, at n_rules) since the set was given or the last reset, and returns how many it
 * copied; reset != 0 starts them again from zero.
 * Return 0 (hits: the count), -EINVAL (also: hits before the switch was ever on), -EBUSY (set: a batch is in
 * flight, drain first), -ENOMEM, -EIO. */
int sr_core_set_name_rules(sr_core *core, const sr_rules_config *cfg_or_null);
int sr_core_name_rule_hits(sr_core *core, sr_rule_hits *hits, size_t n, int reset);

/* Line grammar. With sr_core_set_validate(core, cfg) (cfg as sr_validate_open takes it, sr_route.h) every later
 * batch of sr_core_route*, sr_core_submit* and sr_core_submit_slots has the lines whose reason cfg->drop_mask names
 * taken out on the GPU right after the route launch, before the name rules and the coalescing when those switches
 * are on too (sr_set_validate); with a drop_mask of 0 the lines are only counted. The kept lines, their order per
 * downstream, the log lines and the name statistics are those of the switch being off; packets, traffic counters
 * and pending bytes describe the kept lines. Ping lines are not subject (sr_core_ping routes them outside the
 * submit path). NULL turns the switch off. A new configuration starts the hits again from zero.
 * sr_core_validate_hits: drains first, then copies the first min(n, SR_VALID_REASONS) pairs {lines, bytes} per
 * reason (index 0: the OK lines) since the configuration was given or the last reset, and returns how many it
 * copied; reset != 0 starts them again from zero.
 * Return 0 (hits: the count), -EINVAL (also: hits before the switch was ever on), -EBUSY (set: a batch is in
 * flight, drain first), -ENOMEM, -EIO. */
int sr_core_set_validate(sr_core *core, const sr_validate_config *cfg_or_null);
int sr_core_validate_hits(sr_core *core, sr_validate_hits *hits, size_t n, int reset);

/* Sample rates. With sr_core_set_sample(core, cfg) (cfg as sr_sample_open takes it, sr_route.h) every later batch of
 * sr_core_route*, sr_core_submit* and sr_core_submit_slots has the names that exceed cfg->limit lines in the batch
 * thinned on the GPU, after the line grammar and the name rules and before the coalescing when those switches are on
 * too (sr_set_sample): of such a name one line in K is kept, and a kept line leaves with `|@<1/K>` inserted behind
 * its type. The first batch is thinned under cfg->seed, the next under cfg->seed + 1, and so on. The log lines and
 * the name statistics are those of the switch being off; packets, traffic counters and pending bytes describe the
 * thinned batch. A packet's line lies in the batch, in the sample text (a rewritten line) or in the merged text
 * (sr_core_set_coalesce). Ping lines are routed outside the submit path and are never sampled. NULL turns the switch
 * off. A new configuration starts the hits again from zero.
 * sr_core_sample_hits: drains first, then copies the first min(n, SR_SAMPLE_STEPS) pairs {seen, kept} per step since
 * the configuration was given or the last reset, and returns how many it copied; reset != 0 starts them again
 * from zero.
 * Return 0 (hits: the count), -EINVAL (also: hits before the switch was ever on), -EBUSY (set: a batch is in
 * flight, drain first), -ENOMEM, -EIO. */
int sr_core_set_sample(sr_core *core, const sr_sample_config *cfg_or_null);
int sr_core_sample_hits(sr_core *core, sr_sample_hits *hits, size_t n, int reset);

/* Test hook (fault injection; nothing calls it in the executable): the fail_submit-th call of
 * sr_core_submit* fails as a failed sr_route_pack_submit (the batch is not taken), and the
 * fail_finish-th batch to complete fails as a failed sr_route_pack_result (its packets and log lines
 * are lost; a batch submitted after it on device-chained fills is taken back and routed again from
 * the host's pending buffers). 0 = never. Counts start at this call. */
int sr_core_inject_faults(sr_core *core, unsigned fail_submit, unsigned fail_finish);

/* The slot whose batch is on the GPU (0 or 1), -1 if none, -EINVAL. After a failed sr_core_submit
 * it tells the caller whether the new batch was taken (the call can also fail after submitting it,
 * when completing the previous batch failed): a caller that refills the other slot only when
 * sr_core_in_flight() == slot never overwrites a batch still in flight. */
int sr_core_in_flight(const sr_core *core);

/* ds_flush_timer_cb (sr-main.c:194-204): flush every non-empty pending buffer. */
int sr_core_flush_timer(sr_core *core);

/* ping_cb (sr-main.c:206-235): per-downstream connection counters to live downstreams, traffic and
 * packet counters routed like data lines, then the healthy-downstreams gauge. */
int sr_core_ping(sr_core *core);

/* Pending (active) buffer and counters of downstream ds. */
int sr_core_state(const sr_core *core, uint32_t ds, const uint8_t **pending, size_t *len, int32_t *traffic,
                  int32_t *packets);

/* The ping metric names (sr-init.c:57,112-118): which = 0 per-downstream connections (two lines),
 * 1 traffic, 2 packets, 3 the thread's healthy-downstreams gauge (ds ignored). */
const char *sr_core_metric_name(const sr_core *core, uint32_t ds, int which);

void sr_core_close(sr_core *core);

#ifdef __cplusplus
}
#endif

#endif /* SR_ROUTER_H */
