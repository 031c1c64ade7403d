"""statsd-router_amd — MI355X-native statsd-router hot path.

Python view of the C ABI in ``include/sr_route.h`` (ctypes; the product is the C library
``lib/libsr_route.so`` built from ``csrc/sr_route.hip``). The reference has no Python API; this
module exists so tests and ``bench.py`` can drive the same C entry points a C host (the router's
``udp_read_cb`` replacement) calls. Names follow the reference's domain: datagrams, lines,
downstreams (shards), the alive bitmap.

Loading is strict: if ``libsr_route.so`` is missing or lacks a symbol, importing raises. There is
no CPU fallback of the hot path anywhere in this package.

Import with ``importlib.import_module("statsd-router_amd")`` (the directory name has a hyphen).
"""
from __future__ import annotations

import ctypes
import errno
import os
from dataclasses import dataclass
from typing import Iterable, Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
# SR_ROUTE_LIB: another build of the same library (same-box A/B runs of kernel variants, tools/ab_kernels.sh)
ROUTE_LIB = os.environ.get("SR_ROUTE_LIB") or os.path.join(LIB_DIR, "libsr_route.so")
GEN_LIB = os.path.join(LIB_DIR, "libsr_gen.so")
HEADER = os.path.join(REPO_DIR, "include", "sr_route.h")

# ---- constants mirrored from include/sr_route.h (checked against the header by tests) --------
SR_DATA_BUF_SIZE = 4096
SR_MAX_DATAGRAM = 4095
SR_DOWNSTREAM_BUF_SIZE = 1450
SR_MIN_LINE_LENGTH = 6
SR_MAX_LINE_LENGTH = 1449
SR_MAX_DOWNSTREAMS = 65533
SR_VALID, SR_INVALID_LENGTH, SR_INVALID_FORMAT, SR_ALL_DEAD = 0, 1, 2, 3
SR_ROUTE_INVALID_LENGTH = 0xFFFD
SR_ROUTE_INVALID_FORMAT = 0xFFFE
SR_ROUTE_ALL_DEAD = 0xFFFF

RECORD_DTYPE = np.dtype([("offset", "<u4"), ("length", "<u2"), ("route", "<u2")])
assert RECORD_DTYPE.itemsize == 8

# every function the header declares (tests check the library exports exactly these)
ABI_FUNCTIONS = (
    "sr_frame_datagram", "sr_frame_datagrams", "sr_open", "sr_set_alive", "sr_set_stream", "sr_set_layout",
    "sr_last_layout", "sr_last_hash_engine",
    "sr_route_batch", "sr_last_probed_dead", "sr_route_device", "sr_route_device_many", "sr_pack_by_owner",
    "sr_pack_many_by_owner", "sr_pack_packets", "sr_pack_packets_many", "sr_route_pack_batch", "sr_alloc_host", "sr_free_host", "sr_sync", "sr_close", "sr_version",
    "sr_pack_owner_sizes", "sr_pack_owner_scatter", "sr_regroup_launch",
    "sr_comm_id", "sr_comm_open", "sr_comm_close", "sr_exchange_sizes", "sr_exchange_data",
    "sr_exchange_plan", "sr_exchange_run", "sr_exchange_rebase", "sr_route_pack_submit", "sr_route_pack_result",
    "sr_set_trace", "sr_route_pack_trace", "sr_set_knob", "sr_route_pack_many", "sr_regroup_run",
    "sr_pack_payloads_many", "sr_pack_payloads", "sr_set_payloads", "sr_route_pack_payloads",
    "sr_exchange_dead_run", "sr_exchange_dead", "sr_owner_pack", "sr_flush_pending",
    "sr_comm_group_open", "sr_comm_group_close", "sr_comm_open_local", "sr_comm_set_timeout", "sr_comm_transport",
    "sr_frame_slots_size", "sr_frame_slots", "sr_route_pack_submit_slots",
    "sr_format_log", "sr_set_logtext", "sr_route_pack_set_prefix", "sr_route_pack_set_ends", "sr_route_pack_logtext",
    "sr_stats_open", "sr_stats_update", "sr_stats_reset", "sr_stats_read", "sr_stats_free", "sr_stats_close",
    "sr_name_hash", "sr_stats_estimate", "sr_stats_cardinality", "sr_stats_merge", "sr_set_name_stats",
    "sr_coalesce_open", "sr_coalesce_close", "sr_coalesce", "sr_coalesce_parse", "sr_coalesce_format",
    "sr_set_coalesce", "sr_route_pack_coalesced",
    "sr_rules_open", "sr_rules_close", "sr_rules", "sr_rules_read", "sr_rules_reset", "sr_rules_check", "sr_rules_match",
    "sr_rules_parse_text", "sr_rules_free", "sr_set_name_rules", "sr_route_pack_rules",
    "sr_validate_open", "sr_validate_close", "sr_validate", "sr_validate_read", "sr_validate_reset", "sr_validate_check",
    "sr_validate_line", "sr_validate_reason_name", "sr_validate_parse_spec", "sr_set_validate", "sr_route_pack_validate",
    "sr_sample_open", "sr_sample_close", "sr_sample", "sr_sample_read", "sr_sample_reset", "sr_sample_check",
    "sr_sample_parse", "sr_sample_step", "sr_sample_keep", "sr_sample_rate_text", "sr_sample_rewrite",
    "sr_sample_parse_spec", "sr_set_sample", "sr_route_pack_sample",
)
SR_LOG_MAX_PREFIX = 256
SR_LOG_TRACE, SR_LOG_WARN = 0, 3   # sr_log_batch.min_level and the d_levels values


def log_default_text_cap(max_batch_bytes: int) -> int:
    """SR_LOG_DEFAULT_TEXT_CAP: the slots' text arena when sr_set_logtext is given 0."""
    return max_batch_bytes * 8 + 65536


def log_max_msgs(nbytes: int, n_datagrams: int) -> int:
    """SR_LOG_MAX_MSGS: index room that always suffices."""
    return nbytes + n_datagrams


def log_text_capacity(nbytes: int, n_datagrams: int, prefix_max: int) -> int:
    """SR_LOG_TEXT_CAPACITY: text room that always suffices (the worst case is a batch of one-byte lines)."""
    return nbytes * (prefix_max + 43) + n_datagrams * (prefix_max + 25)
SR_MAX_SLOTS = 65536
SR_MAX_SLOT_STRIDE = 1 << 27
SR_MAX_PACK_DOWNSTREAMS = 4096
SR_LAYOUT_AUTO, SR_LAYOUT_UNIFORM, SR_LAYOUT_SEGMENTS, SR_LAYOUT_CHUNKS = 0, 1, 2, 3
SR_HASH_VALU, SR_HASH_MATRIX = 1, 2   # sr_last_hash_engine
SR_COMM_ID_BYTES = 128
# sr_set_knob (developer / test knobs of one context; none changes a result)
SR_KNOB_LB_SPIN, SR_KNOB_DEFER_PICKS, SR_KNOB_MTU_CHUNK, SR_KNOB_MTU_XCD, SR_KNOB_MTU_WALK = 1, 2, 3, 4, 5
SR_KNOB_HIST, SR_KNOB_PREFETCH, SR_KNOB_FUSE_DEFER = 7, 8, 9
LAYOUT_NAMES = {0: "none", 1: "uniform", 2: "segments", 3: "chunks"}
PACKET_DTYPE = np.dtype([("first", "<u4"), ("nlines", "<u2"), ("shard", "<u2"), ("length", "<u2"),
                         ("carry", "<u2"), ("open", "<u4")])
assert PACKET_DTYPE.itemsize == 16


def max_packets(nbytes: int, n_downstreams: int) -> int:
    """SR_MAX_PACKETS: descriptor room that always suffices."""
    return 2 * nbytes // 1450 + 5 * n_downstreams + 4
SR_MAX_OWNERS = 64


def pack_capacity(nbytes: int) -> int:
    """SR_PACK_CAPACITY: packed-bytes room that always suffices for a batch of nbytes."""
    return nbytes + nbytes // 2 + 4
SR_MAX_BATCHES_PER_LAUNCH = 32
PENDING_STRIDE = 1456   # SR_PENDING_STRIDE: one downstream's pending slot (1450 rounded up to 16)


def payload_capacity(nbytes: int, n_downstreams: int) -> int:
    """SR_PAYLOAD_CAPACITY: arena room that always suffices (every byte of the batch once, plus at most
    1450 pending bytes per downstream)."""
    return nbytes + SR_DOWNSTREAM_BUF_SIZE * n_downstreams


class SrBatch(ctypes.Structure):
    """struct sr_batch (include/sr_route.h): one device-resident batch of sr_route_device_many."""
    _fields_ = [
        ("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_out", ctypes.c_void_p),
        ("max_records", ctypes.c_size_t), ("d_hashes", ctypes.c_void_p), ("d_n_records", ctypes.c_void_p),
        ("d_probed_dead", ctypes.c_void_p),
    ]


class SrPackBatch(ctypes.Structure):
    """struct sr_pack_batch (include/sr_route.h): one batch of sr_pack_packets_many."""
    _fields_ = [
        ("d_recs", ctypes.c_void_p), ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t),
        ("d_fill_in", ctypes.c_void_p), ("d_probed_dead", ctypes.c_void_p), ("d_sorted", ctypes.c_void_p),
        ("d_packets", ctypes.c_void_p), ("max_packets", ctypes.c_size_t), ("d_counts", ctypes.c_void_p),
        ("d_fill_out", ctypes.c_void_p),
    ]


class SrPayloadBatch(ctypes.Structure):
    """struct sr_payload_batch (include/sr_route.h): one batch of sr_pack_payloads_many."""
    _fields_ = [
        ("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_sorted", ctypes.c_void_p),
        ("max_records", ctypes.c_size_t), ("d_packets", ctypes.c_void_p), ("max_packets", ctypes.c_size_t),
        ("d_counts", ctypes.c_void_p), ("d_fill_out", ctypes.c_void_p), ("d_pend_in", ctypes.c_void_p),
        ("d_pend_out", ctypes.c_void_p), ("d_payload", ctypes.c_void_p), ("payload_cap", ctypes.c_size_t),
        ("d_offsets", ctypes.c_void_p), ("d_total", ctypes.c_void_p),
    ]


class SrSlotBatch(ctypes.Structure):
    _fields_ = [("d_slots", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("d_lens", ctypes.c_void_p),
                ("count", ctypes.c_size_t), ("d_bytes", ctypes.c_void_p), ("cap", ctypes.c_size_t),
                ("d_ends", ctypes.c_void_p), ("d_total", ctypes.c_void_p)]


class SrLogBatch(ctypes.Structure):
    """struct sr_log_batch (include/sr_route.h): one batch of sr_format_log."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_recs", ctypes.c_void_p),
                ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t), ("d_hashes", ctypes.c_void_p),
                ("d_ends", ctypes.c_void_p), ("n_datagrams", ctypes.c_size_t), ("min_level", ctypes.c_int),
                ("d_prefix", ctypes.c_void_p), ("prefix_len", ctypes.c_uint32 * 2), ("max_msg", ctypes.c_uint32),
                ("d_text", ctypes.c_void_p), ("text_cap", ctypes.c_size_t), ("d_offsets", ctypes.c_void_p),
                ("d_levels", ctypes.c_void_p), ("max_msgs", ctypes.c_size_t), ("d_total", ctypes.c_void_p),
                ("d_n_msgs", ctypes.c_void_p)]


class SrStatsConfig(ctypes.Structure):
    """struct sr_stats_config (include/sr_route.h); all zero selects the defaults."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("hll_p", "cms_rows", "cms_width", "hot_slots", "hot_div",
                                               "hot_min_lines")]


class SrStatsBatch(ctypes.Structure):
    """struct sr_stats_batch (include/sr_route.h): one routed batch of sr_stats_update."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_recs", ctypes.c_void_p),
                ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t), ("d_hashes", ctypes.c_void_p)]


class SrStatsHot(ctypes.Structure):
    """struct sr_stats_hot (include/sr_route.h): one hot name, 128 bytes."""
    _fields_ = [("hash", ctypes.c_uint64), ("lines", ctypes.c_uint64), ("name_len", ctypes.c_uint32),
                ("name", ctypes.c_uint8 * 108)]


SR_STATS_NAME_MAX = 108
SR_STATS_ALL = 0xFFFFFFFF
SR_STATS_MAX_CELLS = 16384
SR_STATS_DEFAULTS = dict(hll_p=10, cms_rows=4, cms_width=4096, hot_slots=256, hot_div=256, hot_min_lines=1024)
STATS_TILE = 1024   # kStatsTile (csrc/stats_kernel.hpp): records per tile of the statistics kernels
STATS_LDS_SHARDS = 512   # kStatsLdsShards: per-shard sums in LDS up to this many downstreams
STATS_HOT_DTYPE = np.dtype([("hash", "<u8"), ("lines", "<u8"), ("name_len", "<u4"), ("name", "u1", (108,))])
assert STATS_HOT_DTYPE.itemsize == 128 == ctypes.sizeof(SrStatsHot)


class SrCoalesceConfig(ctypes.Structure):
    """struct sr_coalesce_config (include/sr_route.h); slots = 0 selects the default."""
    _fields_ = [("slots", ctypes.c_uint32)]


class SrCoalesceBatch(ctypes.Structure):
    """struct sr_coalesce_batch (include/sr_route.h): one routed batch of sr_coalesce."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("append_cap", ctypes.c_size_t),
                ("d_recs", ctypes.c_void_p), ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t),
                ("d_hashes", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_counts", ctypes.c_void_p)]


SR_COALESCE_NAME_MAX = 1425
SR_COALESCE_MIN_SLOTS = 16
SR_COALESCE_MAX_SLOTS = 1 << 22
SR_COALESCE_DEFAULT_SLOTS = 65536
SR_COALESCE_MAX_BYTES = 1 << 30
COALESCE_TILE = 256   # kCoalesceTile (csrc/coalesce_kernel.hpp): records per tile of the coalescing kernels


def coalesce_append_capacity(nbytes: int) -> int:
    """SR_COALESCE_APPEND_CAPACITY: room behind a batch that always holds its merged text."""
    return nbytes


def coalesce_parse(line: bytes):
    """sr_coalesce_parse on one line ('\\n' included): (name_len, value) of a plain counter, else None."""
    k, v = ctypes.c_uint32(0), ctypes.c_int64(0)
    buf = (ctypes.c_uint8 * max(len(line), 1)).from_buffer_copy(line or b"\0")
    return (int(k.value), int(v.value)) if lib().sr_coalesce_parse(buf, len(line), ctypes.byref(k), ctypes.byref(v)) \
        else None


def coalesce_format(name: bytes, total: int) -> bytes:
    """sr_coalesce_format: the merged line of `name` and the sum `total`."""
    dst = (ctypes.c_uint8 * (len(name) + 24))()
    src = (ctypes.c_uint8 * max(len(name), 1)).from_buffer_copy(name or b"\0")
    n = lib().sr_coalesce_format(dst, src, len(name), total)
    return bytes(dst[:n])


class SrRule(ctypes.Structure):
    """struct sr_rule (include/sr_route.h)."""
    _fields_ = [("pattern", ctypes.c_void_p), ("len", ctypes.c_uint32), ("kind", ctypes.c_uint8), ("action", ctypes.c_uint8)]


class SrRulesConfig(ctypes.Structure):
    """struct sr_rules_config (include/sr_route.h)."""
    _fields_ = [("rules", ctypes.POINTER(SrRule)), ("n_rules", ctypes.c_uint32), ("default_action", ctypes.c_uint32)]


class SrRulesBatch(ctypes.Structure):
    """struct sr_rules_batch (include/sr_route.h): one routed batch of sr_rules."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_recs", ctypes.c_void_p),
                ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t), ("d_out", ctypes.c_void_p),
                ("d_hashes", ctypes.c_void_p), ("d_hashes_out", ctypes.c_void_p), ("d_match", ctypes.c_void_p),
                ("d_counts", ctypes.c_void_p)]


class SrRuleHits(ctypes.Structure):
    """struct sr_rule_hits (include/sr_route.h)."""
    _fields_ = [("lines", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


SR_RULES_MAX = 256
SR_RULES_PATTERN_MAX = 64
SR_RULES_TEXT_MAX = 4096
SR_RULES_NOT_SUBJECT = 0xFFFF
SR_RULE_PREFIX, SR_RULE_EXACT = 0, 1
SR_RULE_DROP, SR_RULE_KEEP = 0, 1
RULES_TILE = 256   # kRulesTile (csrc/rules_kernel.hpp): records per tile of the rules kernels


class RuleSet:
    """A sr_rules_config and the memory it points into. `rules` is [(pattern bytes, kind, action), ...]."""

    def __init__(self, rules=(), default_action: int = SR_RULE_KEEP):
        self.rules = [(bytes(p), int(k), int(a)) for p, k, a in rules]
        self.default_action = int(default_action)
        self._keep = [(ctypes.c_uint8 * max(len(p), 1)).from_buffer_copy(p or b"\0") for p, _, _ in self.rules]
        self._arr = (SrRule * max(len(self.rules), 1))()
        for i, ((p, k, a), buf) in enumerate(zip(self.rules, self._keep)):
            self._arr[i] = SrRule(ctypes.addressof(buf), len(p), k, a)
        self.cfg = SrRulesConfig(self._arr, len(self.rules), self.default_action)

    def __len__(self):
        return len(self.rules)

    def ref(self):
        return ctypes.byref(self.cfg)

    def check(self) -> int:
        """sr_rules_check: 0 or a negative errno."""
        return int(lib().sr_rules_check(self.ref()))

    def match(self, line: bytes) -> int:
        """sr_rules_match: the winning rule's index for one line, len(self) for the default."""
        buf = (ctypes.c_uint8 * max(len(line), 1)).from_buffer_copy(line or b"\0")
        return _check(lib().sr_rules_match(self.ref(), buf, len(line)), "sr_rules_match")


def rules_parse_text(text: bytes) -> RuleSet:
    """sr_rules_parse_text: the rule file's text into a RuleSet. A bad file raises SrError with `.line` set to the
    1-based line at fault."""
    out, line = ctypes.POINTER(SrRulesConfig)(), ctypes.c_size_t(0)
    rc = lib().sr_rules_parse_text(text, len(text), ctypes.byref(out), ctypes.byref(line))
    if rc < 0:
        e = SrError(-rc, f"sr_rules_parse_text: line {line.value}: {os.strerror(-rc)}")
        e.line = int(line.value)
        raise e
    try:
        cfg = out.contents
        rules = [(ctypes.string_at(cfg.rules[i].pattern, cfg.rules[i].len), cfg.rules[i].kind, cfg.rules[i].action)
                 for i in range(cfg.n_rules)]
        return RuleSet(rules, cfg.default_action)
    finally:
        lib().sr_rules_free(out)


class SrValidateConfig(ctypes.Structure):
    """struct sr_validate_config (include/sr_route.h)."""
    _fields_ = [("drop_mask", ctypes.c_uint32), ("accept_types", ctypes.c_uint32)]


class SrValidateBatch(ctypes.Structure):
    """struct sr_validate_batch (include/sr_route.h): one routed batch of sr_validate."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("d_recs", ctypes.c_void_p),
                ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t), ("d_out", ctypes.c_void_p),
                ("d_hashes", ctypes.c_void_p), ("d_hashes_out", ctypes.c_void_p), ("d_reason", ctypes.c_void_p),
                ("d_counts", ctypes.c_void_p)]


class SrValidateHits(ctypes.Structure):
    """struct sr_validate_hits (include/sr_route.h)."""
    _fields_ = [("lines", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


(SR_VALID_OK, SR_VALID_NO_COLON, SR_VALID_EMPTY_NAME, SR_VALID_NAME_BYTE, SR_VALID_NO_TYPE, SR_VALID_TYPE, SR_VALID_VALUE,
 SR_VALID_SECTION, SR_VALID_RATE, SR_VALID_TAGS, SR_VALID_REASONS) = range(11)
SR_VALID_NOT_SUBJECT = 0xFF
SR_VALID_TYPE_C, SR_VALID_TYPE_G, SR_VALID_TYPE_MS, SR_VALID_TYPE_H, SR_VALID_TYPE_S, SR_VALID_TYPE_D = 1, 2, 4, 8, 16, 32
SR_VALID_TYPES_ALL = 63
SR_VALID_DROP_ALL = 0x3FE   # every reason but OK
VALIDATE_TILE = 256   # kValidTile (csrc/validate_kernel.hpp): records per tile of the grammar kernels


class ValidateConfig:
    """A sr_validate_config: the reasons to drop (bit r of drop_mask) and the accepted types."""

    def __init__(self, drop_mask: int = 0, accept_types: int = SR_VALID_TYPES_ALL):
        self.drop_mask, self.accept_types = int(drop_mask), int(accept_types)
        self.cfg = SrValidateConfig(self.drop_mask, self.accept_types)

    def ref(self):
        return ctypes.byref(self.cfg)

    def check(self) -> int:
        """sr_validate_check: 0 or a negative errno."""
        return int(lib().sr_validate_check(self.ref()))

    def line(self, line: bytes) -> int:
        """sr_validate_line: the reason of one line ('\n' included when it has one)."""
        buf = (ctypes.c_uint8 * max(len(line), 1)).from_buffer_copy(line or b"\0")
        return _check(lib().sr_validate_line(self.ref(), buf, len(line)), "sr_validate_line")


def validate_reason_name(reason: int):
    """sr_validate_reason_name: the reason's name, None for a number that is no reason."""
    name = lib().sr_validate_reason_name(reason)
    return name.decode() if name is not None else None


def validate_parse_spec(text: str) -> ValidateConfig:
    """sr_validate_parse_spec: `count`, `drop` or a comma list of reason names into a ValidateConfig."""
    cfg = SrValidateConfig()
    _check(lib().sr_validate_parse_spec(text.encode(), ctypes.byref(cfg)), "sr_validate_parse_spec")
    return ValidateConfig(cfg.drop_mask, cfg.accept_types)


class SrSampleConfig(ctypes.Structure):
    """struct sr_sample_config (include/sr_route.h)."""
    _fields_ = [("slots", ctypes.c_uint32), ("limit", ctypes.c_uint32), ("types", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("seed", ctypes.c_uint64)]


class SrSampleBatch(ctypes.Structure):
    """struct sr_sample_batch (include/sr_route.h): one routed batch of sr_sample."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("nbytes", ctypes.c_size_t), ("append_cap", ctypes.c_size_t),
                ("d_recs", ctypes.c_void_p), ("d_n_records", ctypes.c_void_p), ("max_records", ctypes.c_size_t),
                ("d_hashes", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_hashes_out", ctypes.c_void_p),
                ("d_step", ctypes.c_void_p), ("d_counts", ctypes.c_void_p), ("seed_add", ctypes.c_uint64)]


class SrSampleHits(ctypes.Structure):
    """struct sr_sample_hits (include/sr_route.h)."""
    _fields_ = [("seen", ctypes.c_uint64), ("kept", ctypes.c_uint64)]


SR_SAMPLE_STEPS, SR_SAMPLE_EXTRA_MAX, SR_SAMPLE_LINE_MAX = 13, 8, 1441
SR_SAMPLE_NOT_SAMPLEABLE, SR_SAMPLE_DROPPED = 0xFF, 0x80
SR_SAMPLE_DEFAULT_SLOTS, SR_SAMPLE_MIN_SLOTS, SR_SAMPLE_MAX_SLOTS = 65536, 16, 1 << 22
SR_SAMPLE_MAX_BYTES = 1 << 30
SR_SAMPLE_TYPES_ALL = SR_VALID_TYPE_C | SR_VALID_TYPE_MS | SR_VALID_TYPE_H | SR_VALID_TYPE_D
SAMPLE_TILE = 256   # kSampleTile (csrc/sample_kernel.hpp): records per tile of the sample kernels


def sample_append_capacity(nbytes: int) -> int:
    """SR_SAMPLE_APPEND_CAPACITY: room behind the batch that always suffices for records that do not overlap."""
    return nbytes + (nbytes // 6) * 8


class SampleConfig:
    """A sr_sample_config: the slots (0: the default), the limit per slot and batch, the types and the seed."""

    def __init__(self, limit: int, types: int = SR_VALID_TYPE_MS | SR_VALID_TYPE_H | SR_VALID_TYPE_D, slots: int = 0,
                 seed: int = 0, reserved: int = 0):
        self.limit, self.types, self.slots, self.seed = int(limit), int(types), int(slots), int(seed)
        self.cfg = SrSampleConfig(self.slots, self.limit, self.types, int(reserved), self.seed)

    def ref(self):
        return ctypes.byref(self.cfg)

    def check(self) -> int:
        """sr_sample_check: 0 or a negative errno."""
        return int(lib().sr_sample_check(self.ref()))


def sample_parse(line: bytes, types: int = SR_SAMPLE_TYPES_ALL):
    """sr_sample_parse: (ins, type bit) of a sampleable line ('\n' included), None for any other."""
    buf = (ctypes.c_uint8 * max(len(line), 1)).from_buffer_copy(line or b"\0")
    ins, bit = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = _check(lib().sr_sample_parse(buf, len(line), types, ctypes.byref(ins), ctypes.byref(bit)), "sr_sample_parse")
    return (ins.value, bit.value) if rc else None


def sample_step(limit: int, count: int) -> int:
    """sr_sample_step: the ladder's step for a limit and a slot's count."""
    return int(lib().sr_sample_step(limit, count))


def sample_keep(name_hash: int, seed: int, index: int, step: int) -> bool:
    """sr_sample_keep: whether record `index` of a batch is kept at `step`."""
    return bool(_check(lib().sr_sample_keep(name_hash, seed, index, step), "sr_sample_keep"))


def sample_rate_text(step: int):
    """sr_sample_rate_text: the step's rate as the rewritten line carries it, None for a number that is no step."""
    text = lib().sr_sample_rate_text(step)
    return text.decode() if text is not None else None


def sample_rewrite(line: bytes, ins: int, step: int) -> bytes:
    """sr_sample_rewrite: the line with `|@<rate>` inserted at ins (empty for step 0 or a bad argument)."""
    src = (ctypes.c_uint8 * max(len(line), 1)).from_buffer_copy(line or b"\0")
    dst = (ctypes.c_uint8 * (len(line) + SR_SAMPLE_EXTRA_MAX))()
    n = int(lib().sr_sample_rewrite(dst, src, len(line), ins, step))
    return bytes(dst[:n])


def sample_parse_spec(text: str) -> SampleConfig:
    """sr_sample_parse_spec: `<limit>` or `<limit>:<comma list of c, ms, h, d>` into a SampleConfig."""
    cfg = SrSampleConfig()
    _check(lib().sr_sample_parse_spec(text.encode(), ctypes.byref(cfg)), "sr_sample_parse_spec")
    return SampleConfig(cfg.limit, cfg.types, cfg.slots, cfg.seed)


class SrStatsSnapshot(ctypes.Structure):
    """struct sr_stats_snapshot (include/sr_route.h)."""
    _fields_ = [("cfg", SrStatsConfig), ("n_downstreams", ctypes.c_uint32), ("hot_overflow", ctypes.c_uint32),
                ("lines", ctypes.c_uint64 * 4), ("bytes", ctypes.c_uint64 * 4), ("ignored", ctypes.c_uint64),
                ("shard_lines", ctypes.c_void_p), ("shard_bytes", ctypes.c_void_p), ("regs", ctypes.c_void_p),
                ("cells", ctypes.c_void_p), ("hot", ctypes.c_void_p), ("n_hot", ctypes.c_uint32)]


class StatsSnapshot:
    """A sr_stats_snapshot in numpy arrays this object owns; `.c` is the C structure over them, for the host-only
    entry points (sr_stats_estimate, sr_stats_cardinality, sr_stats_merge). Fields: cfg (dict), n, lines[4],
    bytes[4], ignored, shard_lines[n], shard_bytes[n], regs[n, 2^p] u8, cells[rows, width] u64, hot_overflow,
    hot (STATS_HOT_DTYPE, room for hot_slots; the first n_hot are valid)."""

    def __init__(self, cfg: dict, n: int):
        self.cfg, self.n = dict(cfg), int(n)
        self.lines = np.zeros(4, np.uint64)
        self.bytes = np.zeros(4, np.uint64)
        self.ignored = 0
        self.hot_overflow = 0
        self.shard_lines = np.zeros(max(n, 1), np.uint64)[:n]
        self.shard_bytes = np.zeros(max(n, 1), np.uint64)[:n]
        self.regs = np.zeros((n, 1 << cfg["hll_p"]), np.uint8)
        self.cells = np.zeros((cfg["cms_rows"], cfg["cms_width"]), np.uint64)
        self._hot = np.zeros(cfg["hot_slots"], STATS_HOT_DTYPE)
        self.n_hot = 0
        self.c = SrStatsSnapshot()

    @property
    def hot(self) -> np.ndarray:
        return self._hot[: self.n_hot]

    def set_hot(self, entries: np.ndarray) -> None:
        self.n_hot = len(entries)
        self._hot[: self.n_hot] = entries

    def sync_c(self) -> "SrStatsSnapshot":
        """The C structure pointing at this object's arrays, scalars copied in."""
        c = self.c
        c.cfg = SrStatsConfig(**self.cfg)
        c.n_downstreams, c.hot_overflow, c.ignored, c.n_hot = self.n, int(self.hot_overflow), int(self.ignored), self.n_hot
        for v in range(4):
            c.lines[v], c.bytes[v] = int(self.lines[v]), int(self.bytes[v])
        c.shard_lines, c.shard_bytes = self.shard_lines.ctypes.data, self.shard_bytes.ctypes.data
        c.regs, c.cells, c.hot = self.regs.ctypes.data, self.cells.ctypes.data, self._hot.ctypes.data
        return c

    def from_c(self) -> None:
        """The scalars back from the C structure (after sr_stats_merge wrote through it)."""
        c = self.c
        self.hot_overflow, self.ignored, self.n_hot = int(c.hot_overflow), int(c.ignored), int(c.n_hot)
        self.lines[:] = list(c.lines)
        self.bytes[:] = list(c.bytes)

    @classmethod
    def copy_of(cls, c: "SrStatsSnapshot") -> "StatsSnapshot":
        cfg = {k: int(getattr(c.cfg, k)) for k, _ in SrStatsConfig._fields_}
        s = cls(cfg, int(c.n_downstreams))
        take = lambda addr, count, dt: (np.frombuffer(ctypes.string_at(addr, count * np.dtype(dt).itemsize), dtype=dt).copy()
                                        if count else np.zeros(0, dt))
        s.lines[:], s.bytes[:] = list(c.lines), list(c.bytes)
        s.ignored, s.hot_overflow = int(c.ignored), int(c.hot_overflow)
        s.shard_lines = take(c.shard_lines, s.n, np.uint64)
        s.shard_bytes = take(c.shard_bytes, s.n, np.uint64)
        s.regs = take(c.regs, s.n << cfg["hll_p"], np.uint8).reshape(s.n, 1 << cfg["hll_p"])
        s.cells = take(c.cells, cfg["cms_rows"] * cfg["cms_width"], np.uint64).reshape(cfg["cms_rows"], cfg["cms_width"])
        s.set_hot(take(c.hot, int(c.n_hot), STATS_HOT_DTYPE))
        return s


def name_hash(name: bytes) -> int:
    """sr_name_hash: the reference's sdbm (signed char) over the bytes of a name."""
    return int(lib().sr_name_hash(name, len(name)))


def stats_estimate(snap: StatsSnapshot, h: int) -> int:
    return int(lib().sr_stats_estimate(ctypes.byref(snap.sync_c()), h))


def stats_cardinality(snap: StatsSnapshot, shard: int = SR_STATS_ALL) -> float:
    return float(lib().sr_stats_cardinality(ctypes.byref(snap.sync_c()), shard))


def stats_merge(into: StatsSnapshot, other: StatsSnapshot) -> None:
    _check(lib().sr_stats_merge(ctypes.byref(into.sync_c()), ctypes.byref(other.sync_c())), "sr_stats_merge")
    into.from_c()


class SrOwnerBatch(ctypes.Structure):
    """struct sr_owner_batch (include/sr_route.h): one launch's receive buffer for sr_owner_pack. Device
    pointers are plain integers (None / 0 = NULL); fields left out of the constructor are zero."""
    _fields_ = [
        ("d_recv_bytes", ctypes.c_void_p), ("recv_nbytes", ctypes.c_size_t), ("d_recv_recs", ctypes.c_void_p),
        ("max_records", ctypes.c_size_t), ("d_recv_counts", ctypes.c_void_p), ("world", ctypes.c_int),
        ("d_all_dead", ctypes.c_void_p), ("d_fill_in", ctypes.c_void_p), ("d_sorted", ctypes.c_void_p),
        ("d_packets", ctypes.c_void_p), ("max_packets", ctypes.c_size_t), ("d_counts", ctypes.c_void_p),
        ("d_fill_out", ctypes.c_void_p), ("d_pend_in", ctypes.c_void_p), ("d_pend_out", ctypes.c_void_p),
        ("d_payload", ctypes.c_void_p), ("payload_cap", ctypes.c_size_t), ("d_offsets", ctypes.c_void_p),
        ("d_total", ctypes.c_void_p),
    ]


class SrPackResult(ctypes.Structure):
    """struct sr_pack_result (include/sr_route.h): the outputs of a sr_route_pack_submit slot."""
    _fields_ = [("sorted", ctypes.c_void_p), ("n_records", ctypes.c_size_t), ("n_valid", ctypes.c_size_t),
                ("packets", ctypes.c_void_p), ("n_packets", ctypes.c_size_t), ("fill", ctypes.c_void_p),
                ("probed_dead", ctypes.c_void_p)]


class SrExchangePeer(ctypes.Structure):
    """struct sr_exchange_peer (include/sr_route.h): one peer's share of an exchange plan."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("send_line0", "send_lines", "send_byte0", "send_bytes",
                                               "recv_line0", "recv_lines", "recv_byte0", "recv_bytes")]


PEER_DTYPE = np.dtype([(n, "<u8") for n, _ in SrExchangePeer._fields_])

_GROUP_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)
_SEND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                            ctypes.c_int)
_COPY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_REBASE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SrExchangePeer),
                              ctypes.c_int, ctypes.c_uint64)
_SIZES_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p)


class SrTransport(ctypes.Structure):
    """struct sr_transport (include/sr_route.h)."""
    _fields_ = [("user", ctypes.c_void_p), ("group_start", _GROUP_FN), ("group_end", _GROUP_FN),
                ("send", _SEND_FN), ("recv", _SEND_FN), ("copy", _COPY_FN), ("rebase", _REBASE_FN)]


class SrError(OSError):
    """A negative errno returned by the C ABI."""


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise SrError(-rc, f"{what}: {os.strerror(-rc)}")
    return rc


def verdicts(routes: np.ndarray) -> np.ndarray:
    """Map the record ``route`` field to sr_verdict values (sr_record_verdict in the header)."""
    r = np.asarray(routes, dtype=np.uint16)
    v = np.zeros(r.shape, dtype=np.uint8)
    bad = r >= SR_ROUTE_INVALID_LENGTH
    v[bad] = (r[bad].astype(np.int32) - 0xFFFC).astype(np.uint8)
    return v


def _load_route_lib() -> ctypes.CDLL:
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64.so.1 (same sonames as /opt/rocm's). If torch is importable, load it first
    # so libsr_route.so binds to the runtime torch already uses (a second HSA runtime in the same
    # process cannot open the GPUs).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(ROUTE_LIB):
        raise ImportError(
            f"{ROUTE_LIB} is missing: build it with __graft_entry__.build() or `make -C statsd-router_amd`"
        )
    lib = ctypes.CDLL(ROUTE_LIB)
    c_size_p = ctypes.POINTER(ctypes.c_size_t)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    vp = ctypes.c_void_p
    sig = {
        "sr_frame_datagram": (ctypes.c_size_t, [vp, vp, ctypes.c_size_t]),
        "sr_frame_datagrams": (ctypes.c_size_t, [vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t]),
        "sr_open": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32]),
        "sr_set_alive": (ctypes.c_int, [vp, u64p]),
        "sr_set_stream": (ctypes.c_int, [vp, vp]),
        "sr_set_layout": (ctypes.c_int, [vp, ctypes.c_int]),
        "sr_last_layout": (ctypes.c_int, [vp]),
        "sr_last_hash_engine": (ctypes.c_int, [vp]),
        "sr_route_batch": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, c_size_p, vp]),
        "sr_last_probed_dead": (ctypes.c_int, [vp, u64p]),
        "sr_route_device": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]),
        "sr_route_device_many": (ctypes.c_int, [vp, ctypes.POINTER(SrBatch), ctypes.c_size_t]),
        "sr_pack_by_owner": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, ctypes.c_uint32,
                                            vp, ctypes.c_size_t, vp, vp]),
        "sr_pack_many_by_owner": (ctypes.c_int, [vp, ctypes.POINTER(SrBatch), ctypes.c_size_t, ctypes.c_uint32, vp,
                                                 ctypes.c_size_t, vp, vp]),
        "sr_pack_owner_sizes": (ctypes.c_int, [vp, ctypes.POINTER(SrBatch), ctypes.c_size_t, ctypes.c_uint32, vp]),
        "sr_pack_owner_scatter": (ctypes.c_int, [vp, ctypes.POINTER(SrBatch), ctypes.c_size_t, ctypes.c_uint32,
                                                 ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]),
        "sr_pack_packets": (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t, vp, vp, vp, vp, ctypes.c_size_t, vp, vp]),
        "sr_pack_packets_many": (ctypes.c_int, [vp, ctypes.POINTER(SrPackBatch), ctypes.c_size_t]),
        "sr_route_pack_batch": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, c_size_p, c_size_p,
                                               vp, ctypes.c_size_t, c_size_p, vp]),
        "sr_alloc_host": (vp, [ctypes.c_size_t]),
        "sr_free_host": (None, [vp]),
        "sr_sync": (ctypes.c_int, [vp]),
        "sr_close": (None, [vp]),
        "sr_version": (ctypes.c_char_p, []),
        "sr_comm_id": (ctypes.c_int, [vp]),
        "sr_comm_open": (ctypes.c_int, [ctypes.POINTER(vp), vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "sr_comm_close": (None, [vp]),
        "sr_comm_group_open": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int]),
        "sr_comm_group_close": (ctypes.c_int, [vp]),
        "sr_comm_open_local": (ctypes.c_int, [ctypes.POINTER(vp), vp, ctypes.c_int, ctypes.c_int]),
        "sr_comm_set_timeout": (ctypes.c_int, [vp, ctypes.c_uint32]),
        "sr_comm_transport": (ctypes.c_int, [vp, vp, ctypes.POINTER(SrTransport)]),
        "sr_exchange_sizes": (ctypes.c_int, [vp, vp, vp, vp, vp, vp]),
        "sr_exchange_data": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "sr_exchange_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]),
        "sr_exchange_run": (ctypes.c_int, [ctypes.POINTER(SrTransport), ctypes.c_int, ctypes.c_int, vp, vp, vp, vp,
                                           vp, vp]),
        "sr_exchange_rebase": (ctypes.c_int, [vp, vp, vp, ctypes.c_int]),
        "sr_regroup_launch": (ctypes.c_int, [vp, vp, ctypes.POINTER(SrBatch), ctypes.c_size_t, vp, vp, vp,
                                             ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]),
        "sr_route_pack_submit": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_size_t, vp]),
        "sr_route_pack_result": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(SrPackResult)]),
        "sr_set_trace": (ctypes.c_int, [vp, ctypes.c_int]),
        "sr_route_pack_trace": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), c_size_p]),
        "sr_set_knob": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64]),
        "sr_route_pack_many": (ctypes.c_int, [vp, ctypes.POINTER(SrBatch), ctypes.POINTER(SrPackBatch), ctypes.c_size_t]),
        "sr_pack_payloads_many": (ctypes.c_int, [vp, ctypes.POINTER(SrPayloadBatch), ctypes.c_size_t]),
        "sr_pack_payloads": (ctypes.c_int, [vp, ctypes.POINTER(SrPayloadBatch)]),
        "sr_set_payloads": (ctypes.c_int, [vp, ctypes.c_int]),
        "sr_route_pack_payloads": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), c_size_p]),
        "sr_regroup_run": (ctypes.c_int, [vp, ctypes.POINTER(SrTransport), _SIZES_FN, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(SrBatch), ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, vp, vp,
                                          ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp]),
        "sr_exchange_dead_run": (ctypes.c_int, [vp, ctypes.POINTER(SrTransport), ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(SrBatch), ctypes.c_size_t, vp]),
        "sr_exchange_dead": (ctypes.c_int, [vp, vp, ctypes.POINTER(SrBatch), ctypes.c_size_t, vp]),
        "sr_owner_pack": (ctypes.c_int, [vp, ctypes.POINTER(SrOwnerBatch)]),
        "sr_flush_pending": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, vp]),
        "sr_frame_slots_size": (ctypes.c_size_t, [vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]),
        "sr_frame_slots": (ctypes.c_int, [vp, ctypes.POINTER(SrSlotBatch)]),
        "sr_route_pack_submit_slots": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]),
        "sr_format_log": (ctypes.c_int, [vp, ctypes.POINTER(SrLogBatch)]),
        "sr_set_logtext": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32]),
        "sr_route_pack_set_prefix": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_size_t, vp, ctypes.c_size_t]),
        "sr_route_pack_set_ends": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_size_t]),
        "sr_route_pack_logtext": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), u64p, ctypes.POINTER(vp),
                                                 ctypes.POINTER(vp), c_size_p]),
        "sr_stats_open": (ctypes.c_int, [vp, ctypes.POINTER(SrStatsConfig)]),
        "sr_stats_update": (ctypes.c_int, [vp, ctypes.POINTER(SrStatsBatch), ctypes.c_size_t]),
        "sr_stats_reset": (ctypes.c_int, [vp]),
        "sr_stats_read": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.POINTER(SrStatsSnapshot))]),
        "sr_stats_free": (None, [ctypes.POINTER(SrStatsSnapshot)]),
        "sr_stats_close": (ctypes.c_int, [vp]),
        "sr_name_hash": (ctypes.c_uint64, [ctypes.c_char_p, ctypes.c_size_t]),
        "sr_stats_estimate": (ctypes.c_uint64, [ctypes.POINTER(SrStatsSnapshot), ctypes.c_uint64]),
        "sr_stats_cardinality": (ctypes.c_double, [ctypes.POINTER(SrStatsSnapshot), ctypes.c_uint32]),
        "sr_stats_merge": (ctypes.c_int, [ctypes.POINTER(SrStatsSnapshot), ctypes.POINTER(SrStatsSnapshot)]),
        "sr_set_name_stats": (ctypes.c_int, [vp, ctypes.POINTER(SrStatsConfig)]),
        "sr_coalesce_open": (ctypes.c_int, [vp, ctypes.POINTER(SrCoalesceConfig)]),
        "sr_coalesce_close": (ctypes.c_int, [vp]),
        "sr_coalesce": (ctypes.c_int, [vp, ctypes.POINTER(SrCoalesceBatch), ctypes.c_size_t]),
        "sr_coalesce_parse": (ctypes.c_int, [vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.POINTER(ctypes.c_int64)]),
        "sr_coalesce_format": (ctypes.c_size_t, [vp, vp, ctypes.c_uint32, ctypes.c_int64]),
        "sr_set_coalesce": (ctypes.c_int, [vp, ctypes.POINTER(SrCoalesceConfig)]),
        "sr_route_pack_coalesced": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), c_size_p, u64p]),
        "sr_rules_open": (ctypes.c_int, [vp, ctypes.POINTER(SrRulesConfig)]),
        "sr_rules_close": (ctypes.c_int, [vp]),
        "sr_rules": (ctypes.c_int, [vp, ctypes.POINTER(SrRulesBatch), ctypes.c_size_t]),
        "sr_rules_read": (ctypes.c_int, [vp, ctypes.POINTER(SrRuleHits), ctypes.c_size_t]),
        "sr_rules_reset": (ctypes.c_int, [vp]),
        "sr_rules_check": (ctypes.c_int, [ctypes.POINTER(SrRulesConfig)]),
        "sr_rules_match": (ctypes.c_int, [ctypes.POINTER(SrRulesConfig), vp, ctypes.c_size_t]),
        "sr_rules_parse_text": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.POINTER(SrRulesConfig)), c_size_p]),
        "sr_rules_free": (None, [ctypes.POINTER(SrRulesConfig)]),
        "sr_set_name_rules": (ctypes.c_int, [vp, ctypes.POINTER(SrRulesConfig)]),
        "sr_route_pack_rules": (ctypes.c_int, [vp, ctypes.c_int, u64p]),
        "sr_validate_open": (ctypes.c_int, [vp, ctypes.POINTER(SrValidateConfig)]),
        "sr_validate_close": (ctypes.c_int, [vp]),
        "sr_validate": (ctypes.c_int, [vp, ctypes.POINTER(SrValidateBatch), ctypes.c_size_t]),
        "sr_validate_read": (ctypes.c_int, [vp, ctypes.POINTER(SrValidateHits), ctypes.c_size_t]),
        "sr_validate_reset": (ctypes.c_int, [vp]),
        "sr_validate_check": (ctypes.c_int, [ctypes.POINTER(SrValidateConfig)]),
        "sr_validate_line": (ctypes.c_int, [ctypes.POINTER(SrValidateConfig), vp, ctypes.c_size_t]),
        "sr_validate_reason_name": (ctypes.c_char_p, [ctypes.c_uint32]),
        "sr_validate_parse_spec": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(SrValidateConfig)]),
        "sr_set_validate": (ctypes.c_int, [vp, ctypes.POINTER(SrValidateConfig)]),
        "sr_route_pack_validate": (ctypes.c_int, [vp, ctypes.c_int, u64p]),
        "sr_sample_open": (ctypes.c_int, [vp, ctypes.POINTER(SrSampleConfig)]),
        "sr_sample_close": (ctypes.c_int, [vp]),
        "sr_sample": (ctypes.c_int, [vp, ctypes.POINTER(SrSampleBatch), ctypes.c_size_t]),
        "sr_sample_read": (ctypes.c_int, [vp, ctypes.POINTER(SrSampleHits), ctypes.c_size_t]),
        "sr_sample_reset": (ctypes.c_int, [vp]),
        "sr_sample_check": (ctypes.c_int, [ctypes.POINTER(SrSampleConfig)]),
        "sr_sample_parse": (ctypes.c_int, [vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32)]),
        "sr_sample_step": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint64]),
        "sr_sample_keep": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]),
        "sr_sample_rate_text": (ctypes.c_char_p, [ctypes.c_uint32]),
        "sr_sample_rewrite": (ctypes.c_size_t, [vp, vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]),
        "sr_sample_parse_spec": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(SrSampleConfig)]),
        "sr_set_sample": (ctypes.c_int, [vp, ctypes.POINTER(SrSampleConfig)]),
        "sr_route_pack_sample": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(vp), c_size_p, u64p, u64p]),
    }
    for name in ABI_FUNCTIONS:
        if os.environ.get("SR_ROUTE_LIB") and not hasattr(lib, name):
            continue   # an older build under A/B (SR_ROUTE_LIB) may lack entry points added since
        fn = getattr(lib, name)  # raises AttributeError if the export is missing
        fn.restype, fn.argtypes = sig[name]
    return lib


_LIB: ctypes.CDLL | None = None
_GEN: ctypes.CDLL | None = None


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = _load_route_lib()
    return _LIB


def gen_lib() -> ctypes.CDLL:
    global _GEN
    if _GEN is None:
        if not os.path.exists(GEN_LIB):
            raise ImportError(f"{GEN_LIB} is missing: build with __graft_entry__.build()")
        g = ctypes.CDLL(GEN_LIB)
        g.sr_gen_stream.restype = ctypes.c_size_t
        g.sr_gen_stream.argtypes = [
            ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double,
            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
        ]
        _GEN = g
    return _GEN


# ---- framing (host, no GPU) -----------------------------------------------------------------
def frame_datagrams(dgrams: Sequence[bytes]) -> bytes:
    """Frame datagrams as udp_read_cb does (sr-main.c:163-173) and concatenate them."""
    L = lib()
    cap = sum(min(len(d), SR_MAX_DATAGRAM) + 1 for d in dgrams)
    out = ctypes.create_string_buffer(max(cap, 1))
    bufs = [ctypes.create_string_buffer(bytes(d), max(len(d), 1)) for d in dgrams]
    ptrs = (ctypes.c_void_p * max(len(dgrams), 1))(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * max(len(dgrams), 1))(*[len(d) for d in dgrams])
    n = L.sr_frame_datagrams(out, cap, ptrs, lens, len(dgrams))
    if n == ctypes.c_size_t(-1).value:
        raise SrError(errno.ENOSPC, "sr_frame_datagrams")
    return out.raw[:n]


def frame_slots_size(slots: np.ndarray, stride: int, lens, want_ends: bool = False):
    """sr_frame_slots_size: the framed size of datagrams left in their slots (datagram j = lens[j] bytes at
    slots[j * stride:]), one byte looked at per datagram. Returns the total, or (total, ends u32 [count])."""
    buf = np.ascontiguousarray(slots, dtype=np.uint8)
    ln = np.ascontiguousarray(lens, dtype=np.uint16)
    if ln.size and int(ln.size - 1) * stride + min(int(ln[-1]), SR_MAX_DATAGRAM) > buf.size:
        raise ValueError("the slots are shorter than (count - 1) * stride + the last datagram")
    ends = np.zeros(max(ln.size, 1), dtype=np.uint32)
    total = lib().sr_frame_slots_size(buf.ctypes.data if buf.size else None, stride, ln.ctypes.data if ln.size else None,
                                      int(ln.size), ends.ctypes.data if want_ends else None)
    return (int(total), ends[: ln.size]) if want_ends else int(total)


class HostBuffer:
    """Page-locked host memory from sr_alloc_host as a numpy uint8 array (`.array`); the device reads it in
    place (Router.route_pack_submit_slots). Freed by close() or with the object."""

    def __init__(self, nbytes: int):
        self._lib = lib()
        self.nbytes = int(nbytes)
        self.addr = self._lib.sr_alloc_host(self.nbytes)
        if not self.addr:
            raise SrError(errno.ENOMEM, "sr_alloc_host")
        self.array = np.frombuffer((ctypes.c_uint8 * max(self.nbytes, 1)).from_address(self.addr), dtype=np.uint8)

    def close(self) -> None:
        if self.addr:
            self.array = None
            self._lib.sr_free_host(ctypes.c_void_p(self.addr))
            self.addr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- synthetic traffic ------------------------------------------------------------------------
GEN_FIXED, GEN_TEST_SHAPE = 0, 1


@dataclass
class Stream:
    data: np.ndarray          # uint8, concatenated framed datagrams
    dgram_lens: np.ndarray    # uint32
    n_lines: int


def gen_stream(nbytes: int, line_lens: Iterable[int], seed: int, p_invalid: float = 0.0,
               kind: int = GEN_FIXED, max_dgram: int = SR_MAX_DATAGRAM) -> Stream:
    """Seeded synthetic stream (statsd-router_amd/csrc/sr_gen.c) of at most nbytes bytes."""
    g = gen_lib()
    lens = np.ascontiguousarray(np.array(list(line_lens), dtype=np.uint32))
    out = np.zeros(max(nbytes, 1), dtype=np.uint8)
    dcap = nbytes // 6 + 2
    dl = np.zeros(dcap, dtype=np.uint32)
    nd, nl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    n = g.sr_gen_stream(seed, kind, lens.ctypes.data, len(lens), float(p_invalid), max_dgram,
                        out.ctypes.data, nbytes, dl.ctypes.data, dcap, ctypes.byref(nd), ctypes.byref(nl))
    return Stream(out[:n], dl[: min(nd.value, dcap)].copy(), nl.value)


def bitmap_shards(words, n: int) -> np.ndarray:
    """Shard ids whose bit is set in a ceil(n/64)-word bitmap."""
    w = np.asarray(words, dtype=np.uint64)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:n]
    return np.nonzero(bits)[0]


# ---- the router context -------------------------------------------------------------------------
def alive_words(n_downstreams: int, alive: Iterable[int] | np.ndarray | None) -> np.ndarray:
    """Bitmap words from a 0/1 sequence (None = all alive)."""
    nw = max((n_downstreams + 63) // 64, 1)
    w = np.zeros(nw, dtype=np.uint64)
    bits = np.ones(n_downstreams, dtype=bool) if alive is None else np.asarray(list(alive), dtype=bool)
    for k in np.nonzero(bits)[0]:
        w[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
    return w


class Router:
    """One sr_ctx: a HIP stream's worth of routing state on one GPU (sr_open .. sr_close)."""

    def __init__(self, n_downstreams: int, max_batch_bytes: int, device: int = 0):
        self._lib = lib()
        self.n_downstreams = n_downstreams
        self.max_batch_bytes = max_batch_bytes
        self.device = device
        h = ctypes.c_void_p()
        _check(self._lib.sr_open(ctypes.byref(h), device, max_batch_bytes, n_downstreams), "sr_open")
        self._h = h

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def close(self) -> None:
        if self._h:
            self._lib.sr_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_alive(self, alive) -> None:
        """alive: 0/1 per downstream, or a uint64 word array."""
        a = np.asarray(alive)
        w = a.astype(np.uint64) if a.dtype == np.uint64 else alive_words(self.n_downstreams, alive)
        w = np.ascontiguousarray(w)
        _check(self._lib.sr_set_alive(self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "sr_set_alive")

    def set_stream(self, stream_handle: int | None) -> None:
        """Launch on this HIP stream from now on. 0/None = the context's own non-blocking stream
        (sr_set_stream's NULL), which is NOT the HIP null stream: work on torch's default stream
        is not ordered with it."""
        _check(self._lib.sr_set_stream(self._h, ctypes.c_void_p(stream_handle or 0)), "sr_set_stream")
        self.stream_handle = int(stream_handle or 0)

    def set_layout(self, layout: int) -> None:
        """sr_set_layout: SR_LAYOUT_AUTO (default), SR_LAYOUT_UNIFORM, SR_LAYOUT_SEGMENTS or
        SR_LAYOUT_CHUNKS (the route kernel's lane layout; records are identical either way)."""
        _check(self._lib.sr_set_layout(self._h, int(layout)), "sr_set_layout")

    def set_knob(self, knob: int, value: int) -> None:
        """sr_set_knob: a developer / test knob of this context (SR_KNOB_*); results never change."""
        _check(self._lib.sr_set_knob(self._h, int(knob), int(value)), "sr_set_knob")

    def set_trace(self, on: bool = True) -> None:
        """sr_set_trace: later route + pack submissions also return input-order records and hashes."""
        _check(self._lib.sr_set_trace(self._h, 1 if on else 0), "sr_set_trace")

    def route_pack_trace(self, slot: int):
        """sr_route_pack_trace after route_pack_result(slot) (slot 2: the last route_pack): (records in
        input order, per-line hashes), copied."""
        r, h, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(self._lib.sr_route_pack_trace(self._h, slot, ctypes.byref(r), ctypes.byref(h), ctypes.byref(n)),
               "sr_route_pack_trace")
        k = n.value
        if not k:
            return np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint64)
        recs = np.frombuffer((ctypes.c_uint8 * (8 * k)).from_address(r.value), dtype=RECORD_DTYPE).copy()
        hs = np.frombuffer((ctypes.c_uint8 * (8 * k)).from_address(h.value), dtype=np.uint64).copy()
        return recs, hs

    def set_payloads(self, on: bool = True) -> None:
        """sr_set_payloads: later route + pack submissions also gather the packets' bytes (room left for
        each packet's carry) into the slot's page-locked memory."""
        _check(self._lib.sr_set_payloads(self._h, 1 if on else 0), "sr_set_payloads")

    def route_pack_payloads(self, slot: int):
        """sr_route_pack_payloads after route_pack_result(slot) (slot 2: the last route_pack): (arena bytes
        [offsets[-1]], offsets u32 [n_packets + 1]), copied."""
        a, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(self._lib.sr_route_pack_payloads(self._h, slot, ctypes.byref(a), ctypes.byref(o), ctypes.byref(n)),
               "sr_route_pack_payloads")
        offs = np.frombuffer((ctypes.c_uint8 * (4 * (n.value + 1))).from_address(o.value), dtype=np.uint32).copy()
        total = int(offs[-1])
        arena = (np.frombuffer((ctypes.c_uint8 * total).from_address(a.value), dtype=np.uint8).copy() if total
                 else np.zeros(0, np.uint8))
        return arena, offs

    @staticmethod
    def payload_batches(batches):
        """The sr_payload_batch array of [(d_bytes, nbytes, d_sorted, max_records, d_packets, max_packets,
        d_counts, d_fill_out, d_pend_in, d_pend_out, d_payload, payload_cap, d_offsets, d_total), ...]
        (raw device pointers, 0 = NULL; reusable)."""
        arr = (SrPayloadBatch * max(len(batches), 1))()
        for i, b in enumerate(batches):
            arr[i] = SrPayloadBatch(*[x if j in (1, 3, 5, 11) else (x or None) for j, x in enumerate(b)])
        return arr

    def pack_payloads_many(self, batches) -> None:
        """sr_pack_payloads_many: the packets' bytes of packed batches (batches as payload_batches takes
        them, or its array), asynchronous on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.payload_batches(batches)
        _check(self._lib.sr_pack_payloads_many(self._h, arr, len(batches)), "sr_pack_payloads_many")

    def pack_payloads(self, batch) -> None:
        """sr_pack_payloads: pack_payloads_many for one batch (a tuple as payload_batches takes them)."""
        arr = self.payload_batches([batch])
        _check(self._lib.sr_pack_payloads(self._h, arr), "sr_pack_payloads")

    def last_layout(self) -> int:
        """sr_last_layout: the lane layout of the context's last route launch (1 uniform, 2 segments,
        3 chunks)."""
        return _check(self._lib.sr_last_layout(self._h), "sr_last_layout")

    def last_hash_engine(self) -> int:
        """sr_last_hash_engine: where the last route launch hashed names (SR_HASH_VALU = 1: vector ALU,
        SR_HASH_MATRIX = 2: matrix cores; 0 before the first launch)."""
        return _check(self._lib.sr_last_hash_engine(self._h), "sr_last_hash_engine")

    def route(self, data: bytes | np.ndarray, max_records: int | None = None, want_hashes: bool = False):
        """sr_route_batch on host memory. Returns (records[n] structured array, hashes or None, n)."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        nbytes = int(buf.size)
        cap = nbytes if max_records is None else max_records
        out = np.zeros(max(cap, 1), dtype=RECORD_DTYPE)
        hashes = np.zeros(max(cap, 1), dtype=np.uint64) if want_hashes else None
        n = ctypes.c_size_t(0)
        rc = self._lib.sr_route_batch(self._h, buf.ctypes.data if nbytes else None, nbytes, out.ctypes.data,
                                      cap, ctypes.byref(n), hashes.ctypes.data if want_hashes else None)
        if rc not in (0, -errno.ENOSPC):
            _check(rc, "sr_route_batch")
        k = min(n.value, cap)
        return out[:k], (hashes[:k] if want_hashes else None), n.value

    def last_probed_dead(self) -> np.ndarray:
        """sr_last_probed_dead: the dead downstreams probed by the last route() (sr-main.c:106) as
        a sorted array of shard ids."""
        nw = max((self.n_downstreams + 63) // 64, 1)
        w = np.zeros(nw, dtype=np.uint64)
        _check(self._lib.sr_last_probed_dead(self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
               "sr_last_probed_dead")
        return bitmap_shards(w, self.n_downstreams)

    def route_device(self, d_bytes: int, nbytes: int, d_out: int, max_records: int,
                     d_hashes: int | None, d_count: int) -> None:
        """sr_route_device with raw device pointers (e.g. torch tensors' data_ptr())."""
        _check(self._lib.sr_route_device(self._h, ctypes.c_void_p(d_bytes), nbytes, ctypes.c_void_p(d_out),
                                         max_records, ctypes.c_void_p(d_hashes or 0), ctypes.c_void_p(d_count)),
               "sr_route_device")

    def route_device_many(self, batches) -> None:
        """sr_route_device_many: batches = [(d_bytes, nbytes, d_out, max_records, d_hashes, d_count
        [, d_probed_dead]), ...]."""
        arr = (SrBatch * max(len(batches), 1))()
        for i, b in enumerate(batches):
            db, nb, do, mr, dh, dc = b[:6]
            dp = b[6] if len(b) > 6 else None
            arr[i] = SrBatch(db, nb, do, mr, dh or None, dc, dp or None)
        _check(self._lib.sr_route_device_many(self._h, arr, len(batches)), "sr_route_device_many")

    def pack_by_owner(self, d_bytes: int, nbytes: int, d_recs: int, d_n_records: int, max_records: int,
                      n_owners: int, d_out_bytes: int, out_cap: int, d_out_recs: int, d_owner_counts: int) -> None:
        """sr_pack_by_owner with raw device pointers (asynchronous on the context's stream)."""
        vp = ctypes.c_void_p
        _check(self._lib.sr_pack_by_owner(self._h, vp(d_bytes), nbytes, vp(d_recs), vp(d_n_records), max_records,
                                          n_owners, vp(d_out_bytes), out_cap, vp(d_out_recs), vp(d_owner_counts)),
               "sr_pack_by_owner")

    def route_pack(self, data, fill=None):
        """sr_route_pack_batch on host memory: route + per-downstream MTU packing. fill: pending
        bytes per downstream before the batch (None = 0). Returns (sorted records, packets,
        fill after, n_valid, probed-dead shard ids)."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        nbytes, n = int(buf.size), self.n_downstreams
        f = np.zeros(max(n, 1), dtype=np.uint16)
        if fill is not None:
            f[:n] = np.asarray(fill, dtype=np.uint16)
        srt = np.zeros(max(nbytes, 1), dtype=RECORD_DTYPE)
        mp = max_packets(nbytes, n)
        pk = np.zeros(mp, dtype=PACKET_DTYPE)
        pw = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        nr, nv, npk = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _check(self._lib.sr_route_pack_batch(self._h, buf.ctypes.data if nbytes else None, nbytes, f.ctypes.data,
                                             srt.ctypes.data, srt.size, ctypes.byref(nr), ctypes.byref(nv),
                                             pk.ctypes.data, mp, ctypes.byref(npk), pw.ctypes.data),
               "sr_route_pack_batch")
        return srt[: nr.value], pk[: npk.value], f[:n].copy(), nv.value, bitmap_shards(pw, n)

    def route_pack_submit(self, slot: int, data, fill=None) -> None:
        """sr_route_pack_submit (asynchronous). data must stay alive and unchanged until
        route_pack_result(slot): keep a reference (e.g. a pinned or numpy buffer). fill None = chain
        from the previous submission's pending bytes on the device."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        f = None
        if fill is not None:
            f = np.zeros(max(self.n_downstreams, 1), dtype=np.uint16)
            f[: self.n_downstreams] = np.asarray(fill, dtype=np.uint16)
        self._pending = getattr(self, "_pending", {})
        self._pending[slot] = buf
        _check(self._lib.sr_route_pack_submit(self._h, slot, buf.ctypes.data if buf.size else None, int(buf.size),
                                              f.ctypes.data if f is not None else None), "sr_route_pack_submit")

    def frame_slots(self, d_slots: int, stride: int, d_lens: int, count: int, d_bytes: int, cap: int,
                    d_ends: int | None, d_total: int) -> None:
        """sr_frame_slots with raw device pointers (0 / None = NULL): datagrams framed on the device from
        their slots, asynchronous on the context's stream."""
        b = SrSlotBatch(d_slots or None, stride, d_lens or None, count, d_bytes or None, cap, d_ends or None,
                        d_total or None)
        _check(self._lib.sr_frame_slots(self._h, ctypes.byref(b)), "sr_frame_slots")

    def set_logtext(self, min_level: int | None, text_cap: int = 0, max_msg: int = 0) -> None:
        """sr_set_logtext: later route_pack submissions also format the batch's log text at min_level
        (SR_LOG_TRACE or SR_LOG_WARN); None turns it off."""
        _check(self._lib.sr_set_logtext(self._h, -1 if min_level is None else min_level, text_cap, max_msg),
               "sr_set_logtext")
        self._log_cap = text_cap or log_default_text_cap(self.max_batch_bytes)

    def route_pack_set_prefix(self, slot: int, trace: bytes = b"", warn: bytes = b"") -> None:
        """sr_route_pack_set_prefix: the TRACE and WARN prefixes of the slot's next submission."""
        _check(self._lib.sr_route_pack_set_prefix(self._h, slot, trace or None, len(trace), warn or None, len(warn)),
               "sr_route_pack_set_prefix")

    def route_pack_set_ends(self, slot: int, ends) -> None:
        """sr_route_pack_set_ends: the framed datagram ends of the slot's next submission."""
        e = np.ascontiguousarray(ends, dtype=np.uint32)
        _check(self._lib.sr_route_pack_set_ends(self._h, slot, e.ctypes.data if e.size else None, int(e.size)),
               "sr_route_pack_set_ends")

    def route_pack_logtext(self, slot: int):
        """sr_route_pack_logtext after route_pack_result(slot): (text bytes, total, offsets, levels, complete),
        copied out of the slot; text holds min(total, the arena's size) bytes when incomplete."""
        text, offs, lv = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        total, n = ctypes.c_uint64(), ctypes.c_size_t()
        rc = self._lib.sr_route_pack_logtext(self._h, slot, ctypes.byref(text), ctypes.byref(total), ctypes.byref(offs),
                                             ctypes.byref(lv), ctypes.byref(n))
        if rc != -errno.ENOSPC:
            _check(rc, "sr_route_pack_logtext")
        k = n.value
        offsets = np.frombuffer(ctypes.string_at(offs.value, 4 * (k + 1)), dtype=np.uint32).copy()
        levels = np.frombuffer(ctypes.string_at(lv.value, k), dtype=np.uint8).copy()
        return ctypes.string_at(text.value, min(total.value, self._log_cap)), total.value, offsets, levels, rc == 0

    def format_log(self, batch: SrLogBatch | None = None, **fields) -> None:
        """sr_format_log with raw device pointers (0 / None = NULL): a routed batch's log text written on the
        device, asynchronous on the context's stream. Fields as struct sr_log_batch; prefix_len is a pair
        (TRACE bytes, WARN bytes). Tensors pass their data_ptr()."""
        if batch is None:
            plen = fields.pop("prefix_len", (0, 0))
            batch = SrLogBatch(**{k: (v or None) if k.startswith("d_") else v for k, v in fields.items()})
            batch.prefix_len[0], batch.prefix_len[1] = int(plen[0]), int(plen[1])
        _check(self._lib.sr_format_log(self._h, ctypes.byref(batch)), "sr_format_log")

    def stats_open(self, **cfg) -> None:
        """sr_stats_open: the name statistics of this context (fields of sr_stats_config; none = the defaults)."""
        _check(self._lib.sr_stats_open(self._h, ctypes.byref(SrStatsConfig(**cfg))), "sr_stats_open")

    @staticmethod
    def stats_batches(batches):
        """The sr_stats_batch array of [(d_bytes, nbytes, d_recs, d_n_records, max_records, d_hashes), ...] (raw
        device pointers, 0 = NULL; reusable)."""
        arr = (SrStatsBatch * max(len(batches), 1))()
        for i, (db, nb, dr, dn, mr, dh) in enumerate(batches):
            arr[i] = SrStatsBatch(db or None, nb, dr or None, dn or None, mr, dh or None)
        return arr

    def stats_update(self, batches) -> None:
        """sr_stats_update over the batches of one route launch (as stats_batches takes them, or its array),
        asynchronous on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.stats_batches(batches)
        _check(self._lib.sr_stats_update(self._h, arr, len(batches)), "sr_stats_update")

    def stats_reset(self) -> None:
        _check(self._lib.sr_stats_reset(self._h), "sr_stats_reset")

    def stats_close(self) -> None:
        _check(self._lib.sr_stats_close(self._h), "sr_stats_close")

    def stats_read(self) -> StatsSnapshot:
        """sr_stats_read: waits for the stream and returns a copy of the snapshot."""
        p = ctypes.POINTER(SrStatsSnapshot)()
        _check(self._lib.sr_stats_read(self._h, ctypes.byref(p)), "sr_stats_read")
        try:
            return StatsSnapshot.copy_of(p.contents)
        finally:
            self._lib.sr_stats_free(p)

    def set_name_stats(self, on: bool = True, **cfg) -> None:
        """sr_set_name_stats: later route_pack submissions also update the name statistics on the device."""
        _check(self._lib.sr_set_name_stats(self._h, ctypes.byref(SrStatsConfig(**cfg)) if on else None),
               "sr_set_name_stats")

    def coalesce_open(self, slots: int = 0) -> None:
        """sr_coalesce_open: the coalescing stage of this context (slots = 0: the default table size)."""
        _check(self._lib.sr_coalesce_open(self._h, ctypes.byref(SrCoalesceConfig(slots))), "sr_coalesce_open")

    def coalesce_close(self) -> None:
        _check(self._lib.sr_coalesce_close(self._h), "sr_coalesce_close")

    @staticmethod
    def coalesce_batches(batches):
        """The sr_coalesce_batch array of [(d_bytes, nbytes, append_cap, d_recs, d_n_records, max_records, d_hashes,
        d_out, d_counts), ...] (raw device addresses; 0 = NULL)."""
        arr = (SrCoalesceBatch * max(len(batches), 1))()
        for i, (db, nb, cap, dr, dn, mr, dh, do, dc) in enumerate(batches):
            arr[i] = SrCoalesceBatch(db or None, nb, cap, dr or None, dn or None, mr, dh or None, do or None, dc or None)
        return arr

    def coalesce(self, batches) -> None:
        """sr_coalesce over the batches of one route launch (as coalesce_batches takes them, or its array),
        asynchronous on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.coalesce_batches(batches)
        _check(self._lib.sr_coalesce(self._h, arr, len(batches)), "sr_coalesce")

    def set_coalesce(self, on: bool = True, slots: int = 0) -> None:
        """sr_set_coalesce: later route_pack submissions coalesce plain counters between the route and the
        packing."""
        _check(self._lib.sr_set_coalesce(self._h, ctypes.byref(SrCoalesceConfig(slots)) if on else None),
               "sr_set_coalesce")

    def route_pack_coalesced(self, slot: int):
        """sr_route_pack_coalesced after route_pack_result(slot) (route_pack: slot 2): (merged text, counts[4])."""
        text, n = ctypes.c_void_p(), ctypes.c_size_t()
        counts = (ctypes.c_uint64 * 4)()
        _check(self._lib.sr_route_pack_coalesced(self._h, slot, ctypes.byref(text), ctypes.byref(n), counts),
               "sr_route_pack_coalesced")
        raw = bytes((ctypes.c_uint8 * n.value).from_address(text.value)) if n.value else b""
        return raw, np.array(list(counts), np.uint64)

    def rules_open(self, rules: RuleSet) -> None:
        """sr_rules_open: the name rules' stage of this context, with the compiled set uploaded."""
        _check(self._lib.sr_rules_open(self._h, rules.ref()), "sr_rules_open")
        self._n_rules = len(rules)

    def rules_close(self) -> None:
        _check(self._lib.sr_rules_close(self._h), "sr_rules_close")

    @staticmethod
    def rules_batches(batches):
        """The sr_rules_batch array of [(d_bytes, nbytes, d_recs, d_n_records, max_records, d_out, d_hashes,
        d_hashes_out, d_match, d_counts), ...] (raw device addresses; 0 = NULL)."""
        arr = (SrRulesBatch * max(len(batches), 1))()
        for i, (db, nb, dr, dn, mr, do, dh, dho, dm, dc) in enumerate(batches):
            arr[i] = SrRulesBatch(db or None, nb, dr or None, dn or None, mr, do or None, dh or None, dho or None,
                                  dm or None, dc or None)
        return arr

    def rules(self, batches) -> None:
        """sr_rules over the batches of one route launch (as rules_batches takes them, or its array), asynchronous
        on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.rules_batches(batches)
        _check(self._lib.sr_rules(self._h, arr, len(batches)), "sr_rules")

    def rules_read(self, n: int | None = None) -> np.ndarray:
        """sr_rules_read: the hits as an array of [lines, bytes] rows, one per rule and the default's last."""
        n = SR_RULES_MAX + 1 if n is None else n
        hits = (SrRuleHits * max(n, 1))()
        m = _check(self._lib.sr_rules_read(self._h, hits, n), "sr_rules_read")
        return np.array([[hits[i].lines, hits[i].bytes] for i in range(m)], np.uint64).reshape(m, 2)

    def rules_reset(self) -> None:
        _check(self._lib.sr_rules_reset(self._h), "sr_rules_reset")

    def set_name_rules(self, rules: RuleSet | None) -> None:
        """sr_set_name_rules: later route_pack submissions drop the lines that the set drops, between the route and
        the packing (None: off)."""
        _check(self._lib.sr_set_name_rules(self._h, rules.ref() if rules is not None else None), "sr_set_name_rules")

    def route_pack_rules(self, slot: int) -> np.ndarray:
        """sr_route_pack_rules after route_pack_result(slot) (route_pack: slot 2): [out, dropped, bytes dropped,
        subject]."""
        counts = (ctypes.c_uint64 * 4)()
        _check(self._lib.sr_route_pack_rules(self._h, slot, counts), "sr_route_pack_rules")
        return np.array(list(counts), np.uint64)

    def validate_open(self, cfg: ValidateConfig) -> None:
        """sr_validate_open: the line grammar's stage of this context."""
        _check(self._lib.sr_validate_open(self._h, cfg.ref()), "sr_validate_open")

    def validate_close(self) -> None:
        _check(self._lib.sr_validate_close(self._h), "sr_validate_close")

    @staticmethod
    def validate_batches(batches):
        """The sr_validate_batch array of [(d_bytes, nbytes, d_recs, d_n_records, max_records, d_out, d_hashes,
        d_hashes_out, d_reason, d_counts), ...] (raw device addresses; 0 = NULL)."""
        arr = (SrValidateBatch * max(len(batches), 1))()
        for i, (db, nb, dr, dn, mr, do, dh, dho, dm, dc) in enumerate(batches):
            arr[i] = SrValidateBatch(db or None, nb, dr or None, dn or None, mr, do or None, dh or None, dho or None,
                                     dm or None, dc or None)
        return arr

    def validate(self, batches) -> None:
        """sr_validate over the batches of one route launch (as validate_batches takes them, or its array),
        asynchronous on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.validate_batches(batches)
        _check(self._lib.sr_validate(self._h, arr, len(batches)), "sr_validate")

    def validate_read(self, n: int | None = None) -> np.ndarray:
        """sr_validate_read: the hits as an array of [lines, bytes] rows, one per reason (row 0: the OK lines)."""
        n = SR_VALID_REASONS if n is None else n
        hits = (SrValidateHits * max(n, 1))()
        m = _check(self._lib.sr_validate_read(self._h, hits, n), "sr_validate_read")
        return np.array([[hits[i].lines, hits[i].bytes] for i in range(m)], np.uint64).reshape(m, 2)

    def validate_reset(self) -> None:
        _check(self._lib.sr_validate_reset(self._h), "sr_validate_reset")

    def set_validate(self, cfg: ValidateConfig | None) -> None:
        """sr_set_validate: later route_pack submissions drop the lines whose reason the configuration drops,
        between the route and the name rules (None: off)."""
        _check(self._lib.sr_set_validate(self._h, cfg.ref() if cfg is not None else None), "sr_set_validate")

    def route_pack_validate(self, slot: int) -> np.ndarray:
        """sr_route_pack_validate after route_pack_result(slot) (route_pack: slot 2): [out, dropped, bytes dropped,
        subject]."""
        counts = (ctypes.c_uint64 * 4)()
        _check(self._lib.sr_route_pack_validate(self._h, slot, counts), "sr_route_pack_validate")
        return np.array(list(counts), np.uint64)

    def sample_open(self, cfg: SampleConfig) -> None:
        """sr_sample_open: the sample-rate stage of this context."""
        _check(self._lib.sr_sample_open(self._h, cfg.ref()), "sr_sample_open")

    def sample_close(self) -> None:
        _check(self._lib.sr_sample_close(self._h), "sr_sample_close")

    @staticmethod
    def sample_batches(batches):
        """The sr_sample_batch array of [(d_bytes, nbytes, append_cap, d_recs, d_n_records, max_records, d_hashes,
        d_out, d_hashes_out, d_step, d_counts, seed_add), ...] (raw device addresses; 0 = NULL)."""
        arr = (SrSampleBatch * max(len(batches), 1))()
        for i, (db, nb, cap, dr, dn, mr, dh, do, dho, dst, dc, sa) in enumerate(batches):
            arr[i] = SrSampleBatch(db or None, nb, cap, dr or None, dn or None, mr, dh or None, do or None, dho or None,
                                   dst or None, dc or None, sa)
        return arr

    def sample(self, batches) -> None:
        """sr_sample over the batches of one route launch (as sample_batches takes them, or its array),
        asynchronous on the context's stream."""
        arr = batches if isinstance(batches, ctypes.Array) else self.sample_batches(batches)
        _check(self._lib.sr_sample(self._h, arr, len(batches)), "sr_sample")

    def sample_read(self, n: int | None = None) -> np.ndarray:
        """sr_sample_read: the hits as an array of [seen, kept] rows, one per step."""
        n = SR_SAMPLE_STEPS if n is None else n
        hits = (SrSampleHits * max(n, 1))()
        m = _check(self._lib.sr_sample_read(self._h, hits, n), "sr_sample_read")
        return np.array([[hits[i].seen, hits[i].kept] for i in range(m)], np.uint64).reshape(m, 2)

    def sample_reset(self) -> None:
        _check(self._lib.sr_sample_reset(self._h), "sr_sample_reset")

    def set_sample(self, cfg: SampleConfig | None) -> None:
        """sr_set_sample: later route_pack submissions thin the names over the limit and mark the kept lines with
        the sample rate, between the name rules and the coalescing (None: off)."""
        _check(self._lib.sr_set_sample(self._h, cfg.ref() if cfg is not None else None), "sr_set_sample")

    def route_pack_sample(self, slot: int):
        """sr_route_pack_sample after route_pack_result(slot) (route_pack: slot 2): (rewritten text, counts[4]: out,
        dropped, rewritten, text bytes needed; the seed the batch was thinned under)."""
        text, n = ctypes.c_void_p(), ctypes.c_size_t()
        counts = (ctypes.c_uint64 * 4)()
        seed = ctypes.c_uint64()
        _check(self._lib.sr_route_pack_sample(self._h, slot, ctypes.byref(text), ctypes.byref(n), counts, ctypes.byref(seed)),
               "sr_route_pack_sample")
        raw = bytes((ctypes.c_uint8 * n.value).from_address(text.value)) if n.value else b""
        return raw, np.array(list(counts), np.uint64), int(seed.value)

    def route_pack_submit_slots(self, slot: int, slots, stride: int, lens, fill=None) -> None:
        """sr_route_pack_submit_slots (asynchronous): `slots` is page-locked memory (a HostBuffer, or its
        address) holding datagram j in lens[j] bytes at j * stride; it must stay alive and unchanged until
        route_pack_result(slot). fill as route_pack_submit."""
        addr = slots.addr if isinstance(slots, HostBuffer) else int(slots)
        ln = np.ascontiguousarray(lens, dtype=np.uint16)
        f = None
        if fill is not None:
            f = np.zeros(max(self.n_downstreams, 1), dtype=np.uint16)
            f[: self.n_downstreams] = np.asarray(fill, dtype=np.uint16)
        self._pending = getattr(self, "_pending", {})
        self._pending[slot] = slots
        _check(self._lib.sr_route_pack_submit_slots(self._h, slot, ctypes.c_void_p(addr), stride,
                                                    ln.ctypes.data if ln.size else None, int(ln.size),
                                                    f.ctypes.data if f is not None else None),
               "sr_route_pack_submit_slots")

    def route_pack_result(self, slot: int):
        """sr_route_pack_result: (sorted records, packets, fill after, n_valid, probed-dead shard ids),
        copied out of the slot."""
        r = SrPackResult()
        _check(self._lib.sr_route_pack_result(self._h, slot, ctypes.byref(r)), "sr_route_pack_result")
        n = self.n_downstreams
        take = lambda addr, count, dt: (np.frombuffer((ctypes.c_uint8 * (count * dt.itemsize)).from_address(addr),
                                                      dtype=dt).copy() if count else np.zeros(0, dt))
        srt = take(r.sorted, r.n_records, RECORD_DTYPE)
        pk = take(r.packets, r.n_packets, PACKET_DTYPE)
        fill = take(r.fill, n, np.dtype(np.uint16))
        pw = take(r.probed_dead, max((n + 63) // 64, 1), np.dtype(np.uint64))
        getattr(self, "_pending", {}).pop(slot, None)
        return srt, pk, fill, int(r.n_valid), bitmap_shards(pw, n)

    def pack_packets(self, d_recs: int, d_n_records: int, max_records: int, d_fill_in: int | None,
                     d_probed_dead: int | None, d_sorted: int, d_packets: int, max_pk: int, d_counts: int,
                     d_fill_out: int) -> None:
        """sr_pack_packets with raw device pointers (asynchronous on the context's stream)."""
        vp = ctypes.c_void_p
        _check(self._lib.sr_pack_packets(self._h, vp(d_recs), vp(d_n_records), max_records, vp(d_fill_in or 0),
                                         vp(d_probed_dead or 0), vp(d_sorted), vp(d_packets), max_pk, vp(d_counts),
                                         vp(d_fill_out)), "sr_pack_packets")

    @staticmethod
    def owner_batches(batches):
        """The sr_batch array of [(d_bytes, nbytes, d_recs, max_records, d_n_records[, d_probed_dead]), ...]
        (reusable; the bitmap is what exchange_dead reads, the pack calls ignore it)."""
        arr = (SrBatch * max(len(batches), 1))()
        for i, b in enumerate(batches):
            db, nb, dr, mr, dn = b[:5]
            arr[i] = SrBatch(db, nb, dr, mr, None, dn, (b[5] or None) if len(b) > 5 else None)
        return arr

    _owner_batches = owner_batches

    def pack_many_by_owner(self, batches, n_owners: int, d_out_bytes: int, out_cap: int, d_out_recs: int,
                           d_owner_counts: int) -> None:
        """sr_pack_many_by_owner: batches = [(d_bytes, nbytes, d_recs, max_records, d_n_records), ...]."""
        vp = ctypes.c_void_p
        _check(self._lib.sr_pack_many_by_owner(self._h, self._owner_batches(batches), len(batches), n_owners,
                                               vp(d_out_bytes), out_cap, vp(d_out_recs), vp(d_owner_counts)),
               "sr_pack_many_by_owner")

    def pack_owner_sizes(self, batches, n_owners: int, d_owner_counts: int) -> None:
        """sr_pack_owner_sizes: the split sizes of sr_pack_many_by_owner alone (batches as there)."""
        _check(self._lib.sr_pack_owner_sizes(self._h, self._owner_batches(batches), len(batches), n_owners,
                                             ctypes.c_void_p(d_owner_counts)), "sr_pack_owner_sizes")

    def pack_owner_scatter(self, batches, n_owners: int, own: int, d_own_bytes: int, d_own_recs: int,
                           d_out_bytes: int, out_cap: int, d_out_recs: int) -> None:
        """sr_pack_owner_scatter: the rest of the pack after pack_owner_sizes, owner `own`'s chunk written to
        d_own_bytes / d_own_recs (e.g. its place in the exchange's receive buffers)."""
        vp = ctypes.c_void_p
        _check(self._lib.sr_pack_owner_scatter(self._h, self._owner_batches(batches), len(batches), n_owners, own,
                                               vp(d_own_bytes), vp(d_own_recs), vp(d_out_bytes), out_cap,
                                               vp(d_out_recs)), "sr_pack_owner_scatter")

    def pack_packets_many(self, batches) -> None:
        """sr_pack_packets_many: batches = [(d_recs, d_n_records, max_records, d_fill_in, d_probed_dead,
        d_sorted, d_packets, max_packets, d_counts, d_fill_out), ...] (raw device pointers, 0 = NULL)."""
        arr = (SrPackBatch * max(len(batches), 1))()
        for i, b in enumerate(batches):
            arr[i] = SrPackBatch(*[x or None if j not in (2, 7) else x for j, x in enumerate(b)])
        _check(self._lib.sr_pack_packets_many(self._h, arr, len(batches)), "sr_pack_packets_many")

    def route_pack_many(self, batches) -> None:
        """sr_route_pack_many: batches = [(d_bytes, nbytes, d_out, max_records, d_hashes, d_n_records,
        d_probed_dead, d_fill_in, d_sorted, d_packets, max_packets, d_counts, d_fill_out), ...]: each routed
        into d_out, then packed from it (raw device pointers, 0 = NULL)."""
        n = max(len(batches), 1)
        ra, pa = (SrBatch * n)(), (SrPackBatch * n)()
        for i, b in enumerate(batches):
            db, nb, do, mr, dh, dc, dp, fi, ds, dpk, mp, dcnt, fo = b
            ra[i] = SrBatch(db, nb, do, mr, dh or None, dc, dp or None)
            pa[i] = SrPackBatch(do, dc, mr, fi or None, dp or None, ds, dpk, mp, dcnt, fo)
        _check(self._lib.sr_route_pack_many(self._h, ra, pa, len(batches)), "sr_route_pack_many")

    def exchange_sizes(self, comm: "Comm", d_owner_counts: int, d_recv_counts: int):
        """sr_exchange_sizes: returns (sent, received) as u64 [world, 2] {lines, bytes} arrays."""
        sent = np.zeros((comm.world, 2), dtype=np.uint64)
        received = np.zeros((comm.world, 2), dtype=np.uint64)
        vp = ctypes.c_void_p
        _check(self._lib.sr_exchange_sizes(self._h, comm.handle, vp(d_owner_counts), vp(d_recv_counts),
                                           sent.ctypes.data, received.ctypes.data), "sr_exchange_sizes")
        return sent, received

    def regroup_launch(self, comm: "Comm", batches, d_owner_counts: int, d_recv_counts: int, d_packed: int,
                       packed_cap: int, d_packed_recs: int, d_recv_bytes: int, recv_bytes_cap: int, d_recv_recs: int,
                       recv_recs_cap: int):
        """sr_regroup_launch (batches as pack_many_by_owner's, or an array from owner_batches()): returns
        (fits, sent, received); fits False = -ENOSPC: the sizes are exchanged, nothing scattered or sent yet
        (finish with pack_owner_scatter and exchange_data into buffers of the received totals)."""
        sent = np.zeros((comm.world, 2), dtype=np.uint64)
        received = np.zeros((comm.world, 2), dtype=np.uint64)
        arr = batches if isinstance(batches, ctypes.Array) else self._owner_batches(batches)
        n = len(batches)
        vp = ctypes.c_void_p
        rc = self._lib.sr_regroup_launch(self._h, comm.handle, arr, n, vp(d_owner_counts), vp(d_recv_counts),
                                         vp(d_packed), packed_cap, vp(d_packed_recs), vp(d_recv_bytes),
                                         recv_bytes_cap, vp(d_recv_recs), recv_recs_cap, sent.ctypes.data,
                                         received.ctypes.data)
        if rc == -errno.ENOSPC:
            return False, sent, received
        _check(rc, "sr_regroup_launch")
        return True, sent, received

    def regroup_run(self, transport: "Transport", world: int, rank: int, batches, d_owner_counts: int,
                    d_recv_counts: int, d_packed: int, packed_cap: int, d_packed_recs: int, d_recv_bytes: int,
                    recv_bytes_cap: int, d_recv_recs: int, recv_recs_cap: int):
        """sr_regroup_run: regroup_launch's sequence on a Python transport whose sizes(d_owner_counts,
        d_recv_counts) does the size exchange (returns (sent, received) [world, 2] and writes d_recv_counts).
        Returns (fits, sent, received) as regroup_launch."""
        sent = np.zeros((world, 2), dtype=np.uint64)
        received = np.zeros((world, 2), dtype=np.uint64)
        err = []
        cb = _transport_struct(transport, err)

        def sizes(_u, d_cnt, d_rcv, h_s, h_r):
            try:
                s_, r_ = transport.sizes(int(d_cnt or 0), int(d_rcv or 0))
                hs = np.frombuffer((ctypes.c_uint8 * (16 * world)).from_address(h_s), dtype=np.uint64)
                hr = np.frombuffer((ctypes.c_uint8 * (16 * world)).from_address(h_r), dtype=np.uint64)
                hs[:] = np.asarray(s_, dtype=np.uint64).reshape(-1)
                hr[:] = np.asarray(r_, dtype=np.uint64).reshape(-1)
                return 0
            except Exception as e:   # noqa: BLE001 - reported after the C call returns
                err.append(e)
                return -errno.EIO

        sizes_fn = _SIZES_FN(sizes)
        arr = batches if isinstance(batches, ctypes.Array) else self._owner_batches(batches)
        vp = ctypes.c_void_p
        rc = self._lib.sr_regroup_run(self._h, ctypes.byref(cb), sizes_fn, world, rank, arr, len(batches),
                                      vp(d_owner_counts), vp(d_recv_counts), vp(d_packed), packed_cap,
                                      vp(d_packed_recs), vp(d_recv_bytes), recv_bytes_cap, vp(d_recv_recs),
                                      recv_recs_cap, sent.ctypes.data, received.ctypes.data)
        if err:
            raise err[0]
        if rc == -errno.ENOSPC:
            return False, sent, received
        _check(rc, "sr_regroup_run")
        return True, sent, received

    def exchange_data(self, comm: "Comm", d_packed: int, d_packed_recs: int, sent: np.ndarray,
                      received: np.ndarray, d_recv_bytes: int, d_recv_recs: int) -> None:
        """sr_exchange_data (asynchronous on the router's stream)."""
        sent = np.ascontiguousarray(sent, dtype=np.uint64)
        received = np.ascontiguousarray(received, dtype=np.uint64)
        vp = ctypes.c_void_p
        _check(self._lib.sr_exchange_data(self._h, comm.handle, vp(d_packed), vp(d_packed_recs), sent.ctypes.data,
                                          received.ctypes.data, vp(d_recv_bytes), vp(d_recv_recs)),
               "sr_exchange_data")

    def exchange_rebase(self, d_recv_recs: int, peers: np.ndarray) -> None:
        """sr_exchange_rebase: the exchange's record rebase alone (asynchronous on the router's stream)."""
        p = np.ascontiguousarray(peers, dtype=PEER_DTYPE)
        _check(self._lib.sr_exchange_rebase(self._h, ctypes.c_void_p(d_recv_recs), p.ctypes.data, int(p.size)),
               "sr_exchange_rebase")

    def dead_words(self) -> int:
        """Words of one probed-dead bitmap (a row of d_all_dead): max(1, ceil(n_downstreams / 64))."""
        return max((self.n_downstreams + 63) // 64, 1)

    def exchange_dead_run(self, transport: "Transport", world: int, rank: int, batches, d_all_dead: int) -> None:
        """sr_exchange_dead_run: the launch's probed-dead bitmaps (batches as owner_batches takes them, with
        d_probed_dead, or its array) ORed into row `rank` of d_all_dead (u64 [world, dead_words()]) and the
        rows exchanged on a Python transport under tag 2."""
        err = []
        cb = _transport_struct(transport, err)
        arr = batches if isinstance(batches, ctypes.Array) else self._owner_batches(batches)
        rc = self._lib.sr_exchange_dead_run(self._h, ctypes.byref(cb), world, rank, arr, len(batches),
                                            ctypes.c_void_p(d_all_dead))
        if err:
            raise err[0]
        _check(rc, "sr_exchange_dead_run")

    def exchange_dead(self, comm: "Comm", batches, d_all_dead: int) -> None:
        """sr_exchange_dead: exchange_dead_run over the communicator (asynchronous on the router's stream;
        collective)."""
        arr = batches if isinstance(batches, ctypes.Array) else self._owner_batches(batches)
        _check(self._lib.sr_exchange_dead(self._h, comm.handle, arr, len(batches), ctypes.c_void_p(d_all_dead)),
               "sr_exchange_dead")

    def owner_pack(self, batch: SrOwnerBatch | None = None, **fields) -> None:
        """sr_owner_pack: one launch's receive buffer into packets (an SrOwnerBatch, or its fields by name),
        asynchronous on the router's stream."""
        b = batch if batch is not None else SrOwnerBatch(**{k: (v or None) if k.startswith("d_") else v
                                                            for k, v in fields.items()})
        _check(self._lib.sr_owner_pack(self._h, ctypes.byref(b)), "sr_owner_pack")

    def flush_pending(self, d_fill: int, d_pend: int, d_packets: int, max_pk: int, d_counts: int, d_payload: int,
                      payload_cap: int, d_offsets: int, d_total: int) -> None:
        """sr_flush_pending: every non-empty pending slot on the device into one packet of the arena, its fill
        reset (asynchronous on the router's stream; capturable)."""
        vp = ctypes.c_void_p
        _check(self._lib.sr_flush_pending(self._h, vp(d_fill or 0), vp(d_pend or 0), vp(d_packets or 0), max_pk,
                                          vp(d_counts or 0), vp(d_payload or 0), payload_cap, vp(d_offsets or 0),
                                          vp(d_total or 0)), "sr_flush_pending")

    def sync(self) -> None:
        _check(self._lib.sr_sync(self._h), "sr_sync")


class CommGroup:
    """The meeting place of an in-process communicator's ranks (sr_comm_group_open; host only): the threads
    of one process each open their rank on it with Comm.local. Close it after its communicators."""

    def __init__(self, world: int):
        self._lib = lib()
        h = ctypes.c_void_p()
        _check(self._lib.sr_comm_group_open(ctypes.byref(h), world), "sr_comm_group_open")
        self.handle, self.world = h, world

    def close(self) -> None:
        """sr_comm_group_close: raises SrError(EBUSY) while a communicator of the group is open."""
        if self.handle:
            _check(self._lib.sr_comm_group_close(self.handle), "sr_comm_group_close")
            self.handle = ctypes.c_void_p()


class Comm:
    """A communicator of the C ABI: RCCL (sr_comm_open: `world` ranks, one GPU each) or, with Comm.local,
    ranks that are threads of one process (sr_comm_open_local)."""

    def __init__(self, comm_id: bytes, world: int, rank: int, device: int):
        self._lib = lib()
        if len(comm_id) != SR_COMM_ID_BYTES:
            raise ValueError("communicator id must be SR_COMM_ID_BYTES bytes")
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(comm_id), SR_COMM_ID_BYTES)
        _check(self._lib.sr_comm_open(ctypes.byref(h), buf, world, rank, device), "sr_comm_open")
        self.handle, self.world, self.rank, self.device = h, world, rank, device

    @staticmethod
    def new_id() -> bytes:
        buf = ctypes.create_string_buffer(SR_COMM_ID_BYTES)
        _check(lib().sr_comm_id(buf), "sr_comm_id")
        return buf.raw

    @classmethod
    def from_group(cls, device: int, group=None) -> "Comm":
        """Every rank of a torch.distributed group joins one communicator (rank 0 makes the id)."""
        import torch.distributed as dist
        box = [None]
        if dist.get_rank(group) == 0:   # a failure here still reaches every rank (no rank left waiting)
            try:
                box[0] = cls.new_id()
            except (OSError, RuntimeError) as e:
                box[0] = f"{type(e).__name__}: {e}"
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if isinstance(box[0], str):
            raise RuntimeError(f"rank 0 could not make the communicator id: {box[0]}")
        return cls(box[0], dist.get_world_size(group), dist.get_rank(group), device)

    @classmethod
    def local(cls, group: CommGroup, rank: int, device: int) -> "Comm":
        """sr_comm_open_local: rank `rank` of an in-process group, opened by the thread that owns the rank
        (no RCCL; does not wait for the other ranks)."""
        self = cls.__new__(cls)
        self._lib = lib()
        h = ctypes.c_void_p()
        _check(self._lib.sr_comm_open_local(ctypes.byref(h), group.handle, rank, device), "sr_comm_open_local")
        self.handle, self.world, self.rank, self.device, self.group = h, group.world, rank, device, group
        return self

    def set_timeout(self, ms: int) -> None:
        """sr_comm_set_timeout: every host wait of a collective on this comm gives up after ms milliseconds
        (-ETIMEDOUT, the communicator broken: -EPIPE from then on); 0 = no deadline (the default)."""
        _check(self._lib.sr_comm_set_timeout(self.handle, int(ms)), "sr_comm_set_timeout")

    def close(self) -> None:
        if self.handle:
            self._lib.sr_comm_close(self.handle)
            self.handle = ctypes.c_void_p()


def exchange_plan(world: int, rank: int, sent, received):
    """sr_exchange_plan (host only): returns (peers: PEER_DTYPE [world], totals: u64 [4] = {lines sent,
    bytes sent, lines received, bytes received})."""
    s = np.ascontiguousarray(sent, dtype=np.uint64).reshape(-1)
    r = np.ascontiguousarray(received, dtype=np.uint64).reshape(-1)
    if s.size != 2 * world or r.size != 2 * world:
        raise ValueError("split sizes must be [world, 2]")
    peers = np.zeros(max(world, 1), dtype=PEER_DTYPE)
    tot = np.zeros(4, dtype=np.uint64)
    _check(lib().sr_exchange_plan(world, rank, s.ctypes.data, r.ctypes.data, peers.ctypes.data, tot.ctypes.data),
           "sr_exchange_plan")
    return peers, tot


class Transport:
    """A transport for sr_exchange_run written in Python (override the methods; raise to fail).
    Addresses are plain integers; what they address (host or device memory) is the transport's business."""

    def group_start(self) -> None:
        pass

    def group_end(self) -> None:
        pass

    def send(self, addr: int, nbytes: int, peer: int, tag: int) -> None:
        raise NotImplementedError

    def recv(self, addr: int, nbytes: int, peer: int, tag: int) -> None:
        raise NotImplementedError

    def copy(self, dst: int, src: int, nbytes: int) -> None:
        ctypes.memmove(dst, src, nbytes)

    def sizes(self, d_owner_counts: int, d_recv_counts: int):
        """sr_regroup_run's size exchange: returns (sent, received) u64 [world, 2] and writes the received
        sizes to d_recv_counts."""
        raise NotImplementedError

    def rebase(self, recs_addr: int, peers: np.ndarray, n_lines: int) -> None:
        """Host memory: records [recv_line0, +recv_lines) of every source move by its recv_byte0."""
        recs = host_records(recs_addr, n_lines)
        for p in peers:
            a, n = int(p["recv_line0"]), int(p["recv_lines"])
            recs["offset"][a: a + n] += np.uint32(p["recv_byte0"])


class CommTransport(Transport):
    """The communicator's own sr_transport (sr_comm_transport) bound to a router's stream, as a Python
    Transport: every method calls the C structure's function pointer and raises SrError on a negative
    errno. For exchange_run / Router.regroup_run / Router.exchange_dead_run on a communicator, and for
    sends and receives of the caller's own (device addresses, tags 0..2) between group_start and
    group_end. Call bind() again after Router.set_stream."""

    def __init__(self, comm: "Comm", router: "Router"):
        self.comm, self.router = comm, router
        self._t = SrTransport()
        self.bind()

    def bind(self) -> None:
        _check(lib().sr_comm_transport(self.comm.handle, self.router.handle, ctypes.byref(self._t)),
               "sr_comm_transport")

    def group_start(self) -> None:
        _check(self._t.group_start(self._t.user), "transport group_start")

    def group_end(self) -> None:
        _check(self._t.group_end(self._t.user), "transport group_end")

    def send(self, addr: int, nbytes: int, peer: int, tag: int) -> None:
        _check(self._t.send(self._t.user, addr, nbytes, peer, tag), "transport send")

    def recv(self, addr: int, nbytes: int, peer: int, tag: int) -> None:
        _check(self._t.recv(self._t.user, addr, nbytes, peer, tag), "transport recv")

    def copy(self, dst: int, src: int, nbytes: int) -> None:
        _check(self._t.copy(self._t.user, dst, src, nbytes), "transport copy")

    def rebase(self, recs_addr: int, peers: np.ndarray, n_lines: int) -> None:
        p = np.ascontiguousarray(peers, dtype=PEER_DTYPE)
        _check(self._t.rebase(self._t.user, recs_addr, ctypes.cast(p.ctypes.data, ctypes.POINTER(SrExchangePeer)),
                              int(p.size), int(n_lines)), "transport rebase")

    def sizes(self, d_owner_counts: int, d_recv_counts: int):
        return self.router.exchange_sizes(self.comm, d_owner_counts, d_recv_counts)


def host_records(addr: int, n: int) -> np.ndarray:
    """A writable RECORD_DTYPE view of n records at a host address."""
    if n == 0:
        return np.zeros(0, dtype=RECORD_DTYPE)
    return np.frombuffer((ctypes.c_uint8 * (8 * n)).from_address(addr), dtype=RECORD_DTYPE)


def _transport_struct(transport: Transport, err: list) -> SrTransport:
    """An SrTransport whose callbacks call the Python transport; exceptions go to err (the callback
    returns -EIO). Keep the returned structure alive for the duration of the C call."""
    def wrap(fn):
        def call(*a):
            try:
                fn(*a)
                return 0
            except Exception as e:   # noqa: BLE001 - reported after the C call returns
                err.append(e)
                return -errno.EIO
        return call

    def rebase(_u, recs, peers_p, w, n):
        arr = np.ctypeslib.as_array(ctypes.cast(peers_p, ctypes.POINTER(ctypes.c_uint64)), shape=(w * 8,))
        transport.rebase(recs, arr.copy().view(PEER_DTYPE), int(n))

    return SrTransport(None,
                       _GROUP_FN(wrap(lambda _u: transport.group_start())),
                       _GROUP_FN(wrap(lambda _u: transport.group_end())),
                       _SEND_FN(wrap(lambda _u, b, n, p, t: transport.send(b, n, p, t))),
                       _SEND_FN(wrap(lambda _u, b, n, p, t: transport.recv(b, n, p, t))),
                       _COPY_FN(wrap(lambda _u, d, s, n: transport.copy(d, s, n))),
                       _REBASE_FN(wrap(rebase)))


def exchange_run(transport: Transport, world: int, rank: int, sent, received, packed: int, packed_recs: int,
                 recv_bytes: int, recv_recs: int) -> None:
    """sr_exchange_run: the C exchange plan and its calls, on a Python transport."""
    err = []
    cb = _transport_struct(transport, err)
    s = np.ascontiguousarray(sent, dtype=np.uint64).reshape(-1)
    r = np.ascontiguousarray(received, dtype=np.uint64).reshape(-1)
    if s.size != 2 * world or r.size != 2 * world:
        raise ValueError("split sizes must be [world, 2]")
    vp = ctypes.c_void_p
    rc = lib().sr_exchange_run(ctypes.byref(cb), world, rank, s.ctypes.data, r.ctypes.data, vp(packed),
                               vp(packed_recs), vp(recv_bytes), vp(recv_recs))
    if err:
        raise err[0]
    _check(rc, "sr_exchange_run")


def version() -> str:
    return lib().sr_version().decode()
