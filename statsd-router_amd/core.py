"""ctypes view of one router data thread (include/sr_router.h, lib/libsr_router.so).

The product is the C library (host/sr_core.c over libsr_route.so); this module lets tests and the
bench drive it with Python callbacks. Loading is strict, like the package's.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import SR_SAMPLE_STEPS, SR_VALID_REASONS, SrSampleConfig, SrSampleHits, SrValidateConfig, SrValidateHits
from . import LIB_DIR, SR_RULES_MAX, SrCoalesceConfig, SrError, SrRuleHits, SrRulesConfig, SrStatsConfig, SrStatsSnapshot, StatsSnapshot, _check, alive_words, lib

ROUTER_LIB = os.path.join(LIB_DIR, "libsr_router.so")
SR_TRACE, SR_DEBUG, SR_INFO, SR_WARN, SR_ERROR = range(5)


class IoVec(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class CoreConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("max_batch_bytes", ctypes.c_size_t), ("n_downstreams", ctypes.c_uint32),
                ("ds_hosts", ctypes.POINTER(ctypes.c_char_p)), ("ds_data_ports", ctypes.POINTER(ctypes.c_char_p)),
                ("ping_prefix", ctypes.c_char_p), ("hostname", ctypes.c_char_p), ("data_port", ctypes.c_int),
                ("log_level", ctypes.c_int)]


EMIT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(IoVec), ctypes.c_int, ctypes.c_size_t)
LOG_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t)
FLUSH_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
LOG_PREFIX_FN = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t)
LOG_BLOCK_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t)
LOG_BLOCK = -1   # the level of a block entry in Core.logs

_RLIB = None


def router_lib() -> ctypes.CDLL:
    global _RLIB
    if _RLIB is None:
        lib()   # libsr_route.so first (one HIP runtime per process)
        if not os.path.exists(ROUTER_LIB):
            raise ImportError(f"{ROUTER_LIB} is missing: build it with __graft_entry__.build()")
        L = ctypes.CDLL(ROUTER_LIB)
        vp = ctypes.c_void_p
        L.sr_core_open.restype = ctypes.c_int
        L.sr_core_open.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(CoreConfig), EMIT_FN, LOG_FN, FLUSH_FN, vp]
        L.sr_core_set_alive.restype, L.sr_core_set_alive.argtypes = ctypes.c_int, [vp, vp]
        L.sr_core_batch_buffer.restype = vp
        L.sr_core_batch_buffer.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
        L.sr_core_route.restype, L.sr_core_route.argtypes = ctypes.c_int, [vp, vp, ctypes.c_size_t]
        L.sr_core_slot_buffer.restype = vp
        L.sr_core_slot_buffer.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
        L.sr_core_submit.restype, L.sr_core_submit.argtypes = ctypes.c_int, [vp, ctypes.c_int, ctypes.c_size_t]
        L.sr_core_drain.restype, L.sr_core_drain.argtypes = ctypes.c_int, [vp]
        L.sr_core_in_flight.restype, L.sr_core_in_flight.argtypes = ctypes.c_int, [vp]
        L.sr_core_flush_timer.restype, L.sr_core_flush_timer.argtypes = ctypes.c_int, [vp]
        L.sr_core_ping.restype, L.sr_core_ping.argtypes = ctypes.c_int, [vp]
        L.sr_core_state.restype = ctypes.c_int
        L.sr_core_state.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t),
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        L.sr_core_metric_name.restype = ctypes.c_char_p
        L.sr_core_metric_name.argtypes = [vp, ctypes.c_uint32, ctypes.c_int]
        L.sr_core_close.restype, L.sr_core_close.argtypes = None, [vp]
        L.sr_core_route_datagrams.restype = ctypes.c_int
        L.sr_core_route_datagrams.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t]
        L.sr_core_submit_datagrams.restype = ctypes.c_int
        L.sr_core_submit_datagrams.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp, ctypes.c_size_t]
        L.sr_core_context.restype, L.sr_core_context.argtypes = vp, [vp]
        L.sr_core_inject_faults.restype = ctypes.c_int
        L.sr_core_inject_faults.argtypes = [vp, ctypes.c_uint, ctypes.c_uint]
        L.sr_core_set_payloads.restype, L.sr_core_set_payloads.argtypes = ctypes.c_int, [vp, ctypes.c_int]
        L.sr_core_submit_slots.restype = ctypes.c_int
        L.sr_core_submit_slots.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t]
        L.sr_core_set_device_log.restype = ctypes.c_int
        L.sr_core_set_device_log.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, LOG_PREFIX_FN, LOG_BLOCK_FN]
        L.sr_core_set_name_stats.restype = ctypes.c_int
        L.sr_core_set_name_stats.argtypes = [vp, ctypes.POINTER(SrStatsConfig)]
        L.sr_core_name_stats.restype = ctypes.c_int
        L.sr_core_name_stats.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(SrStatsSnapshot)), ctypes.c_int]
        L.sr_core_set_coalesce.restype = ctypes.c_int
        L.sr_core_set_coalesce.argtypes = [vp, ctypes.POINTER(SrCoalesceConfig)]
        L.sr_core_coalesce_counts.restype = ctypes.c_int
        L.sr_core_coalesce_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
        L.sr_core_set_name_rules.restype = ctypes.c_int
        L.sr_core_set_name_rules.argtypes = [vp, ctypes.POINTER(SrRulesConfig)]
        L.sr_core_name_rule_hits.restype = ctypes.c_int
        L.sr_core_name_rule_hits.argtypes = [vp, ctypes.POINTER(SrRuleHits), ctypes.c_size_t, ctypes.c_int]
        L.sr_core_set_validate.restype = ctypes.c_int
        L.sr_core_set_validate.argtypes = [vp, ctypes.POINTER(SrValidateConfig)]
        L.sr_core_set_sample.restype = ctypes.c_int
        L.sr_core_set_sample.argtypes = [vp, ctypes.POINTER(SrSampleConfig)]
        L.sr_core_sample_hits.restype = ctypes.c_int
        L.sr_core_sample_hits.argtypes = [vp, ctypes.POINTER(SrSampleHits), ctypes.c_size_t, ctypes.c_int]
        L.sr_core_validate_hits.restype = ctypes.c_int
        L.sr_core_validate_hits.argtypes = [vp, ctypes.POINTER(SrValidateHits), ctypes.c_size_t, ctypes.c_int]
        L.sr_core_device_log_stats.restype = ctypes.c_int
        L.sr_core_device_log_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        _RLIB = L
    return _RLIB


class Core:
    """One data thread: packets and log lines are collected in Python lists
    (packets[ds] = [bytes, ...]; logs = [(level, text bytes), ...])."""

    def __init__(self, n_downstreams: int, ds_hosts, ds_data_ports, ping_prefix: str, hostname: str,
                 data_port: int, max_batch_bytes: int = 1 << 20, device: int = 0, log_level: int = SR_WARN):
        self._L = router_lib()
        self.n = n_downstreams
        self.packets: dict[int, list[bytes]] = {}
        self.logs: list[tuple[int, bytes]] = []
        self.flushes = 0
        self.emit_iovecs: list[int] = []   # pieces of every emitted packet, in emit order
        hosts = (ctypes.c_char_p * n_downstreams)(*[h.encode() for h in ds_hosts])
        ports = (ctypes.c_char_p * n_downstreams)(*[p.encode() for p in ds_data_ports])
        self._keep = (hosts, ports, ping_prefix.encode(), hostname.encode())
        cfg = CoreConfig(device, max_batch_bytes, n_downstreams, hosts, ports, self._keep[2], self._keep[3],
                         data_port, log_level)

        def emit(_u, ds, iov, cnt, nbytes):
            b = b"".join(ctypes.string_at(iov[i].base, iov[i].len) for i in range(cnt))
            assert len(b) == nbytes
            self.emit_iovecs.append(int(cnt))
            self.packets.setdefault(int(ds), []).append(b)

        def log(_u, level, msg, n):
            self.logs.append((int(level), ctypes.string_at(msg, n)))

        def flush(_u):
            self.flushes += 1

        self._cb = (EMIT_FN(emit), LOG_FN(log), FLUSH_FN(flush))
        h = ctypes.c_void_p()
        _check(self._L.sr_core_open(ctypes.byref(h), ctypes.byref(cfg), *self._cb, None), "sr_core_open")
        self._h = h

    def close(self):
        if self._h:
            self._L.sr_core_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_alive(self, alive) -> None:
        w = np.ascontiguousarray(alive_words(self.n, alive))
        _check(self._L.sr_core_set_alive(self._h, w.ctypes.data), "sr_core_set_alive")

    @staticmethod
    def _ends(ends):
        """Datagram end offsets as a u32 array (None: no boundaries)."""
        if ends is None:
            return None, 0
        a = np.ascontiguousarray(np.asarray(ends, dtype=np.uint32))
        return a, int(a.size)

    def route(self, framed: bytes, ends=None) -> None:
        """sr_core_route (ends: the framed datagrams' end offsets, for TRACE: sr_core_route_datagrams)."""
        buf = ctypes.create_string_buffer(bytes(framed), max(len(framed), 1))
        a, n = self._ends(ends)
        _check(self._L.sr_core_route_datagrams(self._h, buf, len(framed), a.ctypes.data if n else None, n),
               "sr_core_route")

    def route_in_place(self, framed: bytes, ends=None) -> None:
        """Frame into the core's page-locked batch buffer first (what a C caller does)."""
        cap = ctypes.c_size_t()
        p = self._L.sr_core_batch_buffer(self._h, ctypes.byref(cap))
        if len(framed) > cap.value:
            raise SrError(28, "batch larger than the core's buffer")
        ctypes.memmove(p, bytes(framed), len(framed))
        a, n = self._ends(ends)
        _check(self._L.sr_core_route_datagrams(self._h, p, len(framed), a.ctypes.data if n else None, n),
               "sr_core_route")

    def submit(self, framed: bytes, ends=None) -> None:
        """Double-buffered: frame into the next slot's buffer and sr_core_submit it (the previous
        batch completes here, the new one stays in flight until the next submit or drain)."""
        slot = getattr(self, "_slot", 0)
        cap = ctypes.c_size_t()
        p = self._L.sr_core_slot_buffer(self._h, slot, ctypes.byref(cap))
        if len(framed) > cap.value:
            raise SrError(28, "batch larger than the core's buffer")
        ctypes.memmove(p, bytes(framed), len(framed))
        a, n = self._ends(ends)
        rc = self._L.sr_core_submit_datagrams(self._h, slot, len(framed), a.ctypes.data if n else None, n)
        if self._L.sr_core_in_flight(self._h) == slot:
            self._slot = slot ^ 1   # taken, even when completing the previous batch failed
        _check(rc, "sr_core_submit")

    def submit_slots(self, dgrams) -> None:
        """Double-buffered, without framing on the host: every datagram goes as received into a 4096-byte slot
        of the next slot's buffer (what recvmmsg does) and sr_core_submit_slots takes the lengths."""
        slot = getattr(self, "_slot", 0)
        cap = ctypes.c_size_t()
        p = self._L.sr_core_slot_buffer(self._h, slot, ctypes.byref(cap))
        if len(dgrams) * 4096 > cap.value:
            raise SrError(28, "more datagrams than the core's buffer has slots")
        lens = np.zeros(max(len(dgrams), 1), dtype=np.uint16)
        for j, d in enumerate(dgrams):
            d = bytes(d)[:4095]   # recv() reads at most 4095 bytes
            ctypes.memmove(p + 4096 * j, d, len(d))
            lens[j] = len(d)
        rc = self._L.sr_core_submit_slots(self._h, slot, lens.ctypes.data, len(dgrams))
        if self._L.sr_core_in_flight(self._h) == slot:
            self._slot = slot ^ 1   # taken, even when completing the previous batch failed
        _check(rc, "sr_core_submit_slots")

    def inject_faults(self, fail_submit: int = 0, fail_finish: int = 0) -> None:
        """sr_core_inject_faults (test hook)."""
        _check(self._L.sr_core_inject_faults(self._h, fail_submit, fail_finish), "sr_core_inject_faults")

    def set_payloads(self, on: bool = True) -> None:
        """sr_core_set_payloads: later batches' packets come from the device's arena (at most two pieces
        per emitted packet)."""
        _check(self._L.sr_core_set_payloads(self._h, 1 if on else 0), "sr_core_set_payloads")

    def set_device_log(self, on: bool = True, text_cap: int = 0, prefixes=None) -> None:
        """sr_core_set_device_log. prefixes None: per-message mode (the messages reach `logs` as always).
        prefixes = (TRACE bytes, WARN bytes): block mode; every batch's text is recorded as one
        (LOG_BLOCK, text) entry of `logs`, in its place among the host's messages, and as (text, n_msgs) in
        `blocks`."""
        self.blocks = getattr(self, "blocks", [])

        def prefix(_u, level, dst, cap):
            p = prefixes[1 if level >= SR_WARN else 0][:cap]
            ctypes.memmove(dst, p, len(p))
            return len(p)

        def block(_u, text, n, n_msgs):
            b = ctypes.string_at(text, n)
            self.blocks.append((b, int(n_msgs)))
            self.logs.append((LOG_BLOCK, b))

        blk = on and prefixes is not None
        self._log_cb = (LOG_PREFIX_FN(prefix) if blk else LOG_PREFIX_FN(0), LOG_BLOCK_FN(block) if blk else LOG_BLOCK_FN(0))
        _check(self._L.sr_core_set_device_log(self._h, 1 if on else 0, text_cap, *self._log_cb), "sr_core_set_device_log")

    def device_log_stats(self):
        """sr_core_device_log_stats: (batches whose log came from the device, batches the host formatted)."""
        d, h = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.sr_core_device_log_stats(self._h, ctypes.byref(d), ctypes.byref(h)), "sr_core_device_log_stats")
        return d.value, h.value

    def set_name_stats(self, on: bool = True, **cfg) -> None:
        """sr_core_set_name_stats: later batches are also counted on the GPU (fields of sr_stats_config; none =
        the defaults)."""
        _check(self._L.sr_core_set_name_stats(self._h, ctypes.byref(SrStatsConfig(**cfg)) if on else None),
               "sr_core_set_name_stats")

    def set_coalesce(self, on: bool = True, slots: int = 0) -> None:
        """sr_core_set_coalesce: later batches have their plain counters coalesced on the GPU."""
        _check(self._L.sr_core_set_coalesce(self._h, ctypes.byref(SrCoalesceConfig(slots)) if on else None),
               "sr_core_set_coalesce")

    def set_name_rules(self, rules) -> None:
        """sr_core_set_name_rules: later batches lose the lines that the RuleSet drops (None: off)."""
        _check(self._L.sr_core_set_name_rules(self._h, rules.ref() if rules is not None else None),
               "sr_core_set_name_rules")

    def name_rule_hits(self, reset: bool = False) -> np.ndarray:
        """sr_core_name_rule_hits: drains, then [lines, bytes] per rule and, last, for the default."""
        hits = (SrRuleHits * (SR_RULES_MAX + 1))()
        m = _check(self._L.sr_core_name_rule_hits(self._h, hits, SR_RULES_MAX + 1, 1 if reset else 0),
                   "sr_core_name_rule_hits")
        return np.array([[hits[i].lines, hits[i].bytes] for i in range(m)], np.uint64).reshape(m, 2)

    def set_validate(self, cfg) -> None:
        """sr_core_set_validate: later batches lose the lines whose reason the ValidateConfig drops (None: off)."""
        _check(self._L.sr_core_set_validate(self._h, cfg.ref() if cfg is not None else None), "sr_core_set_validate")

    def set_sample(self, cfg) -> None:
        """sr_core_set_sample: later batches have the names over the SampleConfig's limit thinned and the kept lines
        marked with the sample rate (None: off)."""
        _check(self._L.sr_core_set_sample(self._h, cfg.ref() if cfg is not None else None), "sr_core_set_sample")

    def sample_hits(self, reset: bool = False) -> np.ndarray:
        """sr_core_sample_hits: drains, then [seen, kept] per step."""
        hits = (SrSampleHits * SR_SAMPLE_STEPS)()
        m = _check(self._L.sr_core_sample_hits(self._h, hits, SR_SAMPLE_STEPS, 1 if reset else 0), "sr_core_sample_hits")
        return np.array([[hits[i].seen, hits[i].kept] for i in range(m)], np.uint64).reshape(m, 2)

    def validate_hits(self, reset: bool = False) -> np.ndarray:
        """sr_core_validate_hits: drains, then [lines, bytes] per reason (row 0: the OK lines)."""
        hits = (SrValidateHits * SR_VALID_REASONS)()
        m = _check(self._L.sr_core_validate_hits(self._h, hits, SR_VALID_REASONS, 1 if reset else 0),
                   "sr_core_validate_hits")
        return np.array([[hits[i].lines, hits[i].bytes] for i in range(m)], np.uint64).reshape(m, 2)

    def coalesce_counts(self, reset: bool = False):
        """sr_core_coalesce_counts: [lines out, lines dropped, groups merged, merged text bytes] so far."""
        t = (ctypes.c_uint64 * 4)()
        _check(self._L.sr_core_coalesce_counts(self._h, t, 1 if reset else 0), "sr_core_coalesce_counts")
        return [int(x) for x in t]

    def name_stats(self, reset: bool = False) -> StatsSnapshot:
        """sr_core_name_stats: drains, then a copy of the snapshot; reset starts the statistics again."""
        p = ctypes.POINTER(SrStatsSnapshot)()
        _check(self._L.sr_core_name_stats(self._h, ctypes.byref(p), 1 if reset else 0), "sr_core_name_stats")
        try:
            return StatsSnapshot.copy_of(p.contents)
        finally:
            lib().sr_stats_free(p)

    def set_layout(self, layout: int) -> None:
        """sr_set_layout on the core's device context (sr_core_context)."""
        _check(lib().sr_set_layout(self._L.sr_core_context(self._h), int(layout)), "sr_set_layout")

    def in_flight(self) -> int:
        """sr_core_in_flight: the slot whose batch is on the GPU, or -1."""
        return self._L.sr_core_in_flight(self._h)

    def drain(self) -> None:
        _check(self._L.sr_core_drain(self._h), "sr_core_drain")

    def flush_timer(self) -> None:
        _check(self._L.sr_core_flush_timer(self._h), "sr_core_flush_timer")

    def ping(self) -> None:
        _check(self._L.sr_core_ping(self._h), "sr_core_ping")

    def state(self, ds: int):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        tr, pk = ctypes.c_int32(), ctypes.c_int32()
        _check(self._L.sr_core_state(self._h, ds, ctypes.byref(p), ctypes.byref(n), ctypes.byref(tr),
                                     ctypes.byref(pk)), "sr_core_state")
        return ctypes.string_at(p.value, n.value) if n.value else b"", tr.value, pk.value

    def metric_name(self, ds: int, which: int) -> bytes:
        return self._L.sr_core_metric_name(self._h, ds, which)
