"""What sr_format_log must write (include/sr_route.h), restated in Python from the reference's texts
(sr-main.c:91,102,115,142,174,184; host/sr_core.c trace_batch): per record, in input order, "got packet" when
the record starts a datagram, then the line's WARN or its two find_downstream messages. A plain helper module
(no fixtures); tests/test_log_expect.py pins it to the reference's data thread."""
from __future__ import annotations

import numpy as np

TRACE, WARN = 0, 3
INVALID_LENGTH, INVALID_FORMAT = 0xFFFD, 0xFFFE


def cstr(b: bytes) -> bytes:
    """What printf's %.*s prints of b: up to its first NUL."""
    return b.split(b"\0", 1)[0]


def messages(data, recs, hashes, ends, n_downstreams, min_level=TRACE, max_records=None):
    """[(level, text)] of a routed batch, without prefix, cut or '\\n'. data: bytes or a uint8 array; recs: the
    input-order records; hashes: None allowed at WARN; ends: None, or the framed datagram ends."""
    raw = bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    nbytes = len(raw)
    n = len(recs) if max_records is None else min(len(recs), max_records)
    n = min(n, nbytes)
    ends = None if ends is None or len(ends) == 0 else np.asarray(ends, dtype=np.uint32)
    out = []
    offs, lens, routes = recs["offset"].tolist(), recs["length"].tolist(), recs["route"].tolist()
    hs = None if hashes is None else np.asarray(hashes, dtype=np.uint64).tolist()
    for i in range(n):
        off, ln, route = offs[i], lens[i], routes[i]
        src = min(off, nbytes)
        if min_level <= TRACE and ends is not None:
            g = int(np.searchsorted(ends, off, side="right"))   # the first datagram whose end is past off
            if g < len(ends) and (int(ends[g - 1]) if g else 0) == off:
                out.append((TRACE, b"udp_read_cb: got packet " + cstr(raw[src: max(src, min(int(ends[g]), nbytes))])))
        line = raw[src: min(src + ln, nbytes)]
        if route == INVALID_LENGTH:
            out.append((WARN, b"udp_read_cb: invalid length %d of metric " % ln + cstr(line)))
        elif route == INVALID_FORMAT:
            out.append((WARN, b"process_data_line: invalid metric " + cstr(raw[src: min(src + max(ln - 1, 0), nbytes)])))
        else:
            if min_level <= TRACE:
                out.append((TRACE, b"find_downstream: hash = %x, length = %d, line = " % (hs[i], ln) + cstr(line)))
            if route < n_downstreams:
                if min_level <= TRACE:
                    out.append((TRACE, b"find_downstream: pushing to downstream %d" % route))
            else:
                out.append((WARN, b"find_downstream: all downstreams are dead"))
    return out


def wire(msgs, prefixes=(b"", b""), max_msg=0):
    """(text, offsets u32 [n + 1], levels u8 [n]) of the messages on the wire: prefix[level] + text, cut to
    max_msg bytes when max_msg > 0, then '\\n'."""
    parts, offsets, pos = [], [0], 0
    for level, text in msgs:
        m = prefixes[1 if level == WARN else 0] + text
        if max_msg:
            m = m[:max_msg]
        parts.append(m + b"\n")
        pos += len(m) + 1
        offsets.append(pos)
    return (b"".join(parts), np.asarray(offsets, dtype=np.uint64).astype(np.uint32),
            np.asarray([lv for lv, _ in msgs], dtype=np.uint8))


def expect(data, recs, hashes, ends, n_downstreams, min_level=TRACE, prefixes=(b"", b""), max_msg=0,
           max_records=None):
    """(text, offsets, levels) as sr_format_log writes them with room for everything."""
    return wire(messages(data, recs, hashes, ends, n_downstreams, min_level, max_records), prefixes, max_msg)


def max_msgs(nbytes: int, n_datagrams: int) -> int:
    """SR_LOG_MAX_MSGS"""
    return nbytes + n_datagrams


def text_capacity(nbytes: int, n_datagrams: int, prefix_max: int) -> int:
    """SR_LOG_TEXT_CAPACITY"""
    return nbytes * (prefix_max + 43) + n_datagrams * (prefix_max + 25)
