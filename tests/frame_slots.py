"""Slot arenas for the device-framing tests: datagrams laid out as recvmmsg leaves them, a strided array of
slots plus a length per slot, and what framing them must give, computed by the CPU oracle (oracle.frame,
sr-main.c:163-173) from the datagrams themselves, never by the code under test."""
from __future__ import annotations

import numpy as np

MAX_DATAGRAM = 4095
# the lengths at which framing changes behaviour: empty, shorter / at / past a 16-byte piece and a wave's
# 64 lanes, a full MTU line, the recv() cap and lengths the cap cuts
EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 1449, 4094, 4095, 4096, 65535]
POISON = 0xA5


def make_datagrams(lengths, seed: int, final_newline: bool):
    """Random datagrams of the given lengths whose last KEPT byte (the one framing looks at: byte
    min(len, 4095) - 1) is '\\n' (final_newline) or is not."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        d = rng.integers(0, 256, int(n), dtype=np.uint8)
        if n:
            k = min(int(n), MAX_DATAGRAM) - 1
            d[k] = 10 if final_newline else (d[k] if d[k] != 10 else 11)
        out.append(d.tobytes())
    return out


def build_arena(dgrams, stride: int = 4096, tail: int = 0):
    """(arena uint8, lens uint16): datagram j's first min(len, 4095) bytes at arena[j * stride:], lens[j] =
    min(len, 65535) (a length above 4095 is what a caller that did not cap reports). Bytes between the
    datagrams are POISON; the arena ends `tail` bytes after the last datagram's kept bytes (no slack that a
    stray read could hide in)."""
    count = len(dgrams)
    lens = np.array([min(len(d), 65535) for d in dgrams], dtype=np.uint16)
    last = min(len(dgrams[-1]), MAX_DATAGRAM) if count else 0
    arena = np.full((count - 1) * stride + last + tail if count else tail, POISON, dtype=np.uint8)
    for j, d in enumerate(dgrams):
        k = min(len(d), MAX_DATAGRAM)
        arena[j * stride: j * stride + k] = np.frombuffer(d[:k], dtype=np.uint8)
    return arena, lens


def expected(oracle, dgrams):
    """(framed bytes uint8, ends uint32) by the CPU oracle."""
    parts = [oracle.frame(d) for d in dgrams]
    ends = np.cumsum([len(p) for p in parts], dtype=np.int64).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), ends


def slot_bytes(arena, lens, stride: int):
    """The datagrams as a reader of the arena sees them (the kept bytes of every slot)."""
    return [arena[j * stride: j * stride + min(int(n), MAX_DATAGRAM)].tobytes() for j, n in enumerate(lens)]
