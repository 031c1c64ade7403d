"""What a submission of the host-memory path gives with any of the four record stages on, composed from the existing
restatements in the submit paths' order: the oracle's route launch, tests/validate_expect.py, tests/rules_expect.py,
tests/sample_expect.py, tests/coalesce_expect.py, then the oracle's packing and the payload expectation over the
device's batch as the stages leave it: the batch, the sample text in its arena, the merged text behind that."""
from __future__ import annotations

import numpy as np

import coalesce_expect as CE
import payload_expect as X
import rules_expect as RE
import sample_expect as SE
import validate_expect as VE


class Model:
    """validate: a drop mask or None; rules: a rule list or None; sample: dict(limit, types, slots, seed) with seed =
    cfg.seed + seed_add, or None; coalesce: bool."""

    def __init__(self, oracle, data, n, alive, fills, validate=None, rules=None, sample=None, coalesce=False):
        arr = np.frombuffer(data, np.uint8)
        self.recs, self.hashes, self.n_in = oracle.route(arr, n, alive)
        self.probed = oracle.probed_dead(arr, n, alive) if alive is not None else np.zeros(0, np.int64)
        out, hs = self.recs, self.hashes
        self.v = self.res = self.sa = self.co = None
        if validate is not None:
            self.v = VE.apply(data, out, hs, n, validate)
            out, hs = self.v.out, self.v.hashes_out
        if rules is not None:
            self.res = RE.apply(data, out, hs, n, rules)
            out, hs = self.res.out, self.res.hashes_out
        whole = data
        if sample is not None:
            self.sa = SE.apply(data, out, hs, n, sample["limit"], sample.get("types", SE.TYPES_DEFAULT), sample.get("slots", 0),
                               sample.get("seed", 0) & SE.M64)
            out, hs = self.sa.out, self.sa.hashes_out
            arena = SE.append_capacity(len(data))
            assert len(self.sa.text) <= arena
            whole = data + self.sa.text + bytes(arena - len(self.sa.text))
        if coalesce:   # the stage's batch is the device's batch with the sample arena; its own arena is len(data)
            self.co = CE.coalesce(whole, out, hs, n, CE.DEFAULT_SLOTS, len(data))
            assert self.co.complete
            out = self.co.out
            whole = whole + self.co.text
        self.out = out
        self.whole = whole
        self.sorted, self.packets, self.fill_out, self.n_valid = oracle.pack_packets(out, n, fills, self.probed)
        pending = {k: bytes(int(f)) for k, f in enumerate(fills)}
        self.arena, self.offsets, self.rooms = X.flat_expectation(self.whole, self.sorted, self.packets, pending)
        self.total = int(self.offsets[-1])

    def pack(self):
        return (self.sorted, self.packets, self.fill_out, self.n_valid, self.probed)

    def lines(self):
        """Per shard, the lines the packets carry, in order."""
        per = {}
        for r in self.sorted[: self.n_valid]:
            o, ln = int(r["offset"]), int(r["length"])
            per.setdefault(int(r["route"]), []).append(self.whole[o:o + ln])
        return per
