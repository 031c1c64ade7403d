"""GPU: a plain bench.py run is lean and --dump-outputs writes what its last timed step returned.

One small run (C2 lines, 5 batches in one launch: 1.3 M records, more than the dump's sample) in a
child process; the dumped counts and sampled record fields must equal the C oracle's records of the
same seeded batches at the same sample positions. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

NB = 5      # batches, all in one launch
STEPS = 3


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--min-warmup-ms", "0", "--batches", str(NB), "--per-launch", str(NB),
                        "--dump-outputs", out], capture_output=True, text=True, env=env, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), out


def test_plain_line_has_the_headline_and_no_other_leg(run):
    res, _ = run
    assert res["steps"] == STEPS and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "M metrics/s" and res["higher_is_better"] is True and res["dtype"] == "u64"
    for leg in ("e2e", "route_pack", "regroup"):
        assert leg not in res
    assert res["verify"] is None and res["cpu_baseline"] is None
    assert "achieved" not in res["roofline"]["read_ceiling"]


def test_dump_equals_oracle(run, pkg, oracle):
    import bench

    _, out = run
    files = sorted(os.listdir(out))
    assert files == ["counts.npy", "record_length.npy", "record_offset.npy", "record_route.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 * 10**6

    _, batch_bytes, lens, p_inv, shards, seed0, _ = bench.CONFIGS["c2"]
    recs, counts = [], []
    for b in range(NB):   # bench.py's batches of rank 0
        s = pkg.gen_stream(batch_bytes, lens, seed=seed0 + 65_537 * b, p_invalid=p_inv)
        r, _, n = oracle.route(s.data, shards, [1] * shards)
        assert n == s.n_lines
        recs.append(r)
        counts.append(n)
    flat = np.concatenate(recs)
    assert flat.size > bench.DUMP_SAMPLE   # the sampled path
    flat = flat[np.sort(np.random.default_rng(bench.DUMP_SEED).choice(flat.size, bench.DUMP_SAMPLE, replace=False))]
    assert arrs["counts"].tolist() == counts
    assert np.array_equal(arrs["record_offset"], flat["offset"].astype(np.float64))
    assert np.array_equal(arrs["record_length"], flat["length"].astype(np.float32))
    assert np.array_equal(arrs["record_route"], flat["route"].astype(np.float32))
