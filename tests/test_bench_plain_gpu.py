"""bench.py without --full: the headline alone (set-up, warm-up, the timed steps, one JSON line), and --dump-outputs writing the
last timed step's match lists so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path, oracle_lib):
    from easysfm_amd import synth
    j = _run(tmp_path / "a")
    assert j["unit"] == "image-pairs/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["steps"] == 3
    assert j["value"] > 0 and abs(j["value"] - 300 / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    for side in ("ba", "config4", "config5", "orb", "hard", "cpu_baseline"):
        assert side not in j, side
    files = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(files) == {"pairs.npy", "match_counts.npy", "match_query_idx.npy", "match_train_idx.npy", "match_distance.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    counts = files["match_counts.npy"].astype(np.int64)
    assert len(counts) == len(files["pairs.npy"]) == 300 and counts.sum() == len(files["match_distance.npy"]) > 0
    # pair 0's list is the oracle's, bit for bit
    sets = synth.surf_like_sets(25, 4096, pool=16384, seed_base=1000)
    i, j0 = files["pairs.npy"][0].astype(np.int64)
    rq, rt, rd = oracle_lib.match_l2(sets[i], sets[j0], 0.5)
    n0 = counts[0]
    assert np.array_equal(files["match_query_idx.npy"][:n0], rq) and np.array_equal(files["match_train_idx.npy"][:n0], rt)
    assert np.array_equal(files["match_distance.npy"][:n0].view(np.uint32), rd.view(np.uint32))
    # same arguments, same inputs: a second run writes the same outputs
    _run(tmp_path / "b")
    for f, a in files.items():
        assert np.array_equal(np.load(tmp_path / "b" / f), a), f
