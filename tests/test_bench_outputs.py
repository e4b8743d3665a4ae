"""bench.py's plain run and --dump-outputs on a small job: the line carries the contract's keys and nothing of --full, the
dumped arrays are float64, small, consistent with one another, and the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--gbp", "0.02", "--lsize", "26"]


def _run(out_dir):
    r = subprocess.run([sys.executable, BENCH] + SMALL + ["--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_tables_outputs_and_repeats_them_exactly(gpu, tmp_path):
    import numpy as np
    dumps = []
    for i in range(2):
        line = _run(tmp_path / str(i))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert not {"cpu_baseline", "secondary", "flush_sweep", "end_to_end"} & set(line)
        assert line["repeats"]["n"] == 1
        files = sorted((tmp_path / str(i)).iterdir())
        assert [f.name for f in files] == ["digest.npy", "histo.npy", "sample_counts.npy", "sample_keys.npy", "stats.npy"]
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        dumps.append({f.name: np.load(f) for f in files})
    a, b = dumps
    for name in a:
        assert a[name].dtype == np.float64, name
        assert np.array_equal(a[name], b[name]), name
    unique, distinct, total, max_count, fed = a["stats.npy"]
    n_reads = int(round(0.02e9 / 150))
    assert total == fed == n_reads * 130 == line["config"]["total_kmers"] and distinct == line["config"]["distinct"]
    h = a["histo.npy"]
    assert h.sum() == distinct and (np.arange(len(h)) * h).sum() == total and max_count < len(h)
    digest = a["digest.npy"]
    assert digest[0] == distinct and digest[1] == 0 and digest[2] + digest[3] * 2 ** 32 == total
    keys, counts = a["sample_keys.npy"], a["sample_counts.npy"]
    assert keys.shape == (4096 * 130, 2) and counts.shape == (4096 * 130,)
    assert (keys == np.floor(keys)).all() and (keys >= 0).all() and (keys < 2 ** 32).all()
    assert (counts >= 1).all()          # an unfiltered count holds every k-mer of its input
