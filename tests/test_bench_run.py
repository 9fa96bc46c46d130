r"""GPU: a plain `bench.py` run prints the headline line and nothing beyond it, and `--dump-outputs` writes what its last
timed step computed - the same clusters and centroids as the CPU oracle's fit of the same seeded rows."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    import torch
    from oracle_engine import OracleEngine

    from bblean_amd import BitBirch
    from bench import synth_fake_fps

    n = 30_000
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n-fps", str(n),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "fingerprints/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not {"cpu_baseline", "k1_roofline", "end_to_end", "other_workloads", "regressions"} & set(line)

    got = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert set(got) == {"assignments", "cluster_sizes", "centroids", "centroids_clusters"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    fps = synth_fake_fps(n, 1000, torch.device("cuda")).cpu().numpy()  # bench.py's seed: the very rows it clustered
    ora = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter", _engine_factory=OracleEngine).fit(fps)
    labels = ora.get_assignments()
    assert line["config"]["clusters"] == int(labels.max())
    assert np.array_equal(got["assignments"], labels.astype(np.float64))
    assert np.array_equal(got["cluster_sizes"], np.bincount(labels.astype(np.int64))[1:].astype(np.float64))
    cents = np.stack(ora.get_centroids())
    assert np.array_equal(got["centroids"], cents[got["centroids_clusters"].astype(np.int64) - 1].astype(np.float64))
