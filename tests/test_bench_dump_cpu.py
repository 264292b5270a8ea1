"""CPU tests of bench.py --dump-outputs: the arrays of the largest dump the flags allow stay inside the stated bound, in float
only, and the flag is refused (before any GPU work) where there is no resident step to dump."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_largest_dump_is_bounded(tmp_path):
    import bench
    k, n_pc = 2000, 50                          # bench's defaults; f64 storage: the values sample at 8 bytes
    rows = bench.DUMP_SAMPLE // n_pc
    outputs = {"scores": np.zeros((rows, n_pc)), "components": np.zeros((k, n_pc)), "explained_variance_ratio": np.zeros(n_pc),
               "mean": np.zeros(k), "std": np.zeros(k), "selected_features": np.zeros(k), "x_values": np.zeros(bench.DUMP_SAMPLE)}
    rec = bench.dump_outputs(str(tmp_path / "out"), outputs)
    assert rec["bytes"] <= 64 << 20
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(f"{name}.npy" for name in outputs)
    for f in files:
        assert np.load(tmp_path / "out" / f).dtype in (np.float32, np.float64)
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= (64 << 20) + 4096


def test_dump_outputs_refused_with_backed(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backed", "--dump-outputs", str(tmp_path / "d")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=120)
    assert p.returncode == 2
    assert "--dump-outputs" in p.stderr.decode() and not p.stdout.decode().strip()
    assert not os.path.exists(tmp_path / "d")
