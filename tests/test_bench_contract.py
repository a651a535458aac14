"""The bench.py driver contract: one JSON line, required fields, sane types.

The round driver invokes `python bench.py --gpus N --steps K --warmup W`
and parses rank 0's single JSON line — this test pins that contract so a
refactor cannot silently break the measurement harness.
"""

from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(
    importlib.util.find_spec("torch") is None,
    reason="bench.py needs torch (absent in the lint-only CI image)",
)
def test_bench_emits_contract_json_line():
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--mock", "1x8GiB", "--pods-per-gpu", "2"],
        cwd=REPO, capture_output=True, text=True, timeout=180,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line: {out.stdout!r}"
    d = json.loads(lines[0])

    assert d["metric"].startswith("pods/sec")
    assert isinstance(d["value"], (int, float)) and d["value"] > 0
    assert d["unit"] == "pods/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert isinstance(d["ms_per_step"], (int, float)) and d["ms_per_step"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["vs_baseline"] is None     # reference publishes no numbers
    assert d["data"] == "synthetic"
    cfg = d["config"]
    assert cfg["pods_allocated"] == 2 * 2 and cfg["pods_failed"] == 0
    for key in ("allocate_p50_ms", "allocate_p99_ms", "packing_pct_peak",
                "server_allocate_p50_ms", "plugin_rank_rss_mb"):
        assert isinstance(cfg[key], (int, float)), key


@pytest.mark.skipif(
    importlib.util.find_spec("torch") is None,
    reason="bench.py needs torch (absent in the lint-only CI image)",
)
def test_bench_full_and_dump_outputs(tmp_path):
    """--full keeps the one-line contract; --dump-outputs writes the last
    timed wave's per-pod Allocate results as float64 .npy arrays, the same
    from run to run.  Expected values follow from the inputs: 2 pods of
    8 // 2 = 4 GiB fill the single 8 GiB mock GPU, so both bind to GPU 0
    and packing peaks at 100%; the bench's Allocator has no memguard
    library configured (no limit env, no mount) and injects /dev/kfd plus
    the GPU's render and card nodes."""
    import numpy as np

    def run(outdir, *extra):
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--mock", "1x8GiB", "--pods-per-gpu", "2",
             "--dump-outputs", str(outdir), *extra],
            cwd=REPO, capture_output=True, text=True, timeout=180,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, f"expected exactly one JSON line: {out.stdout!r}"
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["config"]["pods_allocated"] == 3 * 2
        assert d["ms_per_step"] > 0
        return {p.stem: np.load(p) for p in outdir.glob("*.npy")}

    expected = {
        "requested_units": [4, 4],
        "bound": [1, 1],
        "gpu_index": [0, 0],
        "units_by_pod": [4, 4],
        "units_by_container": [4, 4],
        "units_by_dev": [8, 8],
        "visible_device_count": [1, 1],
        "memguard_limit_bytes": [-1, -1],
        "device_spec_count": [3, 3],
        "mount_count": [0, 0],
        "wave_summary": [2, 0, 100],
    }
    written = run(tmp_path / "a", "--full")
    assert set(written) == set(expected)
    for name, want in expected.items():
        assert written[name].dtype == np.float64, name
        assert written[name].tolist() == want, name
    assert sum(a.nbytes for a in written.values()) <= 64 << 20

    again = run(tmp_path / "b")
    assert set(again) == set(written)
    for name, arr in written.items():
        assert np.array_equal(arr, again[name]), name
