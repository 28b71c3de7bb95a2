"""bench.py on the GPU: a plain run prints the headline and nothing it does not need; --full adds the fresh-decisions,
cpu_baseline and random-access legs, and their checks of what the GPU wrote hold.  Small batches (64 pictures of 1080p,
one random-access segment): the driver's command line at work, not a measurement."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "ai1080p8", "--frames", "64"]
LEGS = ("fresh_decisions", "cpu_baseline", "random_access")


def _bench(extra, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone():
    d = _bench([], 300)
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and (d["steps"], d["warmup"]) == (2, 1)
    assert d["config"]["pictures_per_gpu"] == 64 and d["roofline"]["frac"] > 0
    assert not [k for k in LEGS if k in d]


def test_full_run_adds_the_legs():
    d = _bench(["--full", "--one-core-only", "--fresh-steps", "1", "--ra-segments", "1"], 600)
    assert d["value"] > 0
    fresh = d["fresh_decisions"]
    assert "error" not in fresh and fresh["value"] > 0 and fresh["gpu_pictures_identical"] is True
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["gpu_picture_0_identical"] is True and cb["gpu_pictures_identical"] is True
    ra = d["random_access"]
    assert "error" not in ra and ra["value"] > 0
