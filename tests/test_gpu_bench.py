"""bench.py end to end on the device, in fresh child processes: a plain run prints the headline line and nothing that needs runs of its
own; --full adds the roofline block of the profiled pass (--no-cpu-baseline keeps the oracle legs out, as the profiler scripts do)."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2", "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_only():
    out = _bench()
    for k in HEADLINE:
        assert k in out, k
    assert out["unit"] == "problem-iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 2 and out["warmup"] == 1
    B, nb = out["config"]["global_batch"], out["config"]["iterations_per_step"]
    assert out["value"] == pytest.approx(B * nb * 1e3 / out["ms_per_step"], rel=1e-9)
    assert not {"roofline", "cpu_baseline", "parity"} & set(out), sorted(out)


def test_full_run_adds_the_roofline():
    out = _bench("--full", "--no-cpu-baseline")
    for k in HEADLINE:
        assert k in out, k
    roof = out["roofline"]
    assert roof["bound"] == "hbm" and roof["achieved"] > 0 and roof["launches_per_step"]
    assert not {"cpu_baseline", "parity"} & set(out), sorted(out)
