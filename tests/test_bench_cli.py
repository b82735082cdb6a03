"""bench.py's two kinds of run: a plain run measures the headline alone; --full adds the objects that take runs of
their own (other states, the other arithmetic mode, the whole app run, the CPU baselines)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = {"dense_state", "developed_state", "app_figure", "app_run", "sustained", "fast_math", "cpu_baseline"}


def bench_line(*args):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--nx", "256", "--ny", "256"] + list(args),
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_help_lists_full():
    p = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "--full" in p.stdout


@pytest.mark.gpu
def test_plain_run_is_headline_only():
    d = bench_line("--steps", "5", "--warmup", "2")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d
    assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and d["config"]["result_finite"]
    assert not EXTRAS & set(d)


@pytest.mark.gpu
def test_full_run_adds_the_extra_objects():
    d = bench_line("--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert EXTRAS - {"cpu_baseline"} <= set(d) and "cpu_baseline" not in d
    for k in ("dense_state", "developed_state", "app_figure", "app_run", "sustained"):
        assert d[k]["value"] > 0 and d[k]["result_finite"], k
    assert d["fast_math"]["bubble"]["result_finite"] and d["fast_math"]["dense"]["result_finite"]
