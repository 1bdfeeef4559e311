"""bench.py's line and its --dump-outputs: a plain run times only the headline passes, --full adds the legs that take runs of their own, and
what the last timed pass computed is written as DIR/<name>.npy - the same files from two runs with the same arguments."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """small outputs are written whole in their shapes (integers and complex values as float32, float64 kept, integers beyond 2^24 as
    float64); past the byte budget every output keeps the same share of its elements at the same seeded, sorted positions, run after run"""
    bench = _bench_module()
    idx = torch.randint(0, 256, (4, 10))
    bench.dump_outputs({"indices": idx, "c": torch.randn(3, dtype=torch.complex64), "d": torch.rand(2, dtype=torch.float64),
                        "wide": torch.tensor([2 ** 30 + 1, 1])}, str(tmp_path / "small"))
    got = {f[:-4]: np.load(tmp_path / "small" / f) for f in os.listdir(tmp_path / "small")}
    assert sorted(got) == ["c", "d", "indices", "wide"]
    assert got["indices"].dtype == np.float32 and np.array_equal(got["indices"], idx.numpy())
    assert got["c"].dtype == np.float32 and got["c"].shape == (3, 2)
    assert got["d"].dtype == np.float64 and got["wide"].dtype == np.float64 and got["wide"][0] == 2 ** 30 + 1

    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    x = torch.arange(3000).reshape(30, 100)
    for run in ("a", "b"):
        bench.dump_outputs({"x": x, "y": x.double() / 2}, str(tmp_path / run))
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    y = np.load(tmp_path / "a" / "y.npy")
    assert a.ndim == 1 and 0 < a.size and 4 * a.size + 8 * y.size <= 4000
    assert np.array_equal(a, b) and (np.diff(a) > 0).all()             # positions: the same in both runs, sorted, each once
    assert np.array_equal(y, a[:y.size] / 2)                            # the same positions in every output


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    """a plain run: exactly --steps timed passes, ms_per_step consistent with value, none of the --full keys; the dump holds the generated
    classes and their mu-law expansion, identical from two runs with the same arguments"""
    from oracle import torch_ref as O
    args = ("--workload", "wavenet_cfg2", "--gpus", "1", "--steps", "3", "--warmup", "1", "--seconds", "0.05")
    lines = [_run_bench(*args, "--dump-outputs", str(tmp_path / run)) for run in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        units = line["config"]["clips_per_gpu"] * line["config"]["generated_samples_per_clip"]
        assert abs(line["value"] - units / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        assert not {"roofline", "cpu_baseline", "strong_scaling", "other_workloads"} & set(line)
    a = {f: np.load(tmp_path / "a" / f"{f}.npy") for f in ("indices", "audio")}
    b = {f: np.load(tmp_path / "b" / f"{f}.npy") for f in ("indices", "audio")}
    cfg = lines[0]["config"]
    assert a["indices"].shape == (cfg["clips_per_gpu"], cfg["prompt_samples"] + cfg["generated_samples_per_clip"])
    assert a["indices"].dtype == np.float32 and a["audio"].dtype == np.float32
    assert all(np.array_equal(a[f], b[f]) for f in a)
    assert torch.equal(torch.from_numpy(a["audio"]), O.mulaw_expand(torch.from_numpy(a["indices"]).long()))


@pytest.mark.gpu
def test_full_line_adds_roofline_and_cpu_baseline():
    line = _run_bench("--workload", "wavenet_cfg2", "--gpus", "1", "--steps", "1", "--warmup", "1", "--seconds", "0.05", "--full", "--cpu-seconds", "1")
    assert line["roofline"]["achieved"] > 0
    assert line["cpu_baseline"]["matches_gpu_output"] is True
