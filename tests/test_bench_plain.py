"""bench.py's plain run (the headline and nothing else) and --dump-outputs: the dump helpers on the host, then the plain
line, the dumped output against the CPU oracle, run-to-run identity and the per-rank files on the GPU."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

EXTRA_KEYS = ("checked", "split_bf16", "target_shape", "side_legs", "whole_model", "strong", "cpu_baseline")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_is_the_default_and_full_is_an_option(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_rows_fit_the_budget_and_do_not_change(bench):
    """Every workload's whole HR image, at every rank count's share of the budget: either all rows (None) or a sorted,
    duplicate-free, seeded sample of whole rows whose bytes fit."""
    for (_, _), (hu, wu), _ in bench.WORKLOADS.values():
        for world in (1, 2, 8):
            budget = bench.DUMP_BUDGET_BYTES // world
            row_bytes = 3 * wu * 4
            rows = bench.dump_rows(hu, row_bytes, budget)
            if rows is None:
                assert hu * row_bytes + 128 <= budget
                continue
            assert len(rows) * row_bytes + 128 <= budget and len(rows) < hu
            assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < hu
            assert np.array_equal(rows, bench.dump_rows(hu, row_bytes, budget))
    assert bench.dump_rows(1024, 3 * 1024 * 4, bench.DUMP_BUDGET_BYTES) is None        # c2 goes out whole


def test_dump_outputs_writes_float32_whole_or_sampled(bench, tmp_path, monkeypatch):
    out = torch.randn(1, 3, 40, 16)
    bench.dump_outputs(str(tmp_path / "a"), out, 0, 1)
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096 + 10 * 3 * 16 * 4)      # room for 10 rows
    bench.dump_outputs(str(tmp_path / "b"), out, 1, 1)
    got = np.load(tmp_path / "b" / "output.npy")
    rows = bench.dump_rows(40, 3 * 16 * 4, bench.DUMP_BUDGET_BYTES)
    assert got.shape == (1, 3, 10, 16) and np.array_equal(got, out.numpy()[:, :, rows])
    bench.dump_outputs(str(tmp_path / "c"), out, 1, 2)
    assert os.listdir(tmp_path / "c") == ["output_rank1.npy"]


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return env


def _one_line(r):
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def _plain(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=timeout, env=_env(), cwd=ROOT)
    return _one_line(r)


@pytest.mark.gpu
def test_plain_line_dump_matches_the_oracle_and_repeats(bench, tmp_path):
    """The plain default run: the headline fields, none of the --full extras, --steps steps timed; the dumped output is
    the timed c2 image (checked against the oracle on three row bands, as --full checks it) and a second run dumps the
    same bits."""
    res = _plain("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert res["metric"] == bench.METRIC["c2"] and res["unit"] == "Mpixels/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["steps"] == 3 and res["value"] > 0 and res["ms_per_step"] > 0
    assert abs(res["value"] - 1024 * 1024 / res["ms_per_step"] / 1e3) <= 0.01 * res["value"]
    assert not [k for k in EXTRA_KEYS if k in res]
    assert "NOT measured in this run" in res["roofline"]["traffic_source"]
    got = np.load(tmp_path / "a" / "output.npy")
    assert got.dtype == np.float32 and got.shape == (1, 3, 1024, 1024)

    import diinn_amd.synth as synth
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(123)
    feat = torch.randn((1, 64, 256, 256), device="cuda:0", generator=gen).cpu()
    err, ok = bench.check_band_rows(synth.decoder_state_dict(123), feat, 0, 256, (1024, 1024), torch.from_numpy(got), 0,
                                    [(0, 4), (510, 514), (1020, 1024)], "f32")
    assert ok and err <= 1e-4, err

    _plain("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(got, np.load(tmp_path / "b" / "output.npy"))


@pytest.mark.gpu
def test_plain_dump_of_a_large_output_is_a_sample_within_budget(bench, tmp_path):
    res = _plain("--workload", "tgt", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 1 and not [k for k in EXTRA_KEYS if k in res]
    f = tmp_path / "output.npy"
    assert os.path.getsize(f) <= bench.DUMP_BUDGET_BYTES
    got = np.load(f)
    rows = bench.dump_rows(4096, 3 * 4096 * 4, bench.DUMP_BUDGET_BYTES)
    assert got.dtype == np.float32 and got.shape == (1, 3, len(rows), 4096) and np.isfinite(got).all()


@pytest.mark.gpu
def test_plain_two_ranks_dump_one_file_per_rank(tmp_path):
    """The driver's N = 2 command without --full on the one-device test transport: the headline line only, and each rank's
    band of the last timed step in a file of its own."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(_env(), DIINN_BENCH_ONE_DEVICE="1", DIINN_BENCH_BACKEND="gloo", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c1", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["hr"] == [192, 96] and not [k for k in EXTRA_KEYS if k in res]
    bands = [np.load(tmp_path / f"output_rank{i}.npy") for i in range(2)]
    assert sorted(os.listdir(tmp_path)) == ["output_rank0.npy", "output_rank1.npy"]
    assert all(b.dtype == np.float32 and b.shape[:2] == (1, 3) and b.shape[3] == 96 for b in bands)
    assert sum(b.shape[2] for b in bands) == 192 and all(np.isfinite(b).all() for b in bands)
