"""bench.py's command line: a plain run measures the headline only, --full turns every side line
back on with its old defaults, --dump-outputs writes the last timed step's results (CPU tests)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE_SWITCHES = ("no_dropin", "no_psnr_check", "no_psf", "no_planes", "no_scipy", "no_probe", "no_ppo",
                 "no_crop", "no_obs", "no_precision")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 3, False, None)
    assert a.cpu_sample == 0 and a.dbs_flips == 0
    assert all(getattr(a, k) for k in SIDE_SWITCHES)
    assert not a.no_pg and not a.no_gather          # the headline's own process group and metric gather stay


def test_full_keeps_every_side_line_and_its_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.cpu_sample == 20 and a.dbs_flips == 65536 and a.psf_steps == 200
    assert not any(getattr(a, k) for k in SIDE_SWITCHES)
    a = _parse(monkeypatch, "--full", "--no-psf", "--dbs-flips", "0", "--cpu-sample", "0")
    assert a.no_psf and a.dbs_flips == 0 and a.cpu_sample == 0 and not a.no_planes


def test_dump_outputs_writes_float64_npy(monkeypatch, tmp_path):
    import torch
    import bench
    B = 5
    step_out = (torch.arange(B, dtype=torch.float64) * 0.25, torch.full((B,), 9.5, dtype=torch.float64),
                torch.tensor([0, 1, 0, 1, 1], dtype=torch.uint8), torch.zeros(B, dtype=torch.uint8),
                torch.ones(B, dtype=torch.uint8))
    out = tmp_path / "dump" / "nested"
    bench.dump_outputs(str(out), step_out)
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in bench.STEP_OUT_NAMES)
    for name, t in zip(bench.STEP_OUT_NAMES, step_out):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (B,)
        assert np.array_equal(got, t.numpy().astype(np.float64))
    bench.dump_outputs(str(out), step_out, rank=3)            # other ranks never overwrite rank 0's files
    assert (out / "psnr.rank3.npy").exists() and len(os.listdir(out)) == 10
    a = _parse(monkeypatch, "--dump-outputs", str(out))
    assert a.dump_outputs == str(out)
