"""bench.py --dump-outputs: the files hold what the last timed step computed (checked against the CPU oracle on the batch that step
evaluated), two runs with the same arguments write the same files, and a --full run writes them too."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, B, STEPS, WARMUP = 64, 2, 6, 1


def run_bench(out, *extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(STEPS), "--warmup", str(WARMUP), "--settle", "3",
                        "--batch", str(B), "--size", str(N), "--no-cpu", "--dump-outputs", str(out), *extra],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    import bench
    from oracle.fem_oracle import Oracle
    line, got = run_bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert sorted(got) == ["energy", "grad_sumsq", "grad_u", "loss"]
    assert got["loss"].dtype == np.float32 and got["energy"].dtype == got["grad_sumsq"].dtype == np.float64
    assert got["grad_u"].dtype == np.float32 and got["grad_u"].shape == (B, 1, N, N)

    # the steps go through 4 batches in rotation: the last timed one evaluated batch (W + K - 1) % 4
    k = (WARMUP + STEPS - 1) % 4
    u, nu, f, bc = bench.make_inputs((B, 1, N, N), None, 1000 * k + 42)
    ur = u.clone().requires_grad_(True)
    ref = Oracle(domain_size=N, ngp_1d=3).energy(ur, nu, f, dirichlet=[(bc.float(), 0.0)], c=1.0)
    ref.backward()
    g = ur.grad.numpy()
    np.testing.assert_allclose(float(got["loss"]), float(ref.detach()), rtol=1e-5)
    np.testing.assert_allclose(got["grad_u"], g, rtol=1e-4, atol=1e-4 * np.abs(g).max())
    scale = 1.0 / (B * (N - 1) ** 2)                       # loss and gradient: the unscaled sums times 1 / (B * elements)
    np.testing.assert_allclose(float(got["energy"]) * scale, float(got["loss"]), rtol=1e-6)
    np.testing.assert_allclose(float(got["grad_sumsq"]), float(np.sum((got["grad_u"].astype(np.float64) / scale) ** 2)), rtol=1e-5)

    _, again = run_bench(tmp_path / "b")
    for name in got:
        assert np.array_equal(got[name], again[name]), name


def test_full_run_adds_side_fields_and_dumps_the_same(tmp_path):
    """A plain run stops after the timed steps; --full measures the side fields after them and still dumps the last timed step."""
    plain, a = run_bench(tmp_path / "a")
    full, b = run_bench(tmp_path / "b", "--full")
    assert not {"settle", "roofline", "steady_state"} & set(plain)
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[key] == full[key], key
    assert full["settle"] == 3 and full["steady_state"]["ms_per_step"] > 0 and full["roofline"]["kernel_avg_ms"] > 0
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
