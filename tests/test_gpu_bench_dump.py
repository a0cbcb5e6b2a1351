"""bench.py without --full: exactly --steps timed steps, the headline line alone, and --dump-outputs writing what the last timed step computed — held against
the same evaluation made here through the binding (1/10-size problem, the bench's seed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_its_dumped_outputs(tmp_path):
    import torch
    import lvx
    import synth
    d = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--small", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "Mevals/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert not {"roofline", "kernel_ms", "kernel_ms_solo", "secondary", "cpu_baseline"} & set(out)   # side measurements come with --full only

    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(got) == {"gradient", "hessian_diag", "border_block", "border_gradient", "cost"}
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20

    P = synth.make_bench_problem(seed=4, n_imu=20_000, n_surfel=100_000, n_reproj=5_000, n_planes=200)   # bench.py --small, one GPU
    g = lvx.Context(0)
    lvx.load_problem(g, P, lvx.LOCK_LIDAR_TAU | lvx.LOCK_CAM_TAU)
    g.set_state(P["state0"])
    n = g.layout()["border_ld"]
    buf = torch.zeros(n * n + n + 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.evaluate_resident(lvx.EVAL_COST | lvx.EVAL_NORMAL_EQ)
    g.export_border(buf.data_ptr())
    g.synchronize()
    grad, diag = g.gradient()
    g.close()
    b = buf.cpu().numpy()
    assert b[-1] == 0.0

    def close(a, ref, rel):
        assert a.shape == ref.shape and np.abs(a - ref).max() <= rel * np.abs(ref).max()
    close(got["gradient"], grad, 1e-10)
    close(got["hessian_diag"], diag, 1e-10)
    close(got["border_block"], np.tril(b[:n * n].reshape(n, n)), 1e-10)
    close(got["border_gradient"], b[n * n:n * n + n], 1e-10)
    close(got["cost"], b[n * n + n:n * n + n + 1], 1e-12)
    assert got["cost"][0] == pytest.approx(out["config"]["cost"], rel=1e-12)
