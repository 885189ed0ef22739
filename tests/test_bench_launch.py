"""bench.py's multi-rank launch: `python bench.py --gpus N`
without a launcher starts N ranks through one torch.distributed.run child,
relays rank 0's JSON line and checks its n_gpus.  Exercised on the CPU with
--dry-run (gloo ranks, no GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout, cwd=ROOT)


@pytest.mark.parametrize("n", [1, 2])
def test_gpus_n_launches_n_ranks(n):
    p = _run(["--gpus", str(n), "--dry-run", "--steps", "3", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout  # exactly one JSON line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 3 and out["dry_run"]


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """--dump-outputs keeps float32 / float64 arrays as they are and writes a
    fixed sorted sample of an array beyond the byte budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    a = np.arange(300, dtype=np.float32)  # 1200 B: whole
    b = np.arange(1000, dtype=np.float64)  # 8000 B: 250 of 1000 entries
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    got_a, got_b = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert got_a.dtype == np.float32 and np.array_equal(got_a, a)
    assert got_b.dtype == np.float64 and got_b.shape == (250,)
    assert np.all(np.diff(got_b) > 0) and np.all(np.isin(got_b, b))
    assert np.array_equal(got_b, np.load(tmp_path / "two" / "b.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    """A plain run (no --full) on the coarse mesh: --steps sets the timed
    steps, the line carries ms_per_step and none of the --full parts, and
    dst.npy is the FP64 vmult of the bench's inputs (against the operator
    called directly on the same inputs, 1e-12)."""
    import numpy as np
    import torch
    import glsamd
    import glsinputs as gi
    from helpers import deck, rel_err
    p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--nref", "0", "--settle-ms", "0",
              "--dump-outputs", str(tmp_path)])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["dtype"] == "f64" and out["unit"] == "DoF/s"
    assert out["value"] == pytest.approx(out["config"]["dofs"] / (out["ms_per_step"] * 1e-3))
    assert out["parity"] is None and out["cpu_baseline"] is None and out["companions"] is None
    got = np.load(tmp_path / "dst.npy")
    d = deck("input_hoffmann_3D_Re3900.json")
    mesh = d.mesh(0)
    cmask = mesh.constraint_mask(*d.boundary_descriptor())
    params, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(mesh.n_nodes, mesh.dim, d.u_max)
    op = glsamd.NavierStokesOperator(mesh, cmask, "f64")
    op.set_parameters(**params)
    op.set_linearization_point(u)
    op.set_previous_solution(gi.history(u, params["order"]), w)
    dst = op.initialize_dof_vector()
    op.vmult(dst, op._dev(gi.src_vector(mesh.n_dofs)))
    torch.cuda.synchronize()
    assert got.dtype == np.float64 and got.shape == (mesh.n_dofs,)
    assert rel_err(got, dst.cpu().numpy()) < 1e-12


def test_world_size_mismatch_fails():
    # a rank whose WORLD_SIZE differs from --gpus refuses to run
    p = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "1", "RANK": "0"})
    assert p.returncode != 0
