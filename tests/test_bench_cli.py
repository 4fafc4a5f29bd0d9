"""bench.py's command line: ``--steps`` sets the timed steps, the JSON line carries ``ms_per_step``,
``--full`` is accepted, and ``--dump-outputs DIR`` writes the last step's outputs as .npy files
that are identical from run to run. Runs the reference engine on the CPU at a tiny shape."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"losses", "g_params", "d_params", "g_bn_state", "d_bn_state"}


def _env(cpu=True):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    if cpu:  # no visible GPU: the reference engine then runs on the CPU, bit-reproducibly
        env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DCGAN_DIST_BACKEND"):
        env.pop(k, None)
    return env


def _cmd(out_dir, *extra):
    return [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--engine", "reference", "--dtype", "fp32", "--output_size", "28", "--c_dim", "1", "--batch_size", "4",
            "--dump-outputs", str(out_dir)] + list(extra)


def test_bench_dump_outputs_and_full(tmp_path):
    procs = [subprocess.Popen(_cmd(tmp_path / d, *extra), env=_env(), cwd=ROOT, text=True,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for d, extra in (("a", ()), ("b", ("--full",)))]
    results = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
        lines = [l for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out
        results.append(json.loads(lines[0]))
    for res in results:  # --full adds nothing to the line's meaning
        assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
        assert res["unit"] == "images/sec" and res["higher_is_better"] is True and res["dtype"] == "fp32"
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same 3 timed steps of 4 images
        assert abs(res["value"] * res["ms_per_step"] / 1e3 / 4 - 1) < 1e-2
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == NAMES
    total = 0
    for name in NAMES:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all()
        assert np.array_equal(a, b), name  # same arguments -> same inputs -> same outputs
        total += a.nbytes
    assert total <= 64e6
    losses = np.load(tmp_path / "a" / "losses.npy")
    ll = results[0]["config"]["last_losses"]
    want = [ll[k] for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss")]
    assert np.allclose(losses, want, atol=1e-5)  # the JSON line rounds to 5 places


@pytest.mark.gpu
def test_bench_dump_outputs_hip_engine(tmp_path):
    """The HIP engine's dump also holds the generated batch (tanh range) and D's logits on
    [real | fake]; the losses match the JSON line."""
    env = _env(cpu=False)
    B = 16
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--batch_size", str(B), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["config"]["engine"] == "hip"
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == NAMES | {"generated", "logits"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["generated"].shape == (B * 64 * 64 * 3,) and np.abs(got["generated"]).max() <= 1.0
    assert got["generated"].std() > 0 and got["logits"].shape == (2 * B,)
    ll = res["config"]["last_losses"]
    want = [ll[k] for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss")]
    assert np.allclose(got["losses"], want, atol=1e-5)


def test_dump_outputs_samples_to_budget(tmp_path):
    """Arrays over the budget are cut to a common size as a fixed seeded sample; small ones and
    the total stay within the budget, and two dumps pick the same elements."""
    import bench  # (the repository root is on sys.path: tests/conftest.py)

    def ps(n):
        return types.SimpleNamespace(flat=torch.arange(n, dtype=torch.float32))

    eng = types.SimpleNamespace(
        model=types.SimpleNamespace(g=ps(1000), d=ps(300), g_bn=ps(10), d_bn=ps(20)),
        last_losses=lambda: dict(d_loss_real=1.0, d_loss_fake=2.0, g_loss=3.0, d_loss=4.0),
        fake=torch.ones(50, dtype=torch.bfloat16), logits=torch.zeros(8))
    bench.dump_outputs(eng, str(tmp_path / "a"), budget=2000)
    bench.dump_outputs(eng, str(tmp_path / "b"), budget=2000)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == NAMES | {"generated", "logits"}
    assert sum(a.nbytes for a in got.values()) <= 2000
    assert got["losses"].dtype == np.float64 and got["losses"].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert got["generated"].dtype == np.float32 and got["generated"].shape == (50,)
    assert got["g_bn_state"].shape == (10,) and got["d_bn_state"].shape == (20,) and got["logits"].shape == (8,)
    g, d = got["g_params"], got["d_params"]
    assert g.size == d.size < 300 and len(set(g.tolist())) == g.size and (np.diff(g) > 0).all()
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name
