"""CPU tests of the SN-GAN discriminator: the spectral-norm oracle (power iteration, normalised
weight, projected gradient), the ``--d_spectral_norm`` / ``--d_batch_norm`` switches, the
reference engine in all four combinations, checkpoints, a 2-rank gloo run and -- on dry-run HIP
engines -- where every schedule records the ``sn_project`` / ``sn_power`` ops, hazard-free."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig, config_from_flags
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")


def small(d_bn=True):
    return DCGANConfig(output_size=28, c_dim=1, d_bn=d_bn)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("DCGAN_D_SPECTRAL_NORM", "DCGAN_D_BATCH_NORM"):
        monkeypatch.delenv(k, raising=False)


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


# ------------------------------------------------------------------ 1. the oracle
def _rank1_plus_noise(dtype):
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(1600, generator=g, dtype=torch.float64), torch.randn(128, generator=g, dtype=torch.float64)
    W = torch.outer(a, b)
    W = W + 0.01 * W.abs().mean() * torch.randn(1600, 128, generator=g, dtype=torch.float64)
    u = torch.randn(128, generator=g, dtype=torch.float64)
    return W.to(dtype), (u / u.norm()).to(dtype)


def test_power_iteration_converges_to_the_spectral_norm():
    """Rank-1 matrix + 1 % Gaussian noise, [1600, 128]: the second singular value is ~1e-3 of the
    first, so the iteration's error falls by ~1e-6 per step and 20 steps are exact to rounding.
    fp64: within 1e-12 of torch.linalg.matrix_norm(W, 2) (checked first: the method converges).
    fp32: within K * 2^-24 = 9.5e-5 relative, the worst-case forward error of an fp32 dot product
    of K = 1600 terms (the longest reduction of a step)."""
    W, u = _rank1_plus_noise(torch.float64)
    exact = torch.linalg.matrix_norm(W, 2)
    for _ in range(20):
        u, v, s = R.sn_power(W, u)
    assert abs(float(s / exact) - 1.0) < 1e-12
    assert abs(float(u.norm()) - 1.0) < 1e-12 and abs(float(v.norm()) - 1.0) < 1e-12
    assert abs(float(v @ W @ u / exact) - 1.0) < 1e-12  # sigma = v^T W u
    W32, u32 = _rank1_plus_noise(torch.float32)
    for _ in range(20):
        u32, v32, s32 = R.sn_power(W32, u32)
    assert s32.dtype == torch.float32 and not s32.requires_grad
    assert abs(float(s32.double() / exact) - 1.0) < 1600 * 2.0 ** -24


@pytest.mark.parametrize("K,C", [(75, 64), (2048, 1)])
def test_projected_gradient_is_autograd_of_the_normalised_weight(K, C):
    g = torch.Generator().manual_seed(K)
    W = (torch.randn(K, C, generator=g, dtype=torch.float64) * 0.02).requires_grad_(True)
    u0 = torch.randn(C, generator=g, dtype=torch.float64)
    u, v, s = R.sn_power(W.detach(), u0 / u0.norm())
    G = torch.randn(K, C, generator=g, dtype=torch.float64)
    (oracle,) = torch.autograd.grad((W / (v @ W @ u) * G).sum(), W)
    assert rel(R.sn_project(G, W.detach(), u, v, s), oracle) < 1e-12
    (through,) = torch.autograd.grad((R.spectral_normalize(W, u, v) * G).sum(), W)
    assert rel(through, oracle) < 1e-14
    # the projection removes the component along W: <dL/dW, W> = 0 (W / sigma is scale-invariant)
    assert abs(float((oracle * W.detach()).sum())) < 1e-12 * float(oracle.norm() * W.detach().norm())


def test_all_zero_weight_stays_finite():
    W = torch.zeros(75, 64)
    u0 = torch.full((64,), 0.125)
    u, v, s = R.sn_power(W, u0)
    assert float(s) == pytest.approx(1e-12) and not u.any() and not v.any()
    Wr = W.clone().requires_grad_(True)
    hat = R.spectral_normalize(Wr, u, v)
    (g,) = torch.autograd.grad(hat.sum(), Wr)
    for t in (u, v, s, hat, g, R.sn_project(torch.ones(75, 64), W, u, v, s)):
        assert bool(torch.isfinite(t).all())


def test_fresh_u_is_drawn_in_d_variables_order():
    cfg = small()
    shapes = cfg.d_sn_weights()
    assert [n for n, _, _ in shapes] == [n for n, _, _ in cfg.d_variables() if n.endswith("/w") or n.endswith("/Matrix")]
    assert shapes[0] == ("d_h0_conv/w", 25, 64) and shapes[-1] == (cfg.d_lin_name + "/Matrix", cfg.d_lin_in, 1)
    us = R.sn_init_u(shapes, 11)
    gen = torch.Generator().manual_seed(11)
    for name, _, C in shapes:
        u = torch.randn(C, generator=gen)
        assert torch.equal(us[name], u / u.norm())
    m = DCGAN(cfg, seed=11)
    sn = m.enable_d_spectral_norm(11)
    for name, K, C in shapes:
        u, v, s = R.sn_power(m.d[name].reshape(K, C), us[name])
        assert torch.equal(sn.u[name], u) and torch.equal(sn.v[name], v) and torch.equal(sn.sigma[name], s.reshape(1))


# ------------------------------------------------------------------ 2. switches
def test_flags_parse_and_defaults():
    fl = F.parse_flags([])
    assert fl.d_spectral_norm is False and fl.d_batch_norm is True
    assert config_from_flags(fl).d_bn is True
    fl = F.parse_flags(["--gan_loss=hinge", "--d_spectral_norm", "--nod_batch_norm"])
    assert fl.d_spectral_norm is True and fl.d_batch_norm is False and fl.gan_loss == "hinge"
    assert fl.explicitly_set("d_spectral_norm") and fl.explicitly_set("d_batch_norm")
    cfg = config_from_flags(fl)
    assert cfg.d_bn is False and cfg.d_bn_layers() == [] and all(L.bn is None for L in cfg.d_layers())
    assert not [n for n, _, _ in cfg.d_variables() if n.startswith("d_bn")]
    fl = F.parse_flags(["--nod_spectral_norm", "--d_batch_norm=true"])
    assert fl.d_spectral_norm is False and fl.d_batch_norm is True
    helps = {n: h for n, _, _, h in F.ALL_FLAGS}
    for n in ("d_spectral_norm", "d_batch_norm"):
        assert "--gan_loss=hinge --d_spectral_norm --nod_batch_norm" in helps[n]
    assert "layer 0 and the head" in helps["d_spectral_norm"]


def test_flags_pprint_shows_the_switches():
    import pprint
    text = pprint.pformat(F.parse_flags(["--d_spectral_norm"]).__flags)
    assert "'d_spectral_norm': True" in text and "'d_batch_norm': True" in text


def test_environment_defaults(monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    assert DCGANConfig().d_bn is True and ReferenceEngine(small(), 2, CPU).d_spectral_norm is False
    monkeypatch.setenv("DCGAN_D_SPECTRAL_NORM", "1")
    monkeypatch.setenv("DCGAN_D_BATCH_NORM", "0")
    assert DCGANConfig().d_bn is False and DCGANConfig(d_bn=True).d_bn is True  # an explicit value wins
    assert ReferenceEngine(small(), 2, CPU).d_spectral_norm is True
    assert ReferenceEngine(small(), 2, CPU, d_spectral_norm=False).model.d_sn is None
    assert HipEngine(small(), 2, CPU, dry_run=True, graph=False).d_spectral_norm is True
    assert HipEngine(small(), 2, CPU, dry_run=True, graph=False, d_spectral_norm=False).model.d_sn is None
    assert build_engine(small(), 2, CPU, engine="reference").d_spectral_norm is True
    monkeypatch.setenv("DCGAN_D_SPECTRAL_NORM", "perhaps")
    with pytest.raises(ValueError):
        ReferenceEngine(small(), 2, CPU)


@pytest.mark.parametrize("bad", ["perhaps", 2, 0.5, None])
def test_bad_switch_is_rejected_everywhere(bad):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    with pytest.raises(ValueError):
        R.check_spectral_norm(bad)
    with pytest.raises(ValueError):
        ReferenceStep(DCGAN(small()), d_spectral_norm=bad)
    if bad is not None:  # (None = "take the environment's default" for the engines)
        with pytest.raises(ValueError):
            ReferenceEngine(small(), 2, CPU, d_spectral_norm=bad)
        with pytest.raises(ValueError):
            HipEngine(small(), 2, CPU, dry_run=True, graph=False, d_spectral_norm=bad)
        with pytest.raises(ValueError):
            SC.check(small(), 2, d_spectral_norm=bad)
    for ok in (True, False, 0, 1, "1", "false"):
        assert R.check_spectral_norm(ok) in (True, False)


def test_sharded_update_with_spectral_norm_raises(monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    with pytest.raises(ValueError, match="DCGAN_DDP_SHARD"):
        HipEngine(DCGANConfig(), 4, CPU, world=2, dry_run=True, graph=False, d_spectral_norm=True)
    assert HipEngine(DCGANConfig(), 4, CPU, world=2, dry_run=True, graph=False)._sharded()  # off: untouched


def test_fresh_state_on_a_dry_run_engine():
    """A checkpoint without SN keys applied to a dry-run (CPU) engine: reset_d_sn needs no GPU."""
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    eng = HipEngine(small(False), 2, CPU, dry_run=True, graph=False, d_spectral_norm=True, seed=4)
    before = eng.model.d_sn.flat.clone()
    eng.model.d_sn.flat.zero_()
    eng.reset_d_sn()
    assert torch.equal(eng.model.d_sn.flat, before)
    assert HipEngine(small(), 2, CPU, dry_run=True, graph=False, seed=4, z_seed=9).z_seed == 9
    assert HipEngine(small(), 2, CPU, dry_run=True, graph=False, seed=4).z_seed == 4


# ------------------------------------------------------------------ 3. reference engine
def _real(B, cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=g) * 2 - 1


@pytest.mark.parametrize("sn", [False, True])
@pytest.mark.parametrize("bn", [True, False])
def test_reference_step_three_steps(sn, bn):
    cfg = small(bn)
    B = 4
    real = _real(B, cfg)
    m = DCGAN(cfg, seed=3)
    st = ReferenceStep(m, d_spectral_norm=sn, seed=3)
    assert (m.d_sn is not None) == sn and (m.d_bn.flat.numel() == 0) == (not bn)
    today = None
    if not sn and bn:  # both at their defaults: today's step, bit for bit
        mt = DCGAN(DCGANConfig(output_size=28, c_dim=1), seed=3)
        today = ReferenceStep(mt)
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        z = torch.rand(B, cfg.z_dim, generator=g) * 2 - 1
        if sn:  # 1. forward / backward read W_t / sigma of the state left by step t-1
            with torch.no_grad():
                exp = st.forward_losses(real, z, update_ema=False)
                Pd = m.d_sn_weights()
                for name, K, C in m.d_sn.shapes:
                    assert torch.allclose(Pd[name].reshape(K, C), m.d[name].reshape(K, C) / m.d_sn.sigma[name],
                                          rtol=1e-5, atol=0)
            u_t = {n: m.d_sn.u[n].clone() for n, _, _ in m.d_sn.shapes}
        L = st.step(real, z)
        assert all(np.isfinite(v) for v in L.values())
        if sn:
            assert L["d_loss"] == pytest.approx(float(exp["d_loss"]), rel=1e-6)
            # 4. after Adam(D): one power step on W_{t+1} from the stored u
            for name, K, C in m.d_sn.shapes:
                u, v, s = R.sn_power(m.d[name].reshape(K, C), u_t[name])
                assert torch.equal(m.d_sn.u[name], u) and torch.equal(m.d_sn.v[name], v)
                assert torch.equal(m.d_sn.sigma[name], s.reshape(1))
        if today is not None:
            Lt = today.step(real, z)
            assert Lt == L and torch.equal(mt.d.flat, m.d.flat) and torch.equal(mt.g.flat, m.g.flat)
            assert torch.equal(mt.d_bn.flat, m.d_bn.flat)
    assert st.global_step == 3 and m.d_bn.steps.tolist() == [3.0, 3.0]


def test_reference_gradient_is_the_projected_one():
    """ReferenceStep's D gradients with SN == the projection of the gradients w.r.t. W / sigma."""
    cfg = small(False)
    m = DCGAN(cfg, seed=2)
    st = ReferenceStep(m, d_spectral_norm=True, seed=2)
    real, z = _real(4, cfg), torch.rand(4, cfg.z_dim, generator=torch.Generator().manual_seed(2)) * 2 - 1
    _, gd, _ = st.compute_grads(real, z, update_ema=False)
    got = m.d.like()
    got.flat.copy_(gd)
    hat = {k: v.detach().clone().requires_grad_(True) for k, v in m.d_sn_weights().items()}
    out = ReferenceStep(m).forward_losses(real, z, Pd=hat, update_ema=False)
    names = [n for n, _, _ in m.d_sn.shapes]
    ghat = torch.autograd.grad(out["d_loss"], [hat[n] for n in names])
    for (name, K, C), G in zip(m.d_sn.shapes, ghat):
        exp = R.sn_project(G.reshape(K, C), m.d[name].reshape(K, C), m.d_sn.u[name], m.d_sn.v[name], m.d_sn.sigma[name])
        assert rel(got[name], exp) < 1e-5, name


# ------------------------------------------------------------------ 4. checkpoints
def _engine(sn, bn, seed=5, steps=2):
    eng = ReferenceEngine(small(bn), 4, CPU, seed=seed, d_spectral_norm=sn)
    eng.set_batch(_real(4, small(bn)))
    for _ in range(steps):
        eng.train_step()
    return eng


def test_checkpoint_round_trip(tmp_path):
    on = _engine(True, False)
    st = CK.collect_state(on)
    sn_keys = [k for k in st if "/sn_" in k]
    assert sn_keys == [n + suf for n, _, _ in on.cfg.d_sn_weights() for suf in ("/sn_u", "/sn_v", "/sn_sigma")]
    assert list(st)[-len(sn_keys):] == sn_keys
    assert st["d_h1_conv/w/sn_u"].shape == (128,) and st["d_h1_conv/w/sn_v"].shape == (1600,)
    assert st["d_h1_conv/w/sn_sigma"].shape == (1,)
    # a BN-free D: no d_bn* variables or moving averages, the update count is still written
    assert not [k for k in st if k.startswith("d_bn") and k != CK.BN_STEPS_KEYS[1]] and CK.BN_STEPS_KEYS[1] in st
    off = _engine(False, True)
    st_off = CK.collect_state(off)
    assert not [k for k in st_off if "/sn_" in k] and "d_bn1/gamma" in st_off
    # save -> a fresh engine with another seed -> load: exact, without iterating
    mgr = CK.CheckpointManager(str(tmp_path / "on"), save_secs=0)
    mgr.save(on)
    fresh = ReferenceEngine(small(False), 4, CPU, seed=9, d_spectral_norm=True)
    assert not torch.equal(fresh.model.d_sn.flat, on.model.d_sn.flat)
    info = mgr.restore_latest(fresh)
    assert info["d_sn"] == "loaded" and info["global_step"] == 2
    assert torch.equal(fresh.model.d_sn.flat, on.model.d_sn.flat) and torch.equal(fresh.model.d.flat, on.model.d.flat)
    fresh.z_gen.set_state(on.z_gen.get_state())
    fresh.set_batch(_real(4, small(False)))
    on.train_step()
    fresh.train_step()
    assert fresh.last_losses() == on.last_losses() and torch.equal(fresh.model.d.flat, on.model.d.flat)
    assert torch.equal(fresh.model.d_sn.flat, on.model.d_sn.flat)
    # a checkpoint written without SN: a fresh state on the loaded weights, and info says so
    pre = _engine(False, False)
    mgr_pre = CK.CheckpointManager(str(tmp_path / "pre"), save_secs=0)
    mgr_pre.save(pre)
    fresh2 = ReferenceEngine(small(False), 4, CPU, seed=9, d_spectral_norm=True)
    info = mgr_pre.restore_latest(fresh2)
    assert "initialised from the loaded weights" in info["d_sn"]
    assert torch.equal(fresh2.model.d.flat, pre.model.d.flat)
    exp = DCGAN(small(False), seed=9)
    exp.d.flat.copy_(pre.model.d.flat)
    assert torch.equal(fresh2.model.d_sn.flat, exp.enable_d_spectral_norm(9).flat)
    # SN keys into an engine without SN: ignored
    fresh3 = ReferenceEngine(small(False), 4, CPU, seed=9)
    info = mgr.restore_latest(fresh3)
    assert "d_sn" not in info and fresh3.model.d_sn is None


def test_bn_and_bn_free_checkpoints_cross_load(tmp_path):
    bn = _engine(False, True)
    mgr = CK.CheckpointManager(str(tmp_path / "bn"), save_secs=0)
    mgr.save(bn)
    free = ReferenceEngine(small(False), 4, CPU, seed=9)
    info = mgr.restore_latest(free)  # the d_bn* keys are extra: ignored
    assert info["global_step"] == 2 and torch.equal(free.model.d["d_h2_conv/w"], bn.model.d["d_h2_conv/w"])
    mgr2 = CK.CheckpointManager(str(tmp_path / "free"), save_secs=0)
    mgr2.save(_engine(False, False))
    with pytest.raises(KeyError, match="d_bn1"):
        mgr2.restore_latest(ReferenceEngine(small(True), 4, CPU, seed=9))


# ------------------------------------------------------------------ 5. schedules (dry-run HIP engines)
def _dry(dtype="bf16", world=1, schedule=None, timing=False, sn=True, bn=True, cfg=None, wire="fp32"):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    cfg = cfg or small(bn)
    eng = HipEngine(cfg, 4, CPU, dtype=dtype, world=world, schedule=schedule, dry_run=True, graph=False,
                    allreduce_dtype=wire, d_spectral_norm=sn)
    if timing:
        eng._timing = True
        eng._build_updates()
    return eng


def _names(prog):
    return [prog.op_info(i)[0] for i in range(prog.size())]


POWER = ["sn_power.wu", "sn_power.wtv", "sn_power.colsum", "sn_power.apply"]
CASES = [(1, None, False), (1, None, True), (1, "serial", False)] + [
    (w, s, False) for w in (2, 4, 8) for s in (None, "ddp", "serial")]


def _check_positions(eng):
    cfg = eng.cfg
    top = cfg.d_layers()[-1].name
    # projection: behind the launch that finalises each weight gradient; the top layer's (with the
    # head's) before the D chain's first cut
    b = _names(eng.progB)
    proj = [i for i, n in enumerate(b) if n.endswith(".dot")]
    assert [b[i] for i in proj] == ["sn_project.%s.dot" % L.name for L in reversed(cfg.d_layers())]
    for i in proj:
        layer = b[i].split(".")[1]
        assert b[i + 1] == "sn_project.%s.project" % layer
        assert "wgrad" in b[i - 1] and b[i - 1].startswith(layer), (b[i - 1], b[i])
        g = eng.grad_d[layer + "/w"]
        acc = [tuple(a) for a in eng.progB.op_info(i + 1)[4]]
        assert (g.data_ptr(), 4 * g.numel(), True) in acc
        if layer == top:
            assert i + 2 == eng._b_split
            h = eng.grad_d[cfg.d_lin_name + "/Matrix"]
            assert (h.data_ptr(), 4 * h.numel(), True) in acc
    # power step: once, right behind the last Adam launch over D, before step_end
    c = _names(eng.progC)
    k = c.index("sn_power.wu")
    assert c[k:k + 4] == POWER and c.count("sn_power.wu") == 1
    assert c[k - 1] in ("adam_d", "adam_gd") or (c[k - 1] == "ema_g" and c[k - 2] == "adam_gd")
    if "step_end" in c:
        assert k + 3 < c.index("step_end")
    assert not [n for n in _names(eng.progA) + _names(eng.progW) if n.startswith("sn_")]
    # load / init: the mirrors, then the normalised copies from the stored state
    assert _names(eng.progCast)[-1] == "sn_copy"
    wr = [tuple(a) for a in eng.progCast.op_info(eng.progCast.size() - 1)[4] if a[2]]
    es = 4 if eng.f32 else 2
    assert (eng.sn_head.data_ptr(), 4 * eng.sn_head.numel(), True) in wr
    assert (eng.wbf_d[top + "/w"].data_ptr(), es * eng.wbf_d[top + "/w"].numel(), True) in wr
    assert any(t.data_ptr() == eng.model.d_sn.flat.data_ptr() for t in eng.sync_check_tensors())


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("world,schedule,timing", CASES)
def test_schedules_have_no_stream_hazards(dtype, world, schedule, timing, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    for sn, bn in ((True, True), (True, False), (False, False)):
        eng = _dry(dtype, world, schedule, timing, sn=sn, bn=bn)
        assert eng._schedule() == (schedule or ("fused" if world == 1 and not timing else "concurrent"))
        hz, n = SC.check_engine(eng)
        assert n > 60 and hz == [], "%s\n%s" % ((sn, bn), "\n".join(map(str, hz[:10])))
        if sn:
            _check_positions(eng)
            off = _dry(dtype, world, schedule, timing, sn=False, bn=bn)
            assert [x for x in eng.op_names() if not x.startswith("sn_")] == off.op_names()
            assert eng.kernel_count() == off.kernel_count() + 4 + 2 * len(eng.cfg.d_layers())
            assert (eng.wbf_d is not eng.model.d) and (off.wbf_d is off.model.d) == (dtype == "fp32")
        else:
            assert eng.model.d_sn is None and eng.sn_head is None
            assert not [x for x in eng.op_names() + _names(eng.progCast) if x.startswith("sn_")]
            assert not [x for x in eng.op_names() if x.startswith("d_bn")]


@pytest.mark.parametrize("size", [64, 128])
def test_larger_models_and_the_checker_entry_point(size, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    for bn in (True, False):
        cfg = DCGANConfig(output_size=size, d_bn=bn)
        for world, wire in ((1, "fp32"), (2, "bf16")):
            s, hz, n = SC.check(cfg, 4, "bf16", world, None, False, allreduce_dtype=wire, d_spectral_norm=True)
            assert hz == [] and n > 100
        _check_positions(_dry(cfg=cfg, world=2))


def test_checker_finds_a_power_step_in_front_of_adam_d(monkeypatch):
    """A planted race: the power step's launches on another stream than Adam(D)."""
    eng = _dry(dtype="fp16")
    orig = eng._run_fused

    def racy(ex, cs):
        run = ex.run

        def split(prog, streams, begin=0, end=-1):
            if prog is eng.progC:
                names = _names(prog)
                k = names.index("sn_power.wu")
                run(prog, streams, 0, k)
                run(prog, [ex.alt[1], ex.alt[1]], k, k + 4)
                run(prog, streams, k + 4, -1)
            else:
                run(prog, streams, begin, end)
        ex.run = split
        try:
            orig(ex, cs)
        finally:
            ex.run = run
    monkeypatch.setattr(eng, "_run_fused", racy)
    hz, _ = SC.check_engine(eng)
    assert any("sn_power" in h.a or "sn_power" in h.b for h in hz)


# ------------------------------------------------------------------ 6. two ranks (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    from distributed_tensorflow_for_dcgan_amd.parallel import dist as D
    D.init_distributed(world, rank, CPU)
    cfg = small(False)
    eng = ReferenceEngine(cfg, 4, CPU, seed=rank * 100, rank=rank, world=world, d_spectral_norm=True)
    eng.set_batch(_real(4, cfg, seed=10 + rank))  # different seeds and batches: the broadcast and the all-reduce fix it
    for _ in range(2):
        eng.train_step()
    eng.sync_bn_state()  # (an empty d_bn state)
    ok = D.params_in_sync(eng.sync_check_tensors(), CPU)
    torch.save({"d": eng.model.d.flat, "g": eng.model.g.flat, "sn": eng.model.d_sn.flat, "sync": ok},
               os.path.join(out_dir, "r%d.pt" % rank))
    D.shutdown()


def test_two_ranks_stay_bit_identical(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(tmp_path / ("r%d.pt" % r), weights_only=True) for r in (0, 1))
    assert a["sync"] and b["sync"]
    for k in ("d", "g", "sn"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["sn"].abs().sum()) > 0
