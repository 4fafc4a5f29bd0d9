"""CPU tests of ``--d_steps`` (D-only sub-steps), ``--beta2`` and the per-network learning rates:
validation at every entry point, argument precedence, ``ReferenceStep.d_step`` against a hand-written
autograd step, the reference cycle, checkpoints, the CLI and -- on dry-run HIP engines -- the
recorded sub-step schedules (hazard-free, no G work, exactly one D update, a planted race found)."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.optim.adam import TFAdam
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_DDP_SHARD", "DCGAN_DDP_SCHEDULE",
       "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM", "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS", "DCGAN_D_UPDATE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def small(d_bn=True):
    return DCGANConfig(output_size=28, c_dim=1, d_bn=d_bn)


def _real(B, cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=g) * 2 - 1


def _z(B, cfg, seed):
    return torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _hip(cfg=None, **kw):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    kw.setdefault("graph", False)
    return HipEngine(cfg or small(), 4, CPU, dry_run=True, **kw)


# ------------------------------------------------------------------ 1. validation, precedence
def test_beta2_default_is_tf_adams():
    assert inspect.signature(TFAdam.__init__).parameters["beta2"].default == R.ADAM_BETA2
    fl = F.parse_flags([])
    assert (fl.d_steps, fl.beta2, fl.d_learning_rate, fl.g_learning_rate) == (1, R.ADAM_BETA2, 0.0, 0.0)


BAD = [dict(d_steps=0), dict(d_steps=17), dict(beta2=1.0), dict(lr_d=-1e-4), dict(lr_g=-1e-4)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_invalid_values_are_rejected_everywhere(bad, monkeypatch):
    (name, value), = bad.items()
    flag = {"d_steps": "d_steps", "beta2": "beta2", "lr_d": "d_learning_rate", "lr_g": "g_learning_rate"}[name]
    with pytest.raises(SystemExit):
        F.parse_flags(["--%s=%s" % (flag, value)])
    with pytest.raises(ValueError, match=flag if name.startswith("lr") else name):
        ReferenceStep(DCGAN(small(), seed=0), **bad)
    with pytest.raises(ValueError):
        ReferenceEngine(small(), 4, CPU, **bad)
    with pytest.raises(ValueError):
        _hip(**bad)
    with pytest.raises(ValueError):
        build_engine(small(), 4, CPU, engine="reference", **bad)
    env = {"d_steps": "DCGAN_D_STEPS", "beta2": "DCGAN_BETA2", "lr_d": "DCGAN_LR_D", "lr_g": "DCGAN_LR_G"}[name]
    monkeypatch.setenv(env, str(value))
    with pytest.raises(ValueError):
        ReferenceEngine(small(), 4, CPU)
    with pytest.raises(ValueError):
        _hip()


def test_valid_flags_parse():
    fl = F.parse_flags(["--d_steps=5", "--beta1=0", "--beta2=0.9", "--d_learning_rate=4e-4", "--g_learning_rate=1e-4"])
    assert (fl.d_steps, fl.beta1, fl.beta2, fl.d_learning_rate, fl.g_learning_rate) == (5, 0.0, 0.9, 4e-4, 1e-4)
    assert R.check_d_steps(16, 0.0, None, 0.0, 3e-4) == (16, 0.0, 3e-4, 3e-4)


def test_d_steps_conflicts_are_errors(monkeypatch):
    for sched in ("ddp", "serial"):
        with pytest.raises(ValueError, match="d_steps > 1.*%s" % sched):
            _hip(world=2, schedule=sched, d_steps=2)
        _hip(world=2, schedule=sched, d_steps=1)
    monkeypatch.setenv("DCGAN_DDP_SCHEDULE", "ddp")
    with pytest.raises(ValueError, match="d_steps > 1"):
        _hip(world=2, d_steps=2)
    monkeypatch.delenv("DCGAN_DDP_SCHEDULE")
    monkeypatch.setenv("DCGAN_SERIAL_DBWD", "1")
    with pytest.raises(ValueError, match="d_steps > 1"):
        _hip(d_steps=2)
    monkeypatch.delenv("DCGAN_SERIAL_DBWD")
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    with pytest.raises(ValueError, match="d_steps > 1.*DCGAN_DDP_SHARD"):
        _hip(world=2, d_steps=2)
    _hip(world=2, d_steps=1)


def test_an_explicit_argument_wins_over_the_environment(monkeypatch):
    monkeypatch.setenv("DCGAN_D_STEPS", "4")
    monkeypatch.setenv("DCGAN_BETA2", "0.9")
    monkeypatch.setenv("DCGAN_LR_D", "4e-4")
    monkeypatch.setenv("DCGAN_LR_G", "1e-4")
    for mk in (lambda **kw: ReferenceEngine(small(), 4, CPU, **kw), lambda **kw: _hip(**kw)):
        e = mk()
        assert (e.d_steps, e.opt_d.beta2, e.opt_g.beta2, e.opt_d.lr, e.opt_g.lr) == (4, 0.9, 0.9, 4e-4, 1e-4)
        e = mk(d_steps=2, beta2=0.99, lr_d=3e-4, lr_g=5e-5)
        assert (e.d_steps, e.opt_d.beta2, e.opt_g.beta2, e.opt_d.lr, e.opt_g.lr) == (2, 0.99, 0.99, 3e-4, 5e-5)
        assert float(e.opt_d.powers[1]) == pytest.approx(0.99)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    e = _hip(lr=3e-4)
    assert (e.d_steps, e.opt_d.beta2, e.opt_d.lr, e.opt_g.lr) == (1, R.ADAM_BETA2, 3e-4, 3e-4)
    assert len(e.d_ins) == 1 and e.d_ins[0] is e.d_in and e._sub == [] and e.progDU is None


# ------------------------------------------------------------------ 2. ReferenceStep.d_step
def _g_state(st):
    m = st.model
    out = [m.g.flat, st.opt_g.m.flat, st.opt_g.v.flat, st.opt_g.powers, m.g_bn.flat, m.g_bn.steps]
    if m.g_ema is not None:
        out.append(m.g_ema.flat)
    return [torch.as_tensor(t).clone() for t in out]


@pytest.mark.parametrize("sn,bn", [(False, True), (True, True), (True, False), (False, False)])
def test_d_step_is_a_hand_written_d_update_and_leaves_g_alone(sn, bn):
    cfg, B = small(bn), 4
    kw = dict(lr=2e-4, beta1=0.5, beta2=0.9, lr_d=3e-4, lr_g=1e-4, gan_loss="hinge", d_spectral_norm=sn, seed=3,
              g_ema_decay=0.99)
    a = ReferenceStep(DCGAN(cfg, seed=3), **kw)
    b = ReferenceStep(DCGAN(cfg, seed=3), **kw)  # the hand-written side: same state after one full step
    real0, real1, z0, z1 = _real(B, cfg, 1), _real(B, cfg, 2), _z(B, cfg, 1), _z(B, cfg, 2)
    a.step(real0, z0)
    b.step(real0, z0)
    assert torch.equal(a.model.d.flat, b.model.d.flat)
    g_before, step_before = _g_state(a), a.global_step
    d_bn_before, d_steps_before = a.model.d_bn.flat.clone(), torch.as_tensor(a.model.d_bn.steps).clone()
    losses = a.d_step(real1, z1)
    # G: parameters, slots, powers, BN moving averages and counts, EMA shadow, global step
    for x, y in zip(g_before, _g_state(a)):
        assert torch.equal(x, y)
    assert a.global_step == step_before
    # D's BN moving averages (both slots) and their counts moved, as in a full step
    if bn:
        assert not torch.equal(a.model.d_bn.flat, d_bn_before)
    assert torch.equal(torch.as_tensor(a.model.d_bn.steps), d_steps_before + 1)
    # the hand-written step on b: autograd of d_loss alone w.r.t. D, then TF-Adam(lr_d, beta1, beta2)
    m = b.model
    Pd = {k: v.detach().clone().requires_grad_(True) for k, v in m.d.tensors.items()}
    fake = m.generator(z1, train=True, update_ema=False)
    _, logits = m.discriminator(torch.cat([real1, fake], 0), groups=2, slots=(0, 1), train=True,
                                P=m.d_sn_weights(Pd) if sn else Pd, update_ema=False)
    d_real, d_fake, g_loss, d_loss = R.gan_losses(logits[:B], logits[B:], "hinge", 0.0)
    names = m.d.names()
    grads = torch.autograd.grad(d_loss, [Pd[n] for n in names], allow_unused=True)
    gflat = m.d.like()
    for n, g in zip(names, grads):
        if g is not None:
            gflat[n].copy_(g)
    w, mm, vv = m.d.flat.clone(), b.opt_d.m.flat.clone(), b.opt_d.v.flat.clone()
    b1p, b2p = float(b.opt_d.powers[0]), float(b.opt_d.powers[1])
    assert b1p == pytest.approx(0.25) and b2p == pytest.approx(0.81)
    with torch.no_grad():
        R.tf_adam_update(w, gflat.flat, mm, vv, b1p, b2p, 3e-4, 0.5, 0.9)
    assert torch.equal(a.model.d.flat, w) and torch.equal(a.opt_d.m.flat, mm) and torch.equal(a.opt_d.v.flat, vv)
    assert float(a.opt_d.powers[0]) == pytest.approx(0.125) and float(a.opt_d.powers[1]) == pytest.approx(0.729)
    assert losses["d_loss"] == pytest.approx(float(d_loss.detach())) and losses["g_loss"] == pytest.approx(float(g_loss.detach()))
    if sn:  # one power step on the new weights
        m.d.flat.copy_(w)
        m.d_sn.power_step_(m.d.tensors)
        assert torch.equal(a.model.d_sn.flat, m.d_sn.flat)


def test_reference_cycle_is_d_step_d_step_step():
    cfg, B = small(), 4
    eng = ReferenceEngine(cfg, B, CPU, seed=4, d_steps=3, beta2=0.9, d_spectral_norm=True)
    reals = [_real(B, cfg, 10 + k) for k in range(3)]
    for k in range(3):
        eng.set_batch(reals[k], k)
    with pytest.raises(ValueError):
        eng.set_batch(reals[0], 3)
    hand = ReferenceStep(DCGAN(cfg, seed=4), d_steps=3, beta2=0.9, d_spectral_norm=True, seed=4)
    zgen = torch.Generator().manual_seed(4 + 1)  # ReferenceEngine's z stream at rank 0
    for step in range(2):
        eng.train_step()
        zs = [torch.rand(B, cfg.z_dim, generator=zgen) * 2 - 1 for _ in range(3)]
        hand.d_step(reals[0], zs[0])
        hand.d_step(reals[1], zs[1])
        want = hand.step(reals[2], zs[2])
        assert eng.last_losses() == want  # the log line reports the full step's losses
        for x, y in ((eng.model.d.flat, hand.model.d.flat), (eng.model.g.flat, hand.model.g.flat),
                     (eng.opt_d.powers, hand.opt_d.powers), (eng.opt_g.powers, hand.opt_g.powers),
                     (eng.model.d_bn.flat, hand.model.d_bn.flat), (eng.model.g_bn.flat, hand.model.g_bn.flat),
                     (eng.model.d_sn.flat, hand.model.d_sn.flat)):
            assert torch.equal(x, y)
        assert eng.global_step == step + 1
    # D's powers advance d_steps times per training step, G's once
    assert float(eng.opt_d.powers[0]) == pytest.approx(0.5 ** 7) and float(eng.opt_g.powers[0]) == pytest.approx(0.5 ** 3)
    assert list(torch.as_tensor(eng.model.d_bn.steps)) == [6, 6] and list(torch.as_tensor(eng.model.g_bn.steps)) == [2]


def test_each_network_moves_by_its_own_learning_rate():
    """First Adam step from zero slots, one layer: m = (1 - b1) g, v = (1 - b2) g^2 and
    lr_t = lr sqrt(1 - b2) / (1 - b1), so dw = -lr g / (|g| + eps / sqrt(1 - b2))."""
    cfg, B = small(), 4
    lr_d, lr_g, b2 = 1e-3, 1e-4, 0.9
    st = ReferenceStep(DCGAN(cfg, seed=6), lr=5e-4, beta1=0.5, beta2=b2, lr_d=lr_d, lr_g=lr_g)
    assert (st.opt_d.lr, st.opt_g.lr) == (lr_d, lr_g)
    real, z = _real(B, cfg, 3), _z(B, cfg, 3)
    _, gd, gg = st.compute_grads(real, z, update_ema=False)
    d0, g0 = st.model.d.flat.clone(), st.model.g.flat.clone()
    st.step(real, z)
    for name, ps, w0, g, lr in (("d_h3_lin/Matrix", st.model.d, d0, gd, lr_d), ("g_h0_lin/Matrix", st.model.g, g0, gg, lr_g)):
        off, n = ps.offsets[name][0], ps[name].numel()
        gv = g[off:off + n].double()
        want = -lr * gv / (gv.abs() + 1e-8 / (1 - b2) ** 0.5)
        got = (ps.flat[off:off + n] - w0[off:off + n]).double()
        live = gv.abs() > 1e-6
        assert int(live.sum()) > n // 2
        # (the update is an fp32 subtraction from weights of magnitude ~0.02: half an ulp is 1e-9)
        assert torch.allclose(got[live], want[live], rtol=1e-3, atol=2e-9), name
        assert float(got[live].abs().mean()) == pytest.approx(lr, rel=0.05)


# ------------------------------------------------------------------ 3. checkpoints
def test_checkpoint_resume_is_exact_and_adds_no_key(tmp_path):
    cfg, B = small(), 4

    def engine(seed, **kw):
        e = ReferenceEngine(cfg, B, CPU, seed=seed, **kw)
        e.set_synthetic_batch(_real(B, cfg, 7))
        return e
    a = engine(5, d_steps=3, beta2=0.9, lr_d=3e-4)
    for _ in range(2):
        a.train_step()
    plain = engine(5)
    plain.train_step()
    assert list(CK.collect_state(a)) == list(CK.collect_state(plain))
    mgr = CK.CheckpointManager(str(tmp_path), save_secs=0)
    mgr.save(a)
    b = engine(9, d_steps=3, beta2=0.9, lr_d=3e-4)
    info = mgr.restore_latest(b)
    assert info["global_step"] == 2 and info["adam_d"] and info["adam_g"]
    assert torch.equal(b.opt_d.powers, a.opt_d.powers) and float(b.opt_d.powers[0]) == pytest.approx(0.5 ** 7)
    assert torch.equal(torch.as_tensor(b.model.d_bn.steps), torch.as_tensor(a.model.d_bn.steps))
    b.z_gen.set_state(a.z_gen.get_state())
    a.train_step()
    b.train_step()
    assert a.last_losses() == b.last_losses()
    for x, y in ((a.model.d.flat, b.model.d.flat), (a.model.g.flat, b.model.g.flat), (a.opt_d.powers, b.opt_d.powers),
                 (a.opt_d.v.flat, b.opt_d.v.flat), (a.model.d_bn.flat, b.model.d_bn.flat)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 4. schedules (dry-run HIP engines)
G_OPS = ("adam_g", "adam_gd", "ema_g", "g_h0_lin.wgrad", "step_end")


def _check_sub_ops(eng):
    full = eng.op_names()[:eng.progA.size()]
    fwd = [eng.progA.name(i) for i in range(eng._a_fwd)]
    for k in range(eng.d_steps - 1):
        names = eng.sub_op_names(k)
        pf, pb = eng._sub[k]
        assert names[:pf.size()] == fwd == full[:eng._a_fwd]  # the full step's forward ops
        assert names[pf.size():pf.size() + pb.size()] == [eng.progB.name(i) for i in range(eng.progB.size())]
        assert not [n for n in names if n in G_OPS or n.startswith(("adam_g", "g.")) or
                    (n.startswith("g_h") and "wgrad" in n)], names
        upd = [n for n in names if n in ("adam_d", "adam_d1")]
        assert len(upd) == 1, names
        if eng.d_spectral_norm:
            assert names.index("sn_power.wu") == names.index(upd[0]) + 1 and names.count("sn_power.wu") == 1
        assert ("d_step_end" in names) == (upd[0] == "adam_d")
        # the z seed of sub-step k differs from the full step's and the other sub-steps'
    seeds = [eng._zseed()] + [eng._zseed(k) for k in range(eng.d_steps - 1)]
    assert len(set(seeds)) == eng.d_steps and all(0 <= s < 2 ** 64 for s in seeds)
    # G's BN moving averages are not written by a sub-step, D's are
    g_ema_ptr, d_ema_ptr = eng.model.g_bn.flat.data_ptr(), eng.model.d_bn.flat.data_ptr()
    g_end, d_end = g_ema_ptr + 4 * eng.model.g_bn.flat.numel(), d_ema_ptr + 4 * eng.model.d_bn.flat.numel()
    wrote_d = False
    for i in range(eng._sub[0][0].size()):
        for p, n, w in eng._sub[0][0].op_info(i)[4]:
            assert not (w and p < g_end and p + n > g_ema_ptr), eng._sub[0][0].name(i)
            wrote_d |= bool(w and p < d_end and p + n > d_ema_ptr)
    assert wrote_d == (eng.model.d_bn.flat.numel() > 0)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("world,wire", [(1, "fp32"), (1, "bf16"), (2, "fp32"), (2, "bf16"), (4, "fp32"), (4, "bf16"),
                                        (8, "fp32"), (8, "bf16")])
def test_sub_step_schedules_have_no_stream_hazards(dtype, world, wire):
    for sn, bn, ema in ((False, True, 0.0), (True, True, 0.0), (True, False, 0.999), (False, False, 0.999)):
        eng = _hip(small(bn), dtype=dtype, world=world, allreduce_dtype=wire, d_spectral_norm=sn, g_ema_decay=ema,
                   d_steps=3)
        assert eng._schedule() == ("fused" if world == 1 else "concurrent")
        hz, n = SC.check_engine(eng)  # two training steps: sub, sub, full, sub, sub, full
        assert hz == [], "%s\n%s" % ((sn, bn, ema), "\n".join(map(str, hz[:10])))
        one = _hip(small(bn), dtype=dtype, world=world, allreduce_dtype=wire, d_spectral_norm=sn, g_ema_decay=ema)
        assert n > SC.check_engine(one)[1] + 4 * 30
        _check_sub_ops(eng)
        assert eng.sub_op_names(0).count("adam_d1") == int(world == 1 and dtype == "bf16")
        # the full step's programs are those of the engine without sub-steps
        assert one.op_names() == eng.op_names()[:len(one.op_names())]
        assert eng.kernel_count() > one.kernel_count()


def test_flagship_model_and_timed_step_with_sub_steps():
    for kw in (dict(), dict(world=2), dict(world=2, allreduce_dtype="bf16")):
        eng = _hip(DCGANConfig(), d_steps=2, d_spectral_norm=True, **kw)
        hz, _ = SC.check_engine(eng)
        assert hz == []
        _check_sub_ops(eng)
    eng = _hip(DCGANConfig(), d_steps=2)
    eng._timing = True  # (enable_timing without its CUDA events): the segmented step at W = 1
    eng._build_updates()
    assert eng._schedule() == "concurrent" and "adam_d" in eng.sub_op_names(0)
    assert SC.check_engine(eng)[0] == []


def test_split_update_switch(monkeypatch):
    monkeypatch.setenv("DCGAN_D_UPDATE", "split")
    eng = _hip(d_steps=2)
    assert "adam_d" in eng.sub_op_names(0) and "d_step_end" in eng.sub_op_names(0)
    assert SC.check_engine(eng)[0] == []


@pytest.mark.parametrize("world", [1, 2])
def test_checker_finds_the_d_update_ahead_of_the_join(world, monkeypatch):
    """A planted race: the sub-step's D update issued before the main stream joins the D chain."""
    eng = _hip(DCGANConfig(), world=world, d_steps=3)
    assert SC.check_engine(eng)[0] == []
    if world == 1:
        def racy(ex, cs, k):
            F_, Bk = eng._sub[k]
            ex.run(F_, [cs, ex.side])
            ex.wait(ex.alt[0], cs)
            ex.run(Bk, ex.alt)
            ex.run(eng.progDU, [cs, ex.side])  # no ex.wait(cs, alt0)
            ex.wait(cs, ex.alt[0])
        monkeypatch.setattr(eng, "_run_fused_sub", racy)
    else:
        def racy(ex, k):
            cs, alt = ex.main(), ex.alt[0]
            eng._sub_seg(ex, k, 0, cs)
            ex.wait(alt, cs)
            eng._sub_seg(ex, k, 1, alt)
            eng._ar_launch(ex, "dtop", alt)
            eng._sub_seg(ex, k, 2, alt)
            eng._ar_launch(ex, "drest", alt)
            eng._sub_seg(ex, k, 3, cs)         # before the joins with the comm stream and the D chain
            eng._ar_join(ex, cs)
            ex.wait(cs, alt)
        monkeypatch.setattr(eng, "_run_d_substep", racy)
    hz, _ = SC.check_engine(eng)
    txt = "\n".join(map(str, hz))
    assert hz and ("adam_d" in txt) and ("alt0" in txt or "comm" in txt), txt


# ------------------------------------------------------------------ 5. trainer / CLI
def test_trainer_draws_d_steps_batches_per_step(tmp_path, monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.data import pipeline as P
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    calls = []
    orig = P.SyntheticSource.next

    def counting(self):
        calls.append(1)
        return orig(self)
    monkeypatch.setattr(P.SyntheticSource, "next", counting)
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--d_steps=2", "--max_steps=2", "--sample_every=0", "--nosummaries",
                        "--train_size=32", "--epoch=0", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    import io
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    assert len(calls) == 4
    text = out.getvalue()
    assert "2 discriminator update(s) per generator update (2 real batches per step)" in text
    # 32 images / (2 x 1 x 4 per step) = 4 steps per epoch
    lines = [l for l in text.splitlines() if l.startswith("Epoch:")]
    assert len(lines) == 2 and "images/sec" in lines[-1]


def test_cli_runs_with_d_steps(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--d_steps=2", "--max_steps=2", "--device=cpu", "--output_size=28",
            "--c_dim=1", "--batch_size=4", "--sample_every=0", "--nosummaries", "--beta1=0", "--beta2=0.9",
            "--gan_loss=hinge", "--d_spectral_norm", "--nod_batch_norm", "--d_learning_rate=4e-4",
            "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert len([l for l in p.stdout.splitlines() if l.startswith("Epoch:")]) == 2
    assert "Adam lr D 0.0004 / G 0.0002, beta1 0, beta2 0.9" in p.stdout
    assert os.path.exists(tmp_path / "ck" / "model.ckpt-2.index")
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--d_steps=17"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "d_steps" in bad.stdout
