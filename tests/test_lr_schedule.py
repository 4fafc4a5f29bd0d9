"""Learning-rate schedules (--lr_decay / --lr_decay_start / --lr_decay_steps / --lr_end /
--lr_warmup_steps), CPU side: the oracle, validation and precedence, TFAdam / ReferenceStep / the
reference engine with a factor, checkpoint resume, the dry-run HIP schedules, the trainer and CLI."""
import glob
import io
import math
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
from distributed_tensorflow_for_dcgan_amd.obs.events import read_events
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.optim.adam import TFAdam
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_ENV = ("DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP")
ENV = LR_ENV + ("DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_DDP_SHARD", "DCGAN_DDP_SCHEDULE",
                "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM", "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS", "DCGAN_D_UPDATE")
KINDS = ("linear", "cosine", "exponential")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def small():
    return DCGANConfig(output_size=28, c_dim=1)


def _real(B, cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=g) * 2 - 1


def _z(B, cfg, seed):
    return torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _hip(cfg=None, **kw):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    kw.setdefault("graph", False)
    return HipEngine(cfg or small(), 4, CPU, dry_run=True, **kw)


# ------------------------------------------------------------------ 1. the oracle
def _closed_form(kind, start, steps, end, warmup, t):
    k = 0 if t <= start else min(t - start, steps)
    p = k / steps
    f = {"none": 1.0, "linear": 1 - (1 - end) * p, "cosine": 1 - (1 - end) * 0.5 * (1 - math.cos(math.pi * p)),
         "exponential": end ** p if end > 0 else 0.0}[kind]
    return f * (t + 1) / warmup if t < warmup else f


@pytest.mark.parametrize("kind", ("none",) + KINDS)
def test_oracle_matches_the_closed_form(kind):
    start, steps, end, warmup = 5, 40, 0.125, 9
    s = R.check_lr_schedule(kind, start, steps, end, warmup)
    ts = list(range(0, 60)) + [10 ** 6]
    got64 = R.lr_factor(s, torch.tensor(ts), dtype=torch.float64)
    got32 = R.lr_factor(s, torch.tensor(ts))
    assert got64.dtype == torch.float64 and got32.dtype == torch.float32
    want = torch.tensor([_closed_form(kind, start, steps, end, warmup, t) for t in ts], dtype=torch.float64)
    assert torch.allclose(got64, want, rtol=0, atol=1e-15)
    assert torch.allclose(got32.double(), want, rtol=0, atol=2.0 ** -22)
    assert float(R.lr_factor(s, 17)) == float(got32[17])  # a plain int gives the same number


@pytest.mark.parametrize("kind", KINDS)
def test_end_points_are_exact_and_the_factor_is_monotone(kind):
    start, steps, end = 7, 1000, 0.3
    s = R.check_lr_schedule(kind, start, steps, end)
    t = torch.arange(0, start + steps + 50)
    for dt in (torch.float32, torch.float64):
        f = R.lr_factor(s, t, dtype=dt)
        assert bool((f[:start + 1] == 1).all())                          # t <= start: exactly 1
        assert bool((f[start + steps:] == torch.tensor(end, dtype=dt)).all())  # t >= start + steps: exactly end
        assert bool((f[1:] <= f[:-1]).all()) and bool((f[start + 1:start + steps] < 1).all())
        assert bool((f >= torch.tensor(end, dtype=dt)).all())
    assert float(R.lr_factor(s, 2 ** 40)) == float(torch.tensor(end))
    z = R.check_lr_schedule("linear", 0, 2, 0.0)
    assert [float(R.lr_factor(z, t)) for t in range(4)] == [1.0, 0.5, 0.0, 0.0]


def test_warmup_multiplies_the_decay():
    s = R.check_lr_schedule("linear", 2, 10, 0.5, 6)
    dec = R.check_lr_schedule("linear", 2, 10, 0.5, 0)
    for t in range(12):
        w = torch.tensor(float(t + 1)) / torch.tensor(6.0) if t < 6 else torch.tensor(1.0)
        assert float(R.lr_factor(s, t)) == float(R.lr_factor(dec, t) * w)
    only = R.check_lr_schedule("none", warmup=4)
    assert only.active and [float(R.lr_factor(only, t)) for t in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    off = R.check_lr_schedule()
    assert not off.active and off == R.LrSchedule() and float(R.lr_factor(off, 123)) == 1.0


# ------------------------------------------------------------------ 2. validation, precedence
BAD = [("lr_decay", "step"), ("lr_decay_start", -1), ("lr_decay_steps", 0), ("lr_decay_steps", 2 ** 24 + 1),
       ("lr_end", -0.1), ("lr_end", 1.5), ("lr_warmup", -1), ("lr_warmup", 2 ** 24 + 1)]
FLAG = {"lr_warmup": "lr_warmup_steps"}


@pytest.mark.parametrize("name,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_invalid_values_are_rejected_everywhere(name, value, monkeypatch, capsys):
    flag = FLAG.get(name, name)
    kw = dict(lr_decay="linear", lr_decay_steps=10)
    kw[name] = value
    pos = dict(kind=kw["lr_decay"], start=kw.get("lr_decay_start", 0), steps=kw["lr_decay_steps"],
               end=kw.get("lr_end", 0.0), warmup=kw.get("lr_warmup", 0))
    with pytest.raises(ValueError, match=flag):
        R.check_lr_schedule(**pos)
    with pytest.raises(ValueError, match=flag):
        ReferenceStep(DCGAN(small(), seed=0), **kw)
    with pytest.raises(ValueError, match=flag):
        ReferenceEngine(small(), 4, CPU, **kw)
    with pytest.raises(ValueError, match=flag):
        _hip(**kw)
    with pytest.raises(ValueError, match=flag):
        build_engine(small(), 4, CPU, engine="reference", **kw)
    if (name, value) != ("lr_decay_steps", 0):  # (0 on the command line: until the end of training)
        argv = ["--lr_decay=linear", "--lr_decay_steps=10"]
        argv = [a for a in argv if not a.startswith("--%s=" % flag)] + ["--%s=%s" % (flag, value)]
        with pytest.raises(SystemExit):
            F.parse_flags(argv)
        assert flag in capsys.readouterr().err
    env = {"lr_decay": "DCGAN_LR_DECAY", "lr_decay_start": "DCGAN_LR_DECAY_START", "lr_decay_steps":
           "DCGAN_LR_DECAY_STEPS", "lr_end": "DCGAN_LR_END", "lr_warmup": "DCGAN_LR_WARMUP"}
    monkeypatch.setenv("DCGAN_LR_DECAY", "linear")
    monkeypatch.setenv("DCGAN_LR_DECAY_STEPS", "10")
    monkeypatch.setenv(env[name], str(value))
    with pytest.raises(ValueError, match=flag):
        ReferenceEngine(small(), 4, CPU)
    with pytest.raises(ValueError, match=flag):
        _hip()


def test_exponential_needs_a_positive_end_and_none_reads_nothing_else():
    with pytest.raises(ValueError, match="lr_end"):
        R.check_lr_schedule("exponential", 0, 10, 0.0)
    with pytest.raises(SystemExit):
        F.parse_flags(["--lr_decay=exponential", "--lr_decay_steps=10"])
    assert R.check_lr_schedule("exponential", 0, 10, 1e-3).end == 1e-3
    assert R.check_lr_schedule("none", -5, 0, 7.0) == R.LrSchedule()  # not read without a decay
    assert R.check_lr_schedule(" Cosine ", 3, 2 ** 24, 1.0, 2 ** 24) == R.LrSchedule("cosine", 3, 2 ** 24, 1.0, 2 ** 24)
    fl = F.parse_flags([])
    assert (fl.lr_decay, fl.lr_decay_start, fl.lr_decay_steps, fl.lr_end, fl.lr_warmup_steps) == ("none", 0, 0, 0.0, 0)
    fl = F.parse_flags(["--lr_decay=cosine", "--lr_decay_start=5", "--lr_decay_steps=0", "--lr_end=0.1",
                        "--lr_warmup_steps=3"])
    assert (fl.lr_decay, fl.lr_decay_start, fl.lr_decay_steps, fl.lr_end, fl.lr_warmup_steps) == ("cosine", 5, 0, 0.1, 3)


def test_an_explicit_argument_wins_over_the_environment(monkeypatch):
    for k, v in zip(LR_ENV, ("cosine", "3", "50", "0.25", "4")):
        monkeypatch.setenv(k, v)
    assert R.resolve_lr_schedule() == R.LrSchedule("cosine", 3, 50, 0.25, 4)
    for mk in (lambda **kw: ReferenceEngine(small(), 4, CPU, **kw), lambda **kw: _hip(**kw)):
        assert mk().lr_sched == R.LrSchedule("cosine", 3, 50, 0.25, 4)
        e = mk(lr_decay="linear", lr_decay_start=1, lr_decay_steps=9, lr_end=0.5, lr_warmup=0)
        assert e.lr_sched == R.LrSchedule("linear", 1, 9, 0.5, 0)
        assert mk(lr_decay="none", lr_warmup=0).lr_sched == R.LrSchedule()
        assert mk(lr_end=0.75).lr_sched == R.LrSchedule("cosine", 3, 50, 0.75, 4)
    monkeypatch.setenv("DCGAN_LR_END", "lots")
    with pytest.raises(ValueError, match="DCGAN_LR_END"):
        R.resolve_lr_schedule()
    for k in LR_ENV:
        monkeypatch.delenv(k)
    assert R.resolve_lr_schedule() == R.LrSchedule() and not _hip().lr_sched.active


def test_open_ended_length_resolves_to_the_end_of_training():
    assert R.check_lr_schedule("linear", 10, 0, 0.0, total_steps=50).steps == 40
    assert R.check_lr_schedule("linear", 10, 7, 0.0, total_steps=50).steps == 7  # an explicit length stays
    with pytest.raises(ValueError, match="lr_decay_steps"):
        R.check_lr_schedule("linear", 50, 0, 0.0, total_steps=50)
    with pytest.raises(ValueError, match="lr_decay_steps"):
        R.check_lr_schedule("linear", 0, 0, 0.0)
    assert R.check_lr_schedule("linear", 0, 0, 0.0, open_ended=True).steps == 0


# ------------------------------------------------------------------ 3. TFAdam, ReferenceStep, engine
def test_tfadam_with_a_factor_is_the_update_with_lr_times_f():
    cfg = small()
    m = DCGAN(cfg, seed=1)
    opt = TFAdam(m.d, lr=3e-4, beta1=0.5, beta2=0.9)
    n = m.d.flat.numel()
    gen = torch.Generator().manual_seed(2)
    w = m.d.flat.clone()
    mm, vv = torch.zeros(n), torch.zeros(n)
    b1p, b2p = 0.5, float(torch.tensor(0.9))  # the powers are fp32 variables
    for f in (1.0, 0.625, 0.0):
        g = torch.randn(n, generator=gen)
        opt.step(g, f)
        R.tf_adam_update(w, g, mm, vv, b1p, b2p, 3e-4 * f, 0.5, 0.9, 1e-8)
        b1p, b2p = float(torch.tensor(b1p) * 0.5), float(torch.tensor(b2p) * 0.9)
        assert torch.equal(m.d.flat, w) and torch.equal(opt.m.flat, mm) and torch.equal(opt.v.flat, vv)
    before = m.d.flat.clone()
    opt.step(torch.randn(n, generator=gen), 0.0)  # f = 0: the slots move, the weights do not
    assert torch.equal(m.d.flat, before) and not torch.equal(opt.m.flat, mm)
    plain = TFAdam(DCGAN(cfg, seed=1).d, lr=3e-4)
    other = TFAdam(DCGAN(cfg, seed=1).d, lr=3e-4)
    g = torch.randn(n, generator=gen)
    plain.step(g)
    other.step(g, 1.0)
    assert torch.equal(plain.params.flat, other.params.flat)


def _hand_cycle(st, sched, reals, zs, d_steps):
    """One training step by hand: both optimisers' rates set to lr * f(global step) around it."""
    f = float(R.lr_factor(sched, st.global_step))
    lr_d, lr_g = st.opt_d.lr, st.opt_g.lr
    st.opt_d.lr, st.opt_g.lr = lr_d * f, lr_g * f
    for k in range(d_steps - 1):
        st.d_step(reals[k], zs[k])
    out = st.step(reals[-1], zs[-1])
    st.opt_d.lr, st.opt_g.lr = lr_d, lr_g
    return out, f


@pytest.mark.parametrize("d_steps", [1, 2])
def test_reference_step_applies_the_factor_of_its_global_step(d_steps):
    cfg, B = small(), 4
    kw = dict(lr_decay="cosine", lr_decay_start=1, lr_decay_steps=3, lr_end=0.1, lr_warmup=2)
    sched = R.check_lr_schedule("cosine", 1, 3, 0.1, 2)
    a = ReferenceStep(DCGAN(cfg, seed=3), lr=3e-4, d_steps=d_steps, lr_d=5e-4, **kw)
    b = ReferenceStep(DCGAN(cfg, seed=3), lr=3e-4, d_steps=d_steps, lr_d=5e-4)
    assert a.lr_sched == sched and not b.lr_sched.active
    seen = []
    for step in range(4):
        reals = [_real(B, cfg, 10 * step + k) for k in range(d_steps)]
        zs = [_z(B, cfg, 100 * step + k) for k in range(d_steps)]
        assert a.lr_factor() == float(R.lr_factor(sched, step))
        for k in range(d_steps - 1):
            a.d_step(reals[k], zs[k])
            assert a.lr_factor() == float(R.lr_factor(sched, step))  # a sub-step leaves t alone
        got = a.step(reals[-1], zs[-1])
        want, f = _hand_cycle(b, sched, reals, zs, d_steps)
        seen.append(f)
        assert got == want
        for x, y in ((a.model.d.flat, b.model.d.flat), (a.model.g.flat, b.model.g.flat), (a.opt_d.m.flat, b.opt_d.m.flat),
                     (a.opt_g.v.flat, b.opt_g.v.flat), (a.opt_d.powers, b.opt_d.powers)):
            assert torch.equal(x, y)
    assert seen[0] == 0.5 and seen[1] == 1.0 and seen[3] < seen[2] < 1.0  # warm-up, then the decay


def test_resume_continues_the_schedule_exactly_and_adds_no_key(tmp_path):
    cfg, B = small(), 4
    kw = dict(lr_decay="linear", lr_decay_steps=4, lr_end=0.0)

    def engine(seed, **k):
        e = ReferenceEngine(cfg, B, CPU, seed=seed, **k)
        e.set_synthetic_batch(_real(B, cfg, 7))
        return e
    a = engine(5, **kw)
    for _ in range(2):
        a.train_step()
    assert list(CK.collect_state(a)) == list(CK.collect_state(engine(5)))
    mgr = CK.CheckpointManager(str(tmp_path), save_secs=0)
    mgr.save(a)
    b = engine(9, **kw)
    assert mgr.restore_latest(b)["global_step"] == 2
    assert b.step_impl.lr_factor() == a.step_impl.lr_factor() == 0.5
    b.z_gen.set_state(a.z_gen.get_state())
    for _ in range(3):  # factors 0.5, 0.25, then 0: the last step moves no weight
        wa = a.model.g.flat.clone()
        a.train_step()
        b.train_step()
        assert a.last_losses() == b.last_losses()
        for x, y in ((a.model.d.flat, b.model.d.flat), (a.model.g.flat, b.model.g.flat), (a.opt_g.m.flat, b.opt_g.m.flat)):
            assert torch.equal(x, y)
    assert a.global_step == 5 and torch.equal(a.model.g.flat, wa)


# ------------------------------------------------------------------ 4. schedules (dry-run HIP engines)
ON = dict(lr_decay="linear", lr_decay_start=2, lr_decay_steps=10, lr_end=0.1, lr_warmup=3)


def _adam_ops(eng, steps=1):
    ex = SC.RecordingExec(eng.ext)
    eng._ensure_comm()
    for s in range(steps):
        ex.step = s
        eng._run_step(ex)
    return ex, [op for op in ex.ops if "adam" in op.label.split(":", 1)[1]]


def _reads_step(eng, op):
    p = eng.step_counter.data_ptr()
    return any(a == p and n == 8 and not w for a, n, w in op.acc)


CASES = [(1, None, "fp32", 1), (1, None, "fp32", 2), (1, "serial", "fp32", 1)]
for _w in (2, 4, 8):
    for _wire in ("fp32", "bf16"):
        CASES += [(_w, None, _wire, 1), (_w, None, _wire, 2), (_w, "ddp", _wire, 1), (_w, "serial", _wire, 1)]


@pytest.mark.parametrize("world,schedule,wire,d_steps", CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in CASES])
def test_schedules_are_hazard_free_and_every_adam_reads_the_counter(world, schedule, wire, d_steps):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **ON)
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _, adams = _adam_ops(eng)
    names = {op.label.split(":", 1)[1] for op in adams}
    assert names and all(_reads_step(eng, op) for op in adams), names
    if world == 1 and schedule is None:
        assert names == ({"adam_gd", "adam_d1"} if d_steps > 1 else {"adam_gd"})
    elif schedule is None:
        assert {"adam_d", "adam_g_a", "adam_g_b", "adam_g_c"} <= names


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("d_steps", [1, 2])
def test_other_dtypes_are_hazard_free_with_a_schedule(dtype, d_steps):
    for world in (1, 2):
        eng = _hip(dtype=dtype, world=world, d_steps=d_steps, **ON)
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))
        _, adams = _adam_ops(eng)
        assert {op.label.split(":", 1)[1] for op in adams} >= {"adam_d"} and all(_reads_step(eng, op) for op in adams)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free_with_a_schedule(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    eng = _hip(world=world, **ON)
    assert eng._sharded()
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _, adams = _adam_ops(eng)
    names = {op.label.split(":", 1)[1] for op in adams}
    assert {"adam_shard.g_a", "adam_shard.dw_top", "adam.d_small", "adam.g_c"} <= names
    assert all(_reads_step(eng, op) for op in adams)


def test_without_a_schedule_no_adam_reads_the_counter(monkeypatch):
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16")):
        eng = _hip(**kw)
        _, adams = _adam_ops(eng)
        # (adam2 advances the counter itself: it lists the write, and no read)
        assert adams and not any(_reads_step(eng, op) for op in adams), kw
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    eng = _hip(world=2)
    _, adams = _adam_ops(eng)
    assert adams and not any(_reads_step(eng, op) for op in adams)


def _planted(eng):
    """The sharded step with step_end (segment 5, main stream) issued ahead of Adam over g_a's
    shard, which runs on the comm stream: nothing orders the two."""
    def racy(ex):
        cs, alt = ex.main(), ex.alt[0]
        eng._seg(ex, 0, cs)
        ex.wait(alt, cs)
        eng._seg(ex, 1, alt)
        eng._sh_rs(ex, "dw_top", alt)
        gd = []
        eng._g_chain_gw_alt(ex, cs, on_gd=gd.append, sharded=True)
        eng._sh_rs(ex, "g_a", cs)
        eng._sh_update(ex, "g_b")
        ex.run(eng.progB, ex.alt, eng._b_split, eng._b_top_dgrad)
        ex.wait_mark(ex.comm, gd[0])
        ex.wait(ex.comm, alt)
        eng._sh_update(ex, "dw_top")
        ex.run(eng.progB, ex.alt, eng._b_top_dgrad, -1)
        eng._sh_rs(ex, "dw_rest", alt)
        eng._sh_update(ex, "dw_rest")
        eng._ar_launch(ex, "d_small", alt)
        eng._g_tail_gw_alt(ex, cs)
        eng._ar_launch(ex, "g_c", cs)
        eng._ar_join(ex, cs)
        ex.wait(cs, alt)
        eng._seg(ex, 5, cs)                  # step_end moves the counter ...
        eng._sh_update(ex, "g_a")            # ... that this Adam slice still has to read
    return racy


def test_checker_finds_step_end_ahead_of_an_adam_slice(monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")

    def on_counter(eng):
        # (the checker reports an op pair once, and this pair also shares the beta powers: keep
        # only the accesses to the counter, so that the new read range alone decides)
        eng._run_step = _planted(eng)
        assert SC.check_engine(eng, steps=1)[0]
        ex, _ = _adam_ops(eng)
        p = eng.step_counter.data_ptr()
        for op in ex.ops:
            op.acc = [a for a in op.acc if a[0] == p]
        return SC.find_hazards(ex.ops)
    hz = on_counter(_hip(world=2, **ON))
    assert hz and all("step_end" in h.a + h.b and "adam_shard.g_a" in h.a + h.b for h in hz), "\n".join(map(str, hz))
    assert on_counter(_hip(world=2)) == []  # schedule off: that Adam never touches the counter


# ------------------------------------------------------------------ 5. trainer / CLI
def _train_flags(tmp_path, *extra):
    return F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                          "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32",
                          "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
                          "--nolog_device_placement"] + list(extra))


def test_trainer_resolves_an_open_ended_decay(tmp_path, monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    built = []
    orig = T.build_engine

    def spy(*a, **kw):
        built.append(kw)
        return orig(*a, **kw)
    monkeypatch.setattr(T, "build_engine", spy)
    out = io.StringIO()
    # 32 images / (1 x 4) = 8 steps per epoch; --epoch=1 caps --max_steps=100 at 8; minus the start
    fl = _train_flags(tmp_path, "--lr_decay=linear", "--lr_decay_start=5", "--max_steps=100", "--epoch=1", "--lr_end=0.5")
    assert T.run(fl, out=out) == 0
    assert built[-1]["lr_decay_steps"] == 3 and built[-1]["lr_decay"] == "linear"
    assert "learning-rate schedule: linear to 0.5 x over steps 5..8" in out.getvalue()
    assert len([l for l in out.getvalue().splitlines() if l.startswith("Epoch:")]) == 8
    fl = _train_flags(tmp_path / "b", "--lr_decay=linear", "--lr_decay_start=8", "--max_steps=100", "--epoch=1")
    with pytest.raises(SystemExit, match="lr_decay_steps"):
        T.run(fl, out=io.StringIO())
    out = io.StringIO()
    assert T.run(_train_flags(tmp_path / "c", "--max_steps=1", "--epoch=0"), out=out) == 0
    assert "learning-rate schedule" not in out.getvalue() and built[-1]["lr_decay"] == "none"


def test_cli_runs_with_a_schedule_and_logs_the_rates(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=3", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=4", "--sample_every=0", "--save_summaries_secs=0", "--epoch=0", "--lr_decay=linear",
            "--lr_decay_steps=4", "--lr_end=0", "--g_learning_rate=1e-4", "--checkpoint_dir=%s" % (tmp_path / "ck"),
            "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "learning-rate schedule: linear to 0 x over steps 0..4" in p.stdout
    files = glob.glob(str(tmp_path / "ck" / "events.out.tfevents.*"))
    assert len(files) == 1
    rates = {}
    for ev in read_events(files[0]):
        for v in ev["values"]:
            if v.get("tag", "").startswith("learning_rate/"):
                rates[(ev["step"], v["tag"])] = v["simple_value"]
    # the event at step s reports the rates that step s - 1 -> s was taken with
    for s, f in ((1, 1.0), (2, 0.75), (3, 0.5)):
        assert rates[(s, "learning_rate/d")] == pytest.approx(2e-4 * f, rel=1e-6)
        assert rates[(s, "learning_rate/g")] == pytest.approx(1e-4 * f, rel=1e-6)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--lr_decay=step"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "lr_decay" in bad.stdout
