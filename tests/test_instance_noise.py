"""Instance noise on D's inputs (--instance_noise / --instance_noise_end / --instance_noise_steps), CPU
side: the Philox / Box-Muller / sigma oracle, validation and precedence, ``ReferenceStep`` with noise
against a hand-written autograd step, the dry-run HIP schedules (hazards, where ``d_noise`` sits, a
planted race), the trainer and the CLI.

Statistics bounds are 5-sigma bounds of the estimators under the null hypothesis (n independent
standard normals): mean ~ N(0, 1/n), variance ~ N(1, 2/n), a correlation of m pairs ~ N(0, 1/m). The
fp64 oracle on these inputs gives Z1 <= 1.1, Z2 <= 2.4, Z3 <= 2.3, step 0 / step 1 correlation 1.5."""
import glob
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.obs.events import read_events
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_ENV = ("DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS")
ENV = NOISE_ENV + ("DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP",
                   "DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_DDP_SHARD", "DCGAN_DDP_SCHEDULE",
                   "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM", "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS", "DCGAN_D_UPDATE")
SEED = 1000020  # HipEngine._zseed of z_seed = 1, rank 0
N = 1 << 20


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


# ------------------------------------------------------------------ 1. Philox, the normals, sigma
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    """The Random123 known answers of Philox-4x32-10, one by one and as one vectorised call."""
    for ctr, key, want in KAT:
        got = R.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert got.dtype == np.uint32 and " ".join("%08x" % w for w in got) == want
    got = R.philox4x32_10(np.array([c for c, _, _ in KAT], dtype=np.uint64), np.array([k for _, k, _ in KAT], dtype=np.uint64))
    assert [" ".join("%08x" % w for w in row) for row in got] == [w for _, _, w in KAT]


def _box_muller(a, b):
    u0, u1 = ((int(a) >> 8) + 1) * 2.0 ** -24, (int(b) >> 8) * 2.0 ** -24
    r = math.sqrt(-2 * math.log(u0))
    return r * math.cos(2 * math.pi * u1), r * math.sin(2 * math.pi * u1)


def test_counter_layout_and_box_muller_on_hand_computed_indices():
    """Element e -> counter (lo32(e / 4), hi32(e / 4), lo32(t), hi32(t) ^ stream), lane e % 4; lanes
    0, 1 from words (c0, c1), lanes 2, 3 from (c2, c3). Element 5 is counter 1, lane 1."""
    seed, t, stream = 0x0123456789ABCDEF, (7 << 32) + 3, 1
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    eps = R.philox_normal(11, seed, t, stream)
    assert eps.dtype == torch.float64 and eps.shape == (11,)
    blocks = [R.philox4x32_10(np.array([i4, 0, 3, 7 ^ 1], dtype=np.uint64), key) for i4 in range(3)]
    assert (R.philox_words(11, seed, t, stream) == np.stack(blocks)).all()
    for e in range(11):
        w = blocks[e // 4]
        pair = _box_muller(w[0], w[1]) if e % 4 < 2 else _box_muller(w[2], w[3])
        assert float(eps[e]) == pytest.approx(pair[e % 2], rel=1e-14, abs=1e-15), e
    w = blocks[1]
    assert float(eps[5]) == pytest.approx(_box_muller(w[0], w[1])[1], rel=1e-14)
    # a prefix of a longer draw; the high half of the block index reaches counter word 1
    assert torch.equal(R.philox_normal(64, seed, t, stream)[:11], eps)
    hi = R.philox4x32_10(np.array([5, 2, 3, 7 ^ 1], dtype=np.uint64), key)
    i4 = (2 << 32) + 5
    ctr = np.array([[i4 & 0xFFFFFFFF, i4 >> 32, t & 0xFFFFFFFF, ((t >> 32) ^ stream)]], dtype=np.uint64)
    assert (R.philox4x32_10(ctr, key)[0] == hi).all()
    # fp32 form: the same draw within a few fp32 ulps of 5.77
    f32 = R.philox_normal(11, seed, t, stream, dtype=torch.float32)
    assert f32.dtype == torch.float32 and float((f32.double() - eps).abs().max()) < 4e-6
    assert float(eps.abs().max()) <= math.sqrt(48 * math.log(2))


@pytest.fixture(scope="module")
def draws():
    return {t: R.philox_normal(N, SEED, t, 1).numpy() for t in (0, 1, 7)}


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_statistics_of_the_oracle(draws):
    for t, e in draws.items():
        z1 = abs(e.mean()) * math.sqrt(N)
        z2 = abs(e.var() - 1) / math.sqrt(2 / N)
        z3 = abs(_corr(e[:N // 2], e[N // 2:])) * math.sqrt(N / 2)
        print("oracle step %d: Z1 %.2f Z2 %.2f Z3 %.2f" % (t, z1, z2, z3))
        assert z1 <= 5 and z2 <= 5 and z3 <= 5, (t, z1, z2, z3)
    z = abs(_corr(draws[0], draws[1])) * math.sqrt(N)
    print("oracle step 0 / step 1 correlation statistic %.2f" % z)
    assert z <= 5


def test_streams_differ(draws):
    other = R.philox_normal(N, SEED, 0, 0).numpy()
    assert not np.array_equal(other, draws[0]) and abs(_corr(other, draws[0])) * math.sqrt(N) <= 5
    assert (R.philox_words(8, SEED, 0, 1) != R.philox_words(8, SEED, 0, 0)).any()
    assert not np.array_equal(R.philox_normal(64, SEED + 1, 0, 1).numpy(), draws[0][:64])
    assert R.substep_seed(SEED) == SEED and R.substep_seed(SEED, 0) == (SEED + 0x9E3779B97F4A7C15) % 2 ** 64
    assert len({R.substep_seed(SEED, k) for k in (None, 0, 1, 2)}) == 4


@pytest.mark.parametrize("s0,s1,steps", [(0.2, 0.05, 4), (0.1, 0.0, 1000), (0.0, 2.0, 2 ** 24), (1.3, 0.7, 7)])
def test_sigma_against_the_closed_form(s0, s1, steps):
    ts = sorted({0, 1, 2, 3, steps // 3, steps // 2, steps - 1, steps, steps + 1, 2 ** 40})
    t = torch.tensor(ts)
    got32, got64 = R.noise_sigma(t, s0, s1, steps), R.noise_sigma(t, s0, s1, steps, dtype=torch.float64)
    assert got32.dtype == torch.float32 and got64.dtype == torch.float64
    f0, f1 = float(torch.tensor(s0)), float(torch.tensor(s1))  # (the device holds both ends in fp32)
    for i, x in enumerate(ts):
        want = s1 if x >= steps else s0 + (s1 - s0) * x / steps
        assert float(got64[i]) == pytest.approx(want, rel=1e-14, abs=1e-16)
        assert abs(float(got32[i]) - want) <= 2.0 ** -22  # a few fp32 ulps of 2
        if x >= steps:
            assert float(got32[i]) == f1
    assert float(got32[0]) == f0 and float(R.noise_sigma(0, s0, s1, steps)) == f0  # both end points exact
    dense = R.noise_sigma(torch.arange(0, min(steps, 4096) + 2), s0, s1, min(steps, 4096))
    d = dense[1:] - dense[:-1]
    assert bool((d <= 0).all()) if s1 < s0 else bool((d >= 0).all())  # monotone
    assert float(R.noise_sigma(17, s0, s1, steps)) == float(got32[ts.index(17)]) if 17 in ts else True


def test_sigma_constant_when_the_ends_are_equal():
    for steps in (0, 1, 5):
        s = R.noise_sigma(torch.tensor([0, 1, 10, 2 ** 40]), 0.3, 0.3, steps)
        assert s.tolist() == [float(torch.tensor(0.3))] * 4
    n = R.check_instance_noise(0.3, 0.3, 0)
    assert n == R.InstanceNoise(0.3, 0.3, 1) and n.active and n.describe() == "sigma 0.3"
    assert not R.check_instance_noise(0.0, 0.0, 12345).active and R.check_instance_noise() == R.InstanceNoise()
    assert R.check_instance_noise(0.0, 0.5, 3).active
    x = R.instance_noise((4, 2, 2, 1), R.InstanceNoise(0.2, 0.05, 4), SEED, 2)
    want = R.philox_normal(16, SEED, 2, 1) * float(R.noise_sigma(2, 0.2, 0.05, 4))
    assert x.shape == (4, 2, 2, 1) and x.dtype == torch.float32 and torch.equal(x.flatten(), want.float())


# ------------------------------------------------------------------ 2. validation, precedence
BAD = [("instance_noise", -0.1), ("instance_noise", 2.5), ("instance_noise", float("nan")),
       ("instance_noise", float("inf")), ("instance_noise_end", -1.0), ("instance_noise_end", 2.01),
       ("instance_noise_end", float("nan")), ("instance_noise_steps", 0), ("instance_noise_steps", -3),
       ("instance_noise_steps", 2 ** 24 + 1)]


@pytest.mark.parametrize("name,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_invalid_values_are_rejected_everywhere(name, value, monkeypatch, capsys):
    kw = dict(instance_noise=0.2, instance_noise_end=0.1, instance_noise_steps=10)
    kw[name] = value
    with pytest.raises(ValueError, match=name):
        R.check_instance_noise(kw["instance_noise"], kw["instance_noise_end"], kw["instance_noise_steps"])
    with pytest.raises(ValueError, match=name):
        ReferenceStep(DCGAN(small(), seed=0), **kw)
    with pytest.raises(ValueError, match=name):
        ReferenceEngine(small(), 4, CPU, **kw)
    with pytest.raises(ValueError, match=name):
        _hip(**kw)
    with pytest.raises(ValueError, match=name):
        build_engine(small(), 4, CPU, engine="reference", **kw)
    if (name, value) != ("instance_noise_steps", 0):  # (0 on the command line: until the end of training)
        with pytest.raises(SystemExit):
            F.parse_flags(["--%s=%s" % (k, v) for k, v in kw.items()])
        assert name in capsys.readouterr().err
    for k, v in zip(NOISE_ENV, (kw["instance_noise"], kw["instance_noise_end"], kw["instance_noise_steps"])):
        monkeypatch.setenv(k, str(v))
    with pytest.raises(ValueError, match=name):
        ReferenceEngine(small(), 4, CPU)
    with pytest.raises(ValueError, match=name):
        _hip()


def test_the_bindings_validate_on_their_own():
    """(A dry Program: records only.) Null pointers and bad schedules throw at record time."""
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    ok = (0x1000, 0x2000, 64, 1, 0x3000, 1, 0.2, 0.1, 10)
    assert prog.instance_noise("n", *ok) == 0
    name, slot, kind, ev, acc = prog.op_info(0)
    assert (name, slot) == ("n", 0) and sorted(acc) == [(0x1000, 128, False), (0x2000, 128, True), (0x3000, 8, False)]
    assert H.ext().Program(2, True).instance_noise("n", *ok) == 0
    for i in (0, 1, 4):  # x, y, step
        bad = list(ok)
        bad[i] = 0
        with pytest.raises(RuntimeError, match="non-null"):
            prog.instance_noise("n", *bad)
    with pytest.raises(RuntimeError, match="its own"):
        prog.instance_noise("n", 0x1000, 0x1000, 64, 1, 0x3000, 1, 0.2, 0.1, 10)
    for s0, s1, steps in ((-0.1, 0.1, 10), (0.2, 2.5, 10), (float("nan"), 0.1, 10), (0.2, float("inf"), 10),
                          (0.2, 0.1, 0), (0.2, 0.1, 2 ** 24 + 1)):
        with pytest.raises(RuntimeError, match="sigma|steps"):
            prog.instance_noise("n", 0x1000, 0x2000, 64, 1, 0x3000, 1, s0, s1, steps)
        with pytest.raises(RuntimeError, match="sigma|steps"):
            prog.noise_sigma("s", 0x1000, 0x2000, 4, s0, s1, steps)
    assert prog.instance_noise("n", 0x1000, 0x2000, 64, 1, 0x3000, 1, 0.3, 0.3, 0) == 1  # constant: steps not read
    with pytest.raises(RuntimeError, match="non-null"):
        prog.philox_normal("p", 0, 8, 1, 0x3000, 1)
    with pytest.raises(RuntimeError, match="non-null"):
        prog.philox_normal("p", 0x1000, 8, 1, 0, 1)
    with pytest.raises(RuntimeError, match="non-null"):
        prog.noise_sigma("s", 0, 0x2000, 4, 0.2, 0.1, 10)
    assert prog.philox_normal("p", 0x1000, 8, 1, 0x3000, 1) == 2 and prog.noise_sigma("s", 0x1000, 0x2000, 4, 0.2, 0.1, 10) == 3
    assert sorted(prog.op_info(2)[4]) == [(0x1000, 32, True), (0x3000, 8, False)]
    assert sorted(prog.op_info(3)[4]) == [(0x1000, 32, False), (0x2000, 16, True)]


def test_an_explicit_argument_wins_over_the_environment(monkeypatch):
    for k, v in zip(NOISE_ENV, ("0.4", "0.1", "50")):
        monkeypatch.setenv(k, v)
    assert R.resolve_instance_noise() == R.InstanceNoise(0.4, 0.1, 50)
    for mk in (lambda **kw: ReferenceEngine(small(), 4, CPU, **kw), lambda **kw: _hip(**kw)):
        assert mk().noise == R.InstanceNoise(0.4, 0.1, 50)
        assert mk(instance_noise=0.5, instance_noise_end=0.25, instance_noise_steps=9).noise == R.InstanceNoise(0.5, 0.25, 9)
        assert mk(instance_noise_end=0.3).noise == R.InstanceNoise(0.4, 0.3, 50)
        assert not mk(instance_noise=0.0, instance_noise_end=0.0).noise.active
    monkeypatch.setenv("DCGAN_INSTANCE_NOISE", "loud")
    with pytest.raises(ValueError, match="DCGAN_INSTANCE_NOISE"):
        R.resolve_instance_noise()
    for k in NOISE_ENV:
        monkeypatch.delenv(k)
    assert R.resolve_instance_noise() == R.InstanceNoise() and not _hip().noise.active and _hip().d_noisy is None


def test_open_ended_length_resolves_to_the_end_of_training():
    assert R.check_instance_noise(0.1, 0.0, 0, total_steps=50).steps == 50
    assert R.check_instance_noise(0.1, 0.0, 7, total_steps=50).steps == 7  # an explicit length stays
    for total in (0, -2, 2 ** 24 + 1):
        with pytest.raises(ValueError, match="instance_noise_steps"):
            R.check_instance_noise(0.1, 0.0, 0, total_steps=total)
    with pytest.raises(ValueError, match="instance_noise_steps"):
        R.check_instance_noise(0.1, 0.0, 0)
    assert R.check_instance_noise(0.1, 0.0, 0, open_ended=True).steps == 0
    fl = F.parse_flags([])
    assert (fl.instance_noise, fl.instance_noise_end, fl.instance_noise_steps) == (0.0, 0.0, 0)
    fl = F.parse_flags(["--instance_noise=0.1"])
    assert (fl.instance_noise, fl.instance_noise_end, fl.instance_noise_steps) == (0.1, 0.0, 0)


# ------------------------------------------------------------------ 3. ReferenceStep
def _hand_step(model, real, z, noise, full):
    """d_loss / g_loss and their gradients by plain autograd on cat(real, fake) + noise."""
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in model.g.tensors.items()}
    Pd = {k: v.detach().clone().requires_grad_(True) for k, v in model.d.tensors.items()}
    fake = model.generator(z, train=True, P=Pg, update_ema=False)
    both = torch.cat([real, fake], 0) + noise
    _, logits = model.discriminator(both, groups=2, slots=(0, 1), train=True, P=Pd, update_ema=False)
    B = real.shape[0]
    d_real, d_fake, g_loss, d_loss = R.gan_losses(logits[:B], logits[B:], "bce", 0.0)
    dn, gn = model.d.names(), model.g.names()
    gd = torch.autograd.grad(d_loss, [Pd[n] for n in dn], retain_graph=True, allow_unused=True)
    gg = torch.autograd.grad(g_loss, [Pg[n] for n in gn], allow_unused=True) if full else None
    return d_loss, g_loss, dict(zip(dn, gd)), (dict(zip(gn, gg)) if full else None)


def _flat_grads(ps, grads):
    out = ps.like()
    for n, g in grads.items():
        if g is not None:
            out[n].copy_(g)
    return out.flat


def test_reference_step_with_noise_is_autograd_on_the_noisy_input():
    cfg, B = small(), 4
    noise = R.InstanceNoise(0.3, 0.1, 5)
    st = ReferenceStep(DCGAN(cfg, seed=3), instance_noise=0.3, instance_noise_end=0.1, instance_noise_steps=5,
                       noise_seed=SEED, d_steps=2)
    assert st.noise == noise and st.noise_sigma() == float(R.noise_sigma(0, 0.3, 0.1, 5))
    st.global_step = 2
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    shape = (2 * B, 28, 28, 1)
    # the full step: drawn at the global step from the full step's seed
    eps = R.instance_noise(shape, noise, SEED, 2)
    assert torch.equal(st.draw_noise(shape), eps) and float(eps.abs().max()) > 0.1
    d_loss, g_loss, gd, gg = _hand_step(st.model, real, z, eps, True)
    out, fd, fg = st.compute_grads(real, z, update_ema=False)
    assert float(out["d_loss"].detach()) == float(d_loss.detach()) and float(out["g_loss"].detach()) == float(g_loss.detach())
    assert torch.equal(fd, _flat_grads(st.model.d, gd)) and torch.equal(fg, _flat_grads(st.model.g, gg))
    out2, fd2, _ = st.compute_grads(real, z, update_ema=False, noise=eps)  # passed in: the same step
    assert float(out2["d_loss"].detach()) == float(d_loss.detach()) and torch.equal(fd2, fd)
    clean = st.forward_losses(real, z, update_ema=False, noise=False)
    assert float(clean["d_loss"].detach()) != float(d_loss.detach())
    # the D sub-step: the sub-step's seed, the global step of the full step after it
    g0, gbn0, pw0 = st.model.g.flat.clone(), st.model.g_bn.flat.clone(), st.opt_g.powers.clone()
    eps_k = R.instance_noise(shape, noise, R.substep_seed(SEED, 0), 2)
    assert not torch.equal(eps_k, eps)
    d_loss_k, _, gd_k, _ = _hand_step(st.model, real, z, eps_k, False)
    got = st.d_step(real, z)
    assert got["d_loss"] == float(d_loss_k.detach()) and st.global_step == 2 and st._sub_k == 1
    assert torch.equal(st.model.g.flat, g0) and torch.equal(st.model.g_bn.flat, gbn0) and torch.equal(st.opt_g.powers, pw0)
    twin = ReferenceStep(DCGAN(cfg, seed=3), d_steps=2)
    twin.opt_d.step(_flat_grads(twin.model.d, gd_k))
    assert torch.equal(st.model.d.flat, twin.model.d.flat)  # Adam(D) of exactly that gradient
    st.step(real, z)
    assert st.global_step == 3 and st._sub_k == 0 and st.noise_sigma() == float(R.noise_sigma(3, 0.3, 0.1, 5))


def _run_steps(n=3, d_steps=2, **kw):
    cfg, B = small(), 4
    st = ReferenceStep(DCGAN(cfg, seed=3), d_steps=d_steps, **kw)
    losses = []
    for step in range(n):
        for k in range(d_steps - 1):
            losses.append(st.d_step(_real(B, cfg, 10 * step + k), _z(B, cfg, 100 * step + k)))
        losses.append(st.step(_real(B, cfg, 10 * step + 9), _z(B, cfg, 100 * step + 9)))
    return losses, st.model.d.flat.clone(), st.model.g.flat.clone()


def test_inactive_noise_is_bitwise_the_step_without_it_and_seeds_decide():
    plain = _run_steps()
    off = _run_steps(instance_noise=0.0, instance_noise_end=0.0, instance_noise_steps=0, noise_seed=5)
    assert off[0] == plain[0] and torch.equal(off[1], plain[1]) and torch.equal(off[2], plain[2])
    on = dict(instance_noise=0.2, instance_noise_end=0.0, instance_noise_steps=3)
    a, b, c = _run_steps(noise_seed=7, **on), _run_steps(noise_seed=7, **on), _run_steps(noise_seed=8, **on)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[0] != c[0] and not torch.equal(a[1], c[1])
    assert a[0] != plain[0] and not torch.equal(a[1], plain[1]) and not torch.equal(a[2], plain[2])


def test_reference_engine_uses_the_hip_engines_seed_and_clean_eval_losses():
    cfg, B = small(), 4
    kw = dict(instance_noise=0.5, instance_noise_end=0.5)
    e = ReferenceEngine(cfg, B, CPU, seed=3, rank=2, z_seed=1, **kw)
    h = _hip(seed=3, rank=2, z_seed=1, world=4, **kw)
    assert e.step_impl.noise_seed == h._zseed(None) == 1 * 1000003 + 17 + 7919 * 2
    assert R.substep_seed(e.step_impl.noise_seed, 1) == h._zseed(1)
    assert e.noise_sigma() == h.noise_sigma() == 0.5 and _hip().noise_sigma() == 0.0
    plain = ReferenceEngine(cfg, B, CPU, seed=3)
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    assert e.eval_losses(real, z) == plain.eval_losses(real, z)  # sample-time losses stay clean
    e.set_synthetic_batch(real)
    plain.set_synthetic_batch(real)
    e.train_step()
    plain.train_step()
    assert e.last_losses() != plain.last_losses()


# ------------------------------------------------------------------ 4. schedules (dry-run HIP engines)
ON = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=10)
CASES = [(1, None, "fp32", 1), (1, None, "fp32", 2), (1, "serial", "fp32", 1)]
for _w in (2, 4, 8):
    for _wire in ("fp32", "bf16"):
        CASES += [(_w, None, _wire, 1), (_w, None, _wire, 2), (_w, "ddp", _wire, 1), (_w, "serial", _wire, 1)]


def _record(eng, steps=1):
    ex = SC.RecordingExec(eng.ext)
    eng._ensure_comm()
    for s in range(steps):
        ex.step = s
        eng._run_step(ex)
    return ex


def _name(op):
    return op.label.split(":", 1)[1]


def _check_noise_ops(eng, d_steps):
    """One d_noise per forward, on the main stream, after the op writing the fake half and before D's
    first op; it reads the clean input and the 8-byte counter and writes the buffer layer 0 reads."""
    ex = _record(eng)
    idx = [i for i, op in enumerate(ex.ops) if _name(op) == "d_noise"]
    assert len(idx) == d_steps
    es = 4 if eng.f32 else 2
    nbytes = eng.d_in.numel() * es
    for k, i in enumerate(idx):
        op = ex.ops[i]
        d_in = eng.d_ins[k]
        assert op.stream == "main"
        assert sorted(op.acc) == sorted([(d_in.data_ptr(), nbytes, False), (eng.step_counter.data_ptr(), 8, False),
                                         (eng.d_noisy.data_ptr(), nbytes, True)])
        fake_lo = d_in.data_ptr() + nbytes // 2
        writers = [j for j, o in enumerate(ex.ops[:i]) if any(w and a < fake_lo + nbytes // 2 and a + n > fake_lo
                                                              for a, n, w in o.acc)]
        assert writers and writers[-1] == i - 1 and "g_h" in _name(ex.ops[i - 1]), _name(ex.ops[i - 1])
        nxt = ex.ops[i + 1]
        assert _name(nxt).startswith("d0.") or _name(nxt).startswith("d_h0"), _name(nxt)
        assert any(a == eng.d_noisy.data_ptr() and not w for a, _, w in nxt.acc)
    # the noisy copy has two readers: layer 0's forward and its weight gradient
    lo, hi = eng.d_noisy.data_ptr(), eng.d_noisy.data_ptr() + nbytes
    readers = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
    assert readers and all(r.startswith(("d0.", "d_h0")) for r in readers), readers
    assert len(readers) == 2 or readers == {"d0.im2col"}  # (fp32: the weight gradient reuses the forward's columns)
    # and nothing of D's layer 0 reads the clean input any more (G's tanh backward still reads the clean fake)
    for d_in in eng.d_ins:
        lo, hi = d_in.data_ptr(), d_in.data_ptr() + nbytes
        clean = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
        assert "d_noise" in clean and not any(r.startswith(("d0.", "d_h0")) for r in clean), clean


@pytest.mark.parametrize("world,schedule,wire,d_steps", CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in CASES])
def test_schedules_are_hazard_free_with_the_noise_op(world, schedule, wire, d_steps):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **ON)
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_noise_ops(eng, d_steps)
    assert eng.op_names().count("d_noise") == d_steps
    assert all(eng.sub_op_names(k).count("d_noise") == 1 for k in range(d_steps - 1))


@pytest.mark.parametrize("dtype,size,c_dim", [("fp16", 28, 1), ("fp32", 28, 1), ("fp32", 64, 3), ("bf16", 64, 3),
                                              ("bf16", 128, 3)])
@pytest.mark.parametrize("d_steps", [1, 3])
def test_other_dtypes_and_sizes_are_hazard_free_with_the_noise_op(dtype, size, c_dim, d_steps):
    """(Every form of G's RGB layer and of D's layer 0: narrow / direct kernels, im2col, plain GEMMs.)"""
    for world in (1, 2):
        eng = _hip(DCGANConfig(output_size=size, c_dim=c_dim), dtype=dtype, world=world, d_steps=d_steps, **ON)
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))
        _check_noise_ops(eng, d_steps)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free_with_the_noise_op(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    eng = _hip(world=world, **ON)
    assert eng._sharded()
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_noise_ops(eng, 1)


def test_checker_finds_a_d_chain_started_ahead_of_the_noise_op():
    """The fused step with the D chain's stream joined to the main stream BEFORE the forward, not
    after it: layer 0's weight gradient (alt stream) reads d_noisy with nothing ordering it against
    d_noise (main stream). Only the accesses to d_noisy are kept, so the new buffer alone decides."""
    def planted(eng):
        def bad_fused(ex, cs):
            ex.wait(ex.alt[0], cs)
            ex.run(eng.progA, [cs, ex.side], 0, eng._a_fwd)
            ex.run(eng.progB, ex.alt)
            ex.run(eng.progA, [cs, ex.side], eng._a_fwd, -1)
            ex.run(eng.progW, [cs, ex.side])
            ex.wait(cs, ex.alt[0])
            ex.run(eng.progC, [cs, ex.side])
        eng._run_fused = bad_fused
        ex = _record(eng, steps=2)
        assert SC.find_hazards(ex.ops)
        if eng.d_noisy is None:
            return []
        lo = eng.d_noisy.data_ptr()
        hi = lo + eng.d_noisy.numel() * 2
        for op in ex.ops:
            op.acc = [a for a in op.acc if lo <= a[0] < hi]
        return SC.find_hazards(ex.ops)
    eng = _hip(**ON)
    assert SC.check_engine(eng)[0] == []
    hz = planted(eng)
    assert hz and all("d_noise" in h.a + h.b and "wgrad" in h.a + h.b for h in hz), "\n".join(map(str, hz))
    assert planted(_hip()) == []


def test_with_the_switch_off_the_recorded_ops_are_todays():
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16"),
               dict(dtype="fp32")):
        off = _hip(instance_noise=0.0, instance_noise_end=0.0, instance_noise_steps=77, **kw)
        bare = _hip(**kw)
        assert off.d_noisy is None and bare.d_noisy is None and off.noise_sigma() == 0.0
        assert off.op_names() == bare.op_names() and "d_noise" not in bare.op_names()
        assert off.kernel_count() == bare.kernel_count()
        a, b = _record(off), _record(bare)
        assert [(_name(x), x.stream, len(x.acc)) for x in a.ops] == [(_name(x), x.stream, len(x.acc)) for x in b.ops]
        on = _hip(**ON, **kw)
        assert on.kernel_count() == bare.kernel_count() + on.d_steps
        names = [n for n in on.op_names() if n != "d_noise"]
        assert names == bare.op_names()


# ------------------------------------------------------------------ 5. trainer / CLI
def _train_flags(tmp_path, *extra):
    return F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                          "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32",
                          "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
                          "--nolog_device_placement"] + list(extra))


def test_trainer_resolves_an_open_ended_anneal(tmp_path, monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    built = []
    orig = T.build_engine

    def spy(*a, **kw):
        built.append(kw)
        return orig(*a, **kw)
    monkeypatch.setattr(T, "build_engine", spy)
    out = io.StringIO()
    # 32 images / (1 x 4) = 8 steps per epoch; --epoch=1 caps --max_steps=100 at 8
    fl = _train_flags(tmp_path, "--instance_noise=0.1", "--max_steps=100", "--epoch=1")
    assert T.run(fl, out=out) == 0
    assert (built[-1]["instance_noise"], built[-1]["instance_noise_end"], built[-1]["instance_noise_steps"]) == (0.1, 0.0, 8)
    assert "instance noise on D's inputs: sigma 0.1 to 0 over 8 steps" in out.getvalue()
    out = io.StringIO()
    fl = _train_flags(tmp_path / "b", "--instance_noise=0.1", "--instance_noise_end=0.1", "--max_steps=1", "--epoch=0")
    assert T.run(fl, out=out) == 0
    assert built[-1]["instance_noise_steps"] == 0 and "instance noise on D's inputs: sigma 0.1 (of" in out.getvalue()
    fl = _train_flags(tmp_path / "c", "--instance_noise=0.1", "--max_steps=0", "--epoch=0")
    with pytest.raises(SystemExit, match="instance_noise_steps"):
        T.run(fl, out=io.StringIO())
    out = io.StringIO()
    assert T.run(_train_flags(tmp_path / "d", "--max_steps=1", "--epoch=0"), out=out) == 0
    assert "instance noise" not in out.getvalue() and built[-1]["instance_noise"] == 0.0


def test_cli_runs_with_noise_and_logs_a_falling_sigma(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=4", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=4", "--sample_every=0", "--save_summaries_secs=0", "--epoch=0", "--instance_noise=0.1",
            "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "instance noise on D's inputs: sigma 0.1 to 0 over 4 steps" in p.stdout
    files = glob.glob(str(tmp_path / "ck" / "events.out.tfevents.*"))
    assert len(files) == 1
    sig = {}
    for ev in read_events(files[0]):
        for v in ev["values"]:
            if v.get("tag") == "instance_noise/sigma":
                sig[ev["step"]] = v["simple_value"]
    # the event at step s reports the sigma that step s - 1 -> s was taken with
    assert sorted(sig) == [1, 2, 3, 4]
    for s in (1, 2, 3, 4):
        assert sig[s] == pytest.approx(float(R.noise_sigma(s - 1, 0.1, 0.0, 4)), rel=1e-6)
    assert sig[1] == pytest.approx(0.1, rel=1e-6) and sig[1] > sig[2] > sig[3] > sig[4] > 0
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--instance_noise=3"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "instance_noise" in bad.stdout
