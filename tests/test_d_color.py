"""DiffAugment's color policy on D's inputs (--d_color_augment: brightness, saturation, contrast), CPU
side: the draws by hand from one Philox block, the oracle against a plain Python loop and against the
published three functions, the adjoint identities of its transpose, the exact-sum inputs the GPU tests
rely on, validation and precedence at every entry point, ``ReferenceStep``, the dry-run HIP schedules
(hazards, where ``d_color`` and ``d_color_bwd`` sit, a planted race), and the CLI."""
import io
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("DCGAN_D_COLOR_AUGMENT", "DCGAN_D_AUGMENT", "DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END",
       "DCGAN_INSTANCE_NOISE_STEPS", "DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END",
       "DCGAN_LR_WARMUP", "DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_DDP_SHARD",
       "DCGAN_DDP_SCHEDULE", "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM", "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS",
       "DCGAN_D_UPDATE")
SEED = 1000020  # HipEngine._zseed of z_seed = 1, rank 0
SEEDS = (SEED, 0xFEDCBA9876543210)
STEPS = (0, 1, 2 ** 32 + 3)
ALL = R.DColor(True, True, True)
SUBSETS = [R.DColor(*bits) for bits in itertools.product((False, True), repeat=3) if any(bits)]
SHAPES = [(3, 8, 3), (1, 5, 3), (2, 6, 4), (2, 28, 1), (2, 28, 3), (2, 64, 3), (1, 128, 3)]  # the GPU tests' (N, S, C)


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
    return HipEngine(cfg or DCGANConfig(), 8, CPU, dry_run=True, **kw)


def exact_sum_input(N, S, C, seed=0):
    """Values k / 128, integer |k| <= 128: exact in bf16, fp16 and fp32, and every partial sum of up to
    49,152 of them is a multiple of 2^-7 below 2^16, i.e. fits 24 bits: the fp32 sum is exact in any order."""
    k = torch.randint(-128, 129, (N, S, S, C), generator=torch.Generator().manual_seed(seed))
    return k.float() / 128


# ------------------------------------------------------------------ 1. the draws
def test_draws_by_hand_from_the_philox_block_of_each_sample():
    """Sample n: words 0..2 of the block at counter (lo32(n), hi32(n), lo32(t), hi32(t) ^ 3) under the seed."""
    f = np.float32
    for seed in SEEDS:
        for t in STEPS:
            got = R.color_params(5, seed, t)
            assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3)
            for n in range(5):
                ctr = np.array([n & 0xFFFFFFFF, n >> 32, t & 0xFFFFFFFF, ((t >> 32) ^ 3) & 0xFFFFFFFF], dtype=np.uint64)
                key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
                w = [int(v) for v in R.philox4x32_10(ctr, key)]
                u = [f(w[i] >> 8) * f(2.0 ** -24) for i in range(3)]
                want = [f(u[0] - f(0.5)), f(f(2) * u[1]), f(u[2] + f(0.5))]
                assert [f(v) for v in got[n].tolist()] == want
    assert R.COLOR_STREAM == 3 and len({R.COLOR_STREAM, R.AUG_STREAM, R.NOISE_STREAM, 0}) == 4
    p = R.color_params(4096, SEED, 7)
    b, s, c = p[:, 0], p[:, 1], p[:, 2]
    assert -0.5 <= float(b.min()) and float(b.max()) < 0.5 and 0 <= float(s.min()) and float(s.max()) < 2
    assert 0.5 <= float(c.min()) and float(c.max()) <= 1.5
    assert float(b.max()) > 0.45 and float(b.min()) < -0.45 and float(s.max()) > 1.9 and float(c.min()) < 0.55
    # the largest u2 rounds up: c reaches 1.5 itself, so its range is closed
    assert np.float32(np.float32(0xFFFFFF) * np.float32(2.0 ** -24)) + np.float32(0.5) == np.float32(1.5)
    assert not torch.equal(R.color_params(4, SEED, 1), R.color_params(4, SEED, 2))
    assert not torch.equal(R.color_params(4, SEED, 1), R.color_params(4, R.substep_seed(SEED, 0), 1))


# ------------------------------------------------------------------ 2. the oracle
def _loop(x, params, color, mean=None):
    """The definition element by element in numpy fp32 scalars, every operation rounded on its own."""
    f = np.float32
    x = x.numpy().astype(np.float32)
    N, S, _, C = x.shape
    y = np.empty_like(x)
    for n in range(N):
        b, s, c = (f(v) for v in params[n, :3].tolist())
        Mx = f(np.sum(x[n], dtype=np.float32) / f(S * S * C)) if mean is None else f(mean[n])
        M = f(Mx + b) if color.brightness else Mx
        for i in range(S):
            for j in range(S):
                v = [x[n, i, j, ch] for ch in range(C)]
                if color.brightness:
                    v = [f(a + b) for a in v]
                if color.saturation:
                    m = v[0]
                    for a in v[1:]:
                        m = f(m + a)
                    m = f(m / f(C))
                    v = [f(f(s * f(a - m)) + m) for a in v]
                if color.contrast:
                    v = [f(f(c * f(a - M)) + M) for a in v]
                y[n, i, j] = v
    return torch.from_numpy(y)


def _loop_t(g, params, color):
    f = np.float32
    g = g.numpy().astype(np.float32)
    N, S, _, C = g.shape
    y = np.empty_like(g)
    for n in range(N):
        _, s, c = (f(v) for v in params[n, :3].tolist())
        Gm = f(np.sum(g[n], dtype=np.float32) / f(S * S * C))
        for i in range(S):
            for j in range(S):
                v = [g[n, i, j, ch] for ch in range(C)]
                if color.contrast:
                    v = [f(f(c * f(a - Gm)) + Gm) for a in v]
                if color.saturation:
                    m = v[0]
                    for a in v[1:]:
                        m = f(m + a)
                    m = f(m / f(C))
                    v = [f(f(s * f(a - m)) + m) for a in v]
                y[n, i, j] = v
    return torch.from_numpy(y)


@pytest.mark.parametrize("shape", [(3, 8, 3), (1, 5, 3), (2, 6, 4), (2, 9, 1), (2, 7, 2)], ids=str)
def test_oracle_is_the_definition_element_by_element(shape):
    N, S, C = shape
    x = exact_sum_input(N, S, C, 1)
    g = exact_sum_input(N, S, C, 2)
    params = R.color_params(N, SEED, 3)
    for color in SUBSETS:
        assert torch.equal(R.color_augment(x, params, color), _loop(x, params, color)), color
        assert torch.equal(R.color_augment_transpose(g, params, color), _loop_t(g, params, color)), color
        for dt in (torch.bfloat16, torch.float16):  # computed in fp32 from the element's value, rounded once
            y = R.color_augment(x.to(dt), params, color)
            assert y.dtype == dt and torch.equal(y, _loop(x, params, color).to(dt))
    # a recorded Mx in column 3 is used as given
    xg = torch.tanh(torch.randn(N, S, S, C, generator=torch.Generator().manual_seed(5)))
    mean = R.color_mean(xg) + 0.25
    p4 = torch.cat([params, mean[:, None]], 1)
    assert torch.equal(R.color_augment(xg, p4, ALL), _loop(xg, params, ALL, mean=mean.tolist()))
    assert not torch.equal(R.color_augment(xg, p4, ALL), R.color_augment(xg, params, ALL))
    if C == 1:  # saturation: v - m == 0 exactly, the input comes back
        assert torch.equal(R.color_augment(xg, params, R.DColor(False, True, False)), xg)


def test_exact_sum_inputs_sum_exactly_in_any_order():
    """What lets the GPU tests demand bit equality, mean included: on k/128 inputs of at most 49,152
    elements the fp32 sum does not depend on the order."""
    for N, S, C in SHAPES:
        x = exact_sum_input(N, S, C, 7)
        assert S * S * C <= 49152 and float(x.abs().max()) <= 1 and torch.equal(x * 128, (x * 128).round())
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(x.to(dt).float(), x)
        for n in range(N):
            v = x[n].reshape(-1).numpy()
            exact = float(x[n].double().sum())
            fwd = np.float32(0)
            for a in v:
                fwd = np.float32(fwd + a)
            rev = np.float32(0)
            for a in v[::-1]:
                rev = np.float32(rev + a)
            strided = np.float32(sum(np.float32(np.sum(v[k::64], dtype=np.float32)) for k in range(64)))
            assert float(fwd) == float(rev) == float(strided) == exact
            assert float(R.color_mean(x)[n]) == float(np.float32(np.float32(exact) / np.float32(S * S * C)))


def _published(x, rb, rs, rc):
    """DiffAugment_pytorch.py's rand_brightness, rand_saturation, rand_contrast (NHWC here), the random
    numbers passed in: fp64."""
    x = x + (rb - 0.5)
    m = x.mean(dim=3, keepdim=True)
    x = (x - m) * (rs * 2) + m
    m = x.mean(dim=(1, 2, 3), keepdim=True)
    return (x - m) * (rc + 0.5) + m


def test_oracle_is_the_published_color_policy():
    N, S, C = 4, 12, 3
    x = torch.tanh(torch.randn(N, S, S, C, generator=torch.Generator().manual_seed(1)))
    params = R.color_params(N, SEED, 5)
    u = (params.double() - torch.tensor([-0.5, 0.0, 0.5], dtype=torch.float64)) / torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    rb, rs, rc = (u[:, i].reshape(N, 1, 1, 1) for i in range(3))
    want = _published(x.double(), rb, rs, rc)
    got = R.color_augment(x, params, ALL)
    assert got.dtype == torch.float32
    assert float((got.double() - want).abs().max()) <= 1e-6  # the Mx + b identity and fp32 rounding
    got64 = R.color_augment(x.double(), params, ALL)
    assert got64.dtype == torch.float64 and float((got64 - want).abs().max()) <= 1e-12
    assert float((got.double() - x.double()).abs().max()) > 1e-2


def test_transpose_is_the_adjoint_and_autograd():
    N, S, C = 3, 6, 3
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(N, S, S, C, generator=gen, dtype=torch.float64)
    g = torch.randn(N, S, S, C, generator=gen, dtype=torch.float64)
    params = R.color_params(N, SEED, 9)
    zero = torch.zeros_like(x)
    for color in SUBSETS:
        Ax = R.color_augment(x, params, color) - R.color_augment(zero, params, color)  # the linear part
        Atg = R.color_augment_transpose(g, params, color)
        lhs, rhs = float((Ax * g).sum()), float((x * Atg).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), color
        xr = x.clone().requires_grad_(True)
        auto, = torch.autograd.grad(R.color_augment(xr, params, color), xr, g)
        assert float((auto - Atg).abs().max()) <= 1e-12, color
    only_b = R.DColor(True, False, False)
    assert torch.equal(R.color_augment_transpose(g, params, only_b), g)  # brightness: the identity


def test_saturation_and_contrast_commute():
    N, S, C = 2, 5, 3
    x = torch.randn(N, S, S, C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    params = R.color_params(N, SEED, 2)
    sat, con = R.DColor(False, True, False), R.DColor(False, False, True)
    a = R.color_augment(R.color_augment(x, params, sat), params, con)
    b = R.color_augment(R.color_augment(x, params, con), params, sat)
    both = R.color_augment(x, params, R.DColor(False, True, True))
    assert float((a - b).abs().max()) <= 1e-12 and float((a - both).abs().max()) <= 1e-12


# ------------------------------------------------------------------ 3. validation and precedence
def test_parser_accepts_subsets_and_names_bad_tokens(monkeypatch):
    assert R.check_d_color("") == R.check_d_color("none") == R.check_d_color(None) == R.DColor()
    assert not R.DColor().active and R.DColor().mask == 0 and R.DColor().describe() == "off"
    names = R.COLOR_POLICIES
    assert names == ("brightness", "saturation", "contrast")
    for color in SUBSETS:
        on = [n for n, v in zip(names, color) if v]
        for perm in itertools.permutations(on):
            assert R.check_d_color(",".join(perm)) == color
        assert color.active and color.describe() == ",".join(on)
        assert color.mask == sum(1 << i for i, v in enumerate(color) if v)
        assert R.check_d_color(color) == color
    assert R.check_d_color(" Contrast , BRIGHTNESS,") == R.DColor(True, False, True)
    assert sorted(c.mask for c in SUBSETS) == [1, 2, 3, 4, 5, 6, 7]
    for bad in ("color", "translation", "brightness,hue", "none,contrast"):
        tok = [t for t in bad.split(",") if t not in names][0]
        with pytest.raises(ValueError, match="unknown policy %r" % tok):
            R.check_d_color(bad)
    with pytest.raises(ValueError):
        R.check_d_color(3)
    # the environment default, and the explicit argument beating it
    monkeypatch.setenv("DCGAN_D_COLOR_AUGMENT", "contrast")
    assert R.resolve_d_color(None) == R.DColor(False, False, True)
    assert R.resolve_d_color("") == R.DColor() and R.resolve_d_color("brightness") == R.DColor(True, False, False)
    assert _hip(small()).color == R.DColor(False, False, True) and not _hip(small(), d_color_augment="none").color.active
    assert ReferenceEngine(small(), 4, CPU).color == R.DColor(False, False, True)
    assert not ReferenceEngine(small(), 4, CPU, d_color_augment="").color.active
    assert not _hip(small()).aug.active  # independent of --d_augment
    monkeypatch.setenv("DCGAN_D_COLOR_AUGMENT", "hue")
    with pytest.raises(ValueError, match="unknown policy 'hue'"):
        _hip(small())


def test_flags_validate_and_d_augment_color_is_still_an_error(capsys):
    fl = F.parse_flags(["--d_color_augment=saturation,brightness"])
    assert fl.d_color_augment == "saturation,brightness" and F.parse_flags([]).d_color_augment == ""
    assert F.parse_flags(["--d_color_augment=none", "--d_augment=cutout"]).d_augment == "cutout"
    with pytest.raises(SystemExit):
        F.parse_flags(["--d_color_augment=brightness,hue"])
    assert "--d_color_augment" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        F.parse_flags(["--d_augment=color"])
    assert "unknown policy 'color'" in capsys.readouterr().err
    with pytest.raises(ValueError, match="unknown policy 'color'"):
        R.check_d_augment("color")
    assert R.AUG_POLICIES == ("translation", "cutout")


# ------------------------------------------------------------------ 4. ReferenceStep
def test_reference_step_applies_color_first_then_geometry_then_noise():
    cfg, B = DCGANConfig(output_size=28, c_dim=1), 4
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    kw = dict(instance_noise=0.3, instance_noise_end=0.3, noise_seed=SEED, d_steps=2)
    st = ReferenceStep(DCGAN(cfg, seed=3), d_color_augment="brightness,contrast", d_augment="translation", **kw)
    assert st.color == R.DColor(True, False, True)
    st.global_step = 2
    seen = {}
    orig = st.model.discriminator

    def spy(x, **k):
        seen["x"] = x.detach().clone()
        return orig(x, **k)
    st.model.discriminator = spy
    out = st.forward_losses(real, z, update_ema=False)
    both = torch.cat([real, out["fake"].detach()], 0)
    cp = R.color_params(2 * B, SEED, 2)
    assert torch.equal(st.draw_color(both.shape), cp)
    want = R.augment(R.color_augment(both, cp, st.color), R.augment_params(2 * B, 28, SEED, 2), st.aug) + st.draw_noise(both.shape)
    assert torch.equal(seen["x"], want)
    st.forward_losses(real, z, update_ema=False, color=cp, sub=0)  # given params win over the sub-step's draw
    assert torch.equal(st.draw_color(both.shape, 0), R.color_params(2 * B, R.substep_seed(SEED, 0), 2))
    assert not torch.equal(st.draw_color(both.shape, 0), cp)
    st.forward_losses(real, z, update_ema=False, color=False, augment=False, noise=False)
    assert torch.equal(seen["x"], both)
    # G's gradient passes back through it: autograd of the step == autograd by hand on the colored input
    st2 = ReferenceStep(DCGAN(cfg, seed=3), d_color_augment="brightness,saturation,contrast", noise_seed=SEED)
    o, fd, fg = st2.compute_grads(real, z, update_ema=False)
    clean = ReferenceStep(DCGAN(cfg, seed=3), noise_seed=SEED)
    o0, fd0, fg0 = clean.compute_grads(real, z, update_ema=False)
    assert float(o["d_loss"].detach()) != float(o0["d_loss"].detach()) and not torch.equal(fg, fg0)
    o1, fd1, fg1 = st2.compute_grads(real, z, update_ema=False, color=R.color_params(2 * B, SEED, 0))
    assert torch.equal(fd, fd1) and torch.equal(fg, fg1)
    # off: bitwise today's step
    a, b = ReferenceStep(DCGAN(cfg, seed=3), d_color_augment=""), ReferenceStep(DCGAN(cfg, seed=3))
    for _ in range(2):
        assert a.step(real, z) == b.step(real, z)
    assert torch.equal(a.model.d.flat, b.model.d.flat) and torch.equal(a.model.g.flat, b.model.g.flat)


def test_reference_engine_uses_the_hip_engines_seed_and_clean_eval_losses():
    cfg, B = small(), 4
    e = ReferenceEngine(cfg, B, CPU, seed=3, rank=2, z_seed=1, d_color_augment="contrast,brightness")
    h = _hip(seed=3, rank=2, z_seed=1, world=4, d_color_augment="contrast,brightness")
    assert e.step_impl.noise_seed == h._zseed(None) == 1 * 1000003 + 17 + 7919 * 2
    assert e.color == h.color == e.step_impl.color == R.DColor(True, False, True)
    plain = ReferenceEngine(cfg, B, CPU, seed=3)
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    assert e.eval_losses(real, z) == plain.eval_losses(real, z)  # sample-time losses stay clean
    e.set_synthetic_batch(real)
    plain.set_synthetic_batch(real)
    e.train_step()
    plain.train_step()
    assert e.last_losses() != plain.last_losses()


# ------------------------------------------------------------------ 5. schedules (dry-run HIP engines)
ON = dict(d_color_augment="brightness,saturation,contrast")
GEO = dict(d_augment="translation,cutout")
NOISE = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=10)
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


def _check_color_ops(eng, d_steps):
    """One d_color per forward, on the main stream, right behind the op writing the fake half and ahead of
    d_aug / d_noise, which read its output; one d_color_bwd per full step behind the image gradient (and
    d_aug_bwd) and ahead of G's tanh backward. What each reads and writes."""
    ex = _record(eng)
    es = 4 if eng.f32 else 2
    nbytes = eng.d_in.numel() * es
    B2 = 2 * eng.B
    step = (eng.step_counter.data_ptr(), 8, False)
    idx = [i for i, op in enumerate(ex.ops) if _name(op) == "d_color"]
    assert len(idx) == d_steps
    for k, i in enumerate(idx):
        op, d_in = ex.ops[i], eng.d_ins[k]
        assert op.stream == "main"
        assert sorted(op.acc) == sorted([(d_in.data_ptr(), nbytes, False), step, (eng.d_colored.data_ptr(), nbytes, True),
                                         (eng.color_params.data_ptr(), B2 * 16, True)])
        assert "g_h" in _name(ex.ops[i - 1]) and any(w for _, _, w in ex.ops[i - 1].acc)
        src, j = eng.d_colored, i + 1
        if eng.aug.active:
            assert _name(ex.ops[j]) == "d_aug"
            assert sorted(ex.ops[j].acc) == sorted([(src.data_ptr(), nbytes, False), step, (eng.d_auged.data_ptr(), nbytes, True),
                                                    (eng.aug_params.data_ptr(), B2 * 16, True)])
            src, j = eng.d_auged, j + 1
        if eng.noise.active:
            assert _name(ex.ops[j]) == "d_noise"
            assert sorted(ex.ops[j].acc) == sorted([(src.data_ptr(), nbytes, False), step, (eng.d_noisy.data_ptr(), nbytes, True)])
            src, j = eng.d_noisy, j + 1
        assert _name(ex.ops[j]).startswith(("d0.", "d_h0")), _name(ex.ops[j])
        assert src is eng._d_input() and any(a == src.data_ptr() and not w for a, _, w in ex.ops[j].acc)
    # the colored copy has exactly one kind of reader: the next stage, or D's layer 0 (forward and weight gradient)
    lo, hi = eng.d_colored.data_ptr(), eng.d_colored.data_ptr() + nbytes
    readers = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
    if eng.aug.active:
        assert readers == {"d_aug"}
    elif eng.noise.active:
        assert readers == {"d_noise"}
    else:
        assert readers and all(r.startswith(("d0.", "d_h0")) for r in readers), readers
    for d_in in eng.d_ins:  # the clean input: read by d_color, never by D's layer 0 or the later stages
        lo, hi = d_in.data_ptr(), d_in.data_ptr() + nbytes
        clean = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
        assert "d_color" in clean and not clean & {"d_aug", "d_noise"}
        assert not any(r.startswith(("d0.", "d_h0")) for r in clean), clean
    # the backward
    names = [_name(o) for o in ex.ops]
    assert names.count("d_color_bwd") == 1 and names.count("g_out.tanh_bwd") == 1
    assert not any("dgrad_img+tanh_bwd" in n for n in names)
    j = names.index("d_color_bwd")
    op, half = ex.ops[j], nbytes // 2
    src = eng.img_grad_t if eng.aug.active else eng.img_grad
    assert sorted(op.acc) == sorted([(src.data_ptr(), half, False), (eng.color_params.data_ptr() + eng.B * 16, eng.B * 16, False),
                                     (eng.img_grad_c.data_ptr(), half, True)])
    if eng.aug.active:
        assert names[j - 1] == "d_aug_bwd" and names[j - 2].endswith(".dgrad_img")
    else:
        assert names[j - 1].endswith(".dgrad_img") and eng.img_grad_t is None
    assert any(a == src.data_ptr() and w for a, _, w in ex.ops[j - 1].acc) and ex.ops[j - 1].stream == op.stream
    t = names.index("g_out.tanh_bwd")
    assert t > j and ex.ops[t].stream == op.stream
    acc = ex.ops[t].acc
    assert any(a == eng.img_grad_c.data_ptr() and not w for a, _, w in acc)
    assert any(a == eng.fake.data_ptr() and not w for a, _, w in acc)  # tanh' at the clean fake
    assert not any(a == src.data_ptr() for a, _, _ in acc)


@pytest.mark.parametrize("extra", [{}, NOISE, GEO, dict(GEO, **NOISE)], ids=["color", "color+noise", "color+geo", "color+geo+noise"])
@pytest.mark.parametrize("world,schedule,wire,d_steps", CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in CASES])
def test_schedules_are_hazard_free_with_the_color_ops(world, schedule, wire, d_steps, extra):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **ON, **extra)
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_color_ops(eng, d_steps)
    assert eng.op_names().count("d_color") == d_steps and eng.op_names().count("d_color_bwd") == 1
    assert all(eng.sub_op_names(k).count("d_color") == 1 and "d_color_bwd" not in eng.sub_op_names(k)
               for k in range(d_steps - 1))


@pytest.mark.parametrize("dtype,size,c_dim", [("fp16", 28, 1), ("fp32", 28, 1), ("fp32", 64, 3), ("bf16", 64, 3),
                                              ("bf16", 128, 3)])
def test_other_dtypes_and_sizes_are_hazard_free_with_the_color_ops(dtype, size, c_dim):
    for world, d_steps, extra in ((1, 1, {}), (2, 3, dict(GEO, **NOISE)), (1, 3, GEO), (2, 1, NOISE)):
        eng = _hip(DCGANConfig(output_size=size, c_dim=c_dim), dtype=dtype, world=world, d_steps=d_steps, **ON, **extra)
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))
        _check_color_ops(eng, d_steps)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free_with_the_color_ops(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    for extra in ({}, dict(GEO, **NOISE)):
        eng = _hip(world=world, **ON, **extra)
        assert eng._sharded()
        hz, n = SC.check_engine(eng)
        assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
        _check_color_ops(eng, 1)


def test_checker_finds_d_color_bwd_moved_ahead_of_d_aug_bwd():
    """d_color_bwd issued on another stream before d_aug_bwd, which writes the buffer it reads, with nothing
    ordering the two: a race on img_grad_t (and on what tanh_bwd reads). Only the accesses to the three
    image-gradient buffers are kept, so the moved op alone decides."""
    eng = _hip(**ON, **GEO)
    assert SC.check_engine(eng)[0] == []
    ex = _record(eng, steps=2)
    names = [_name(o) for o in ex.ops]
    j = names.index("d_color_bwd")
    assert names[j - 1] == "d_aug_bwd"
    op = ex.ops.pop(j)
    op.stream = "planted"  # (a stream nothing waits for)
    op.vc = {"planted": 1}
    ex.ops.insert(j - 1, op)
    bufs = [(b.data_ptr(), b.data_ptr() + b.numel() * 2) for b in (eng.img_grad, eng.img_grad_t, eng.img_grad_c)]
    for o in ex.ops:
        o.acc = [a for a in o.acc if any(lo <= a[0] < hi for lo, hi in bufs)]
    hz = SC.find_hazards(ex.ops)
    assert hz and any("d_color_bwd" in h.a + h.b and "d_aug_bwd" in h.a + h.b for h in hz), "\n".join(map(str, hz))
    assert any("d_color_bwd" in h.a + h.b and "tanh_bwd" in h.a + h.b for h in hz)


def test_with_the_switch_off_the_recorded_ops_are_todays():
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16"),
               dict(dtype="fp32"), NOISE, GEO):
        off, bare = _hip(d_color_augment="", **kw), _hip(**kw)
        assert off.d_colored is None and off.color_params is None and off.img_grad_c is None
        assert bare.d_colored is None and not bare.color.active
        assert off.op_names() == bare.op_names() and not any("d_color" in n for n in bare.op_names())
        assert off.kernel_count() == bare.kernel_count()
        a, b = _record(off), _record(bare)
        assert [(_name(x), x.stream, len(x.acc)) for x in a.ops] == [(_name(x), x.stream, len(x.acc)) for x in b.ops]
        on = _hip(**ON, **kw)
        names = on.op_names()
        if bare._img_dact():  # the fused image gradient + tanh backward (+ its bias-gradient sum) gives way to
            # the unfused image gradient, the transposed color map and G's tanh backward + bias gradient
            want = bare.op_names()
            f = [i for i, n in enumerate(want) if "dgrad_img+tanh_bwd" in n]
            assert f == [f[0], f[0] + 1] and want[f[1]] == want[f[0]] + ".dbias"
            want[f[0]:f[1] + 1] = [want[f[0]][:-len("+tanh_bwd")], "d_color_bwd", "g_out.tanh_bwd"]
            assert [n for n in names if n != "d_color"] == want
        else:
            assert [n for n in names if n not in ("d_color", "d_color_bwd")] == bare.op_names()
        assert on.kernel_count() == bare.kernel_count() + on.d_steps + 1


def test_bindings_record_the_byte_ranges_and_reject_bad_calls():
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    x, y, p, st = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    nb = 2 * 8 * 8 * 3 * 2
    assert prog.d_color("a", x, y, p, 2, 8, 3, 7, 5, st, 0) == 0
    assert prog.d_color("b", x, y, p, 2, 8, 3, 4, 0, 0, 0) == 1
    assert prog.d_color_bwd("c", x, y, p, 2, 8, 3, 6, 0) == 2
    assert sorted(prog.op_info(0)[4]) == sorted([(x, nb, False), (st, 8, False), (y, nb, True), (p, 32, True)])
    assert sorted(prog.op_info(1)[4]) == sorted([(x, nb, False), (p, 32, False), (y, nb, True), (p, 32, True)])  # the probe
    assert sorted(prog.op_info(2)[4]) == sorted([(x, nb, False), (p, 32, False), (y, nb, True)])
    assert H.ext().Program(2, True).d_color("a", x, y, p, 2, 8, 3, 1, 5, st, 0) == 0
    prog = H.ext().Program(0, True)
    ok = (x, y, p, 2, 8, 3, 7)
    bad = [(0,) + ok[1:], ok[:1] + (0,) + ok[2:], ok[:2] + (0,) + ok[3:], (x, x) + ok[2:], ok[:6] + (0,), ok[:6] + (8,),
           ok[:4] + (0,) + ok[5:], ok[:4] + ((1 << 14) + 1,) + ok[5:], ok[:5] + (0, 7), ok[:5] + (5, 7), ok[:3] + (0,) + ok[4:]]
    for a in bad:
        with pytest.raises(RuntimeError, match="d_color"):
            prog.d_color("a", *a, 1, st, 0)
        with pytest.raises(RuntimeError, match="d_color_bwd"):
            prog.d_color_bwd("b", *a, 0)
    assert prog.size() == 0


# (recorded name, output attribute, gates attribute, image-gradient attribute behind its transpose), in running order
WIRING = (("d_color", "d_colored", "color_gates", "img_grad_c"), ("d_aug", "d_auged", "aug_gates", "img_grad_t"),
          ("d_noise", "d_noisy", None, None))
WIRING_CASES = [(c, g, n, ada) for ada in (False, True) for c, g, n in itertools.product((False, True), repeat=3)
                if c or g or not ada]  # (a probability gates a policy: no ADA case where none is on)


@pytest.mark.parametrize("color,geo,noise,ada", WIRING_CASES,
                         ids=["color%d-geo%d-noise%d-ada%d" % c for c in WIRING_CASES])
def test_stages_on_ds_input_chain_buffer_to_buffer_forward_and_back(color, geo, noise, ada):
    """Every on / off combination of the three stages on D's input, without and with a fixed augmentation
    probability: each forward stage reads exactly the buffer the one before it wrote, from d_in on, and D's
    layer 0 (forward and weight gradient) reads the last; the transposes run in reverse from img_grad, and G's
    tanh backward reads the last -- or stays fused into the image gradient where there is no transpose."""
    kw = dict(ON if color else {}, **(GEO if geo else {}), **(NOISE if noise else {}))
    eng = _hip(**kw, **(dict(d_augment_p=0.5) if ada else {}))
    B, nbytes = eng.B, eng.d_in.numel() * 2
    half = nbytes // 2
    info = lambda prog: [prog.op_info(i) for i in range(prog.size())]  # noqa: E731  (name, stream, kind, event, acc)
    opsA, opsB = info(eng.progA), info(eng.progB)
    names = [o[0] for o in opsA]
    on = [w for w, flag in zip(WIRING, (color, geo, noise)) if flag]
    for w, flag in zip(WIRING, (color, geo, noise)):
        if not flag:
            assert all(getattr(eng, a) is None for a in w[1:] if a) and w[0] not in names and w[0] + "_bwd" not in names
    assert (eng.ada_state is not None) == ada
    copies = [eng.d_in] + [getattr(eng, w[1]) for w in on]

    def only_reads(op, buf, n, among):  # of the buffers `among`, op reads `buf` (n bytes from its start) and no other
        assert (buf.data_ptr(), n, False) in op[4], op
        assert not any(a == o.data_ptr() and not wr for a, _, wr in op[4] for o in among if o is not buf), op

    # forward: consecutive ops, each from the copy before it into its own
    i, prev = None, eng.d_in
    for name, out, gates, _ in on:
        assert names.count(name) == 1 and (i is None or names.index(name) == i + 1)
        i, dst = names.index(name), getattr(eng, out)
        only_reads(opsA[i], prev, nbytes, copies)
        assert (dst.data_ptr(), nbytes, True) in opsA[i][4]
        if ada and gates:  # the gated kernel: p24 from the state, the gate masks of all 2B samples out
            assert (eng.ada_state.data_ptr(), 4, False) in opsA[i][4]
            assert (getattr(eng, gates).data_ptr(), 2 * B * 4, True) in opsA[i][4]
        elif ada:
            assert not any(a == eng.ada_state.data_ptr() for a, _, _ in opsA[i][4])
        elif gates:
            assert getattr(eng, gates) is None
        prev = dst
    assert prev is eng._d_input()
    d0 = [o for o in opsA + opsB if o[0].startswith(("d0.", eng.dl[0].name))
          and any(a == c.data_ptr() and not wr for a, _, wr in o[4] for c in copies)]
    assert any(o in opsA for o in d0) and any(o in opsB for o in d0)  # layer 0's forward, and its weight gradient
    for o in d0:
        only_reads(o, prev, nbytes, copies)
    if on:
        assert opsA[i + 1] in d0

    # backward: the transposes in reverse order, behind the image gradient and ahead of G's tanh backward
    back = [w for w in reversed(on) if w[3]]
    if not back:
        assert sum("dgrad_img+tanh_bwd" in n for n in names) >= 1 and "g_out.tanh_bwd" not in names
        assert not any(n.endswith(".dgrad_img") for n in names)
        return
    assert not any("dgrad_img+tanh_bwd" in n for n in names) and names.count("g_out.tanh_bwd") == 1
    grads = [eng.img_grad] + [getattr(eng, w[3]) for w in back]
    j = [k for k, n in enumerate(names) if n.endswith(".dgrad_img")]
    assert len(j) == 1 and (eng.img_grad.data_ptr(), half, True) in opsA[j[0]][4]
    j, prev = j[0], eng.img_grad
    for name, _, gates, grad in back:
        j += 1
        assert names[j] == name + "_bwd" and names.count(names[j]) == 1
        only_reads(opsA[j], prev, half, grads)
        assert (getattr(eng, grad).data_ptr(), half, True) in opsA[j][4]
        if ada:  # the gate rows the forward recorded for the fake half
            assert (getattr(eng, gates).data_ptr() + B * 4, B * 4, False) in opsA[j][4]
        prev = getattr(eng, grad)
    assert names[j + 1] == "g_out.tanh_bwd"
    only_reads(opsA[j + 1], prev, half, grads)


# ------------------------------------------------------------------ 6. trainer / CLI
def test_cli_runs_with_the_color_policy_on_the_reference_engine(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=2", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=4", "--sample_every=0", "--nosummaries", "--epoch=0", "--d_color_augment=contrast,brightness",
            "--d_augment=cutout", "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "color augmentation of D's inputs: brightness,contrast" in p.stdout
    assert "differentiable augmentation of D's inputs: cutout" in p.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--d_color_augment=hue"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "unknown policy 'hue'" in bad.stdout


def test_trainer_prints_nothing_with_the_switch_off(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32", "--max_steps=1",
                        "--epoch=0", "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
                        "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    assert "color augmentation" not in out.getvalue()
