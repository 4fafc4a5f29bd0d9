"""GPU tests of the instance noise on D's inputs: the normals and sigma probes against the fp64 oracle,
the noise kernel (bf16 / fp16 / fp32 builds) against x + sigma * eps in fp64, the engine's noisy
buffer against the oracle (full step and D sub-steps), steps against ``ReferenceStep`` with the
oracle's noise passed in (the comparison and tolerances of test_hip_d_steps.py, unchanged), hipGraph
replay, the end of the anneal, an inactive 0 -> 0 anneal, clean sample-time losses, one-rank RCCL DDP
and resume through the trainer.

Bounds. Normals: the device's largest absolute error against the fp64 oracle <= 4 x the largest
error of the fp32 numpy oracle on the same inputs (computed in the test). Kernel: with eps from the
device probe and exact = x + sigma * eps in fp64, |y - exact| <= 1/2 ulp_elem(exact) + 1 ulp_fp32(exact)
(one fp32 rounding of the fma, one rounding to the element type; fp32: the second term alone).
Against the fp64 oracle's eps the engine test adds sigma x (4 x the fp32 oracle's error): the
normals' own bound, scaled.

Shapes: n in {5, 8, 1027, 12544}: less than one 16-byte access, exactly one, body + scalar tail over
several blocks, D's stacked 28x28x1 input at B = 8; plus a view one element off 16-byte alignment
(the all-scalar path). Engines at 28x28x1 and 64x64x3, B = 8."""
import io
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

import test_hip_d_spectral_norm as SNT
import test_hip_d_steps as TD
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BUILDS = SNT.BUILDS
PAD = SNT.PAD
_padded, _canaries_intact = SNT._padded, SNT._canaries_intact
ENV = TD.ENV + ("DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS", "DCGAN_LR_DECAY",
                "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP")
SIZES = [5, 8, 1027, 2 * 8 * 28 * 28]
SEEDS = [1000020, 0xFEDCBA9876543210]
STEPS_T = [0, 1, (1 << 32) + 3]
NOISE = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=4)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def small():
    return DCGANConfig(output_size=28, c_dim=1)


def _step(t):
    return torch.tensor([t], dtype=torch.int64, device=dev)


# ------------------------------------------------------------------ 1. the probes
@pytest.fixture(scope="module")
def oracle_err():
    """Largest |fp32 numpy oracle - fp64 oracle| over the probe's inputs (computed once)."""
    worst = 0.0
    for n in SIZES:
        for seed in SEEDS:
            for t in STEPS_T:
                a, b = R.philox_normal(n, seed, t, 1), R.philox_normal(n, seed, t, 1, dtype=torch.float32)
                worst = max(worst, float((b.double() - a).abs().max()))
    return worst


def test_normals_probe_matches_the_fp64_oracle(oracle_err):
    """Measured on an MI355X: largest absolute error of the device 4.50e-7, of the fp32 numpy oracle
    1.35e-6 on the same inputs (bound: 4 x the latter)."""
    h = H()
    worst = 0.0
    for n in SIZES:
        for seed in SEEDS:
            for t in STEPS_T:
                buf, view = _padded(torch.zeros(n))
                step = _step(t)
                view.copy_(h.philox_normal(n, seed, step, 1))
                got = h.philox_normal(n, seed, step, 1).cpu()
                assert torch.equal(got, view.cpu()) and _canaries_intact(buf) and int(step) == t
                want = R.philox_normal(n, seed, t, 1)
                worst = max(worst, float((got.double() - want).abs().max()))
    print("philox_normal: largest abs error device %.3e, fp32 numpy oracle %.3e (bound 4 x)" % (worst, oracle_err))
    assert 0 < oracle_err < 1e-5 and worst <= 4 * oracle_err
    # stream 0 (z's) and another seed draw other numbers
    a = h.philox_normal(64, SEEDS[0], _step(0), 1)
    assert not torch.equal(a, h.philox_normal(64, SEEDS[0], _step(0), 0))
    assert not torch.equal(a, h.philox_normal(64, SEEDS[0] + 1, _step(0), 1))


def test_normals_probe_statistics():
    """The 5-sigma bounds of tests/test_instance_noise.py, on the device's draws (fp64 arithmetic)."""
    h = H()
    n = 1 << 20
    e = {t: h.philox_normal(n, 1000020, _step(t), 1).double() for t in (0, 1, 7)}

    def corr(a, b):
        return float(torch.corrcoef(torch.stack([a, b]))[0, 1])
    for t, x in e.items():
        z1 = abs(float(x.mean())) * math.sqrt(n)
        z2 = abs(float(x.var(unbiased=False)) - 1) / math.sqrt(2 / n)
        z3 = abs(corr(x[:n // 2], x[n // 2:])) * math.sqrt(n / 2)
        print("device step %d: Z1 %.2f Z2 %.2f Z3 %.2f" % (t, z1, z2, z3))
        assert z1 <= 5 and z2 <= 5 and z3 <= 5, (t, z1, z2, z3)
        assert float(x.abs().max()) <= math.sqrt(48 * math.log(2)) * (1 + 1e-6)
    z = abs(corr(e[0], e[1])) * math.sqrt(n)
    print("device step 0 / step 1 correlation statistic %.2f" % z)
    assert z <= 5


M = 1 << 24
# (sigma0, sigma1, steps): every end is an fp32 number, so fp32 and fp64 see the same schedule
SIGMA = [(0.25, 0.0625, 5000), (2.0, 0.0, M), (0.0, 1.5, 7), (0.5, 0.5, 1), (1.0, 0.75, 1)]


def test_sigma_probe_matches_fp64():
    h = H()
    worst_dev = worst_cpu = 0.0
    for s0, s1, steps in SIGMA:
        ts = {0, 1, 2, steps // 3, steps // 2, steps - 1, steps, steps + 1, M - 1, M, M + 1, (1 << 32) + 3, 1 << 40}
        ts |= {(steps * i) // 97 for i in range(98)}
        t = torch.tensor(sorted(ts), dtype=torch.int64)
        buf, view = _padded(torch.zeros(t.numel()))
        view.copy_(h.noise_sigma(t.to(dev), s0, s1, steps))
        got = view.cpu()
        assert _canaries_intact(buf)
        want = R.noise_sigma(t, s0, s1, steps, dtype=torch.float64)
        cpu = R.noise_sigma(t, s0, s1, steps)
        e_dev, e_cpu = float((got.double() - want).abs().max()), float((cpu.double() - want).abs().max())
        print("noise_sigma %g -> %g over %d: max abs error device %.3e, fp32 oracle %.3e" % (s0, s1, steps, e_dev, e_cpu))
        worst_dev, worst_cpu = max(worst_dev, e_dev), max(worst_cpu, e_cpu)
        assert float(got[0]) == s0  # t = 0
        assert bool((got[t >= steps] == s1).all()) if s0 != s1 else bool((got == s0).all())
    assert worst_dev <= 4 * worst_cpu


# ------------------------------------------------------------------ 2. the noise kernel
def _ulp(v, build):
    """ulp of the element type at |v| (fp64 tensor); fp16 / fp32 / bf16 subnormal spacing below the
    smallest normal."""
    mant, emin = {"bf16": (7, -126), "fp16": (10, -14), "fp32": (23, -126)}[build]
    e = torch.frexp(v.abs().clamp_min(1e-300))[1].double() - 1  # floor(log2 |v|)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.clamp_min(emin) - mant)


def _bound(exact, build):
    one32 = _ulp(exact, "fp32")
    return one32 if build == "fp32" else 0.5 * _ulp(exact, build) + one32


@pytest.mark.parametrize("build", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_noise_kernel_matches_fp64(n, build):
    h = H()
    edt = BUILDS[build]
    seed, t = SEEDS[0], 3
    s0, s1, steps = 0.75, 0.25, 8
    x0 = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 2 - 1).to(edt)
    if n >= 8:
        x0[0], x0[1] = 0.0, -0.0
    xb, x = _padded(x0.float(), dtype=edt)
    yb, y = _padded(torch.zeros(n), dtype=edt)
    step = _step(t)
    assert h.instance_noise(x, y, seed, step, s0, s1, steps) is y
    torch.cuda.synchronize()
    assert _canaries_intact(yb) and _canaries_intact(xb) and torch.equal(x.cpu(), x0) and int(step) == t
    sig = h.noise_sigma(step, s0, s1, steps).cpu().double()
    assert float(sig) == float(R.noise_sigma(t, s0, s1, steps)) == 0.5625
    eps = h.philox_normal(n, seed, step, 1).cpu().double()
    exact = x0.double() + sig * eps
    err = (y.cpu().double() - exact).abs()
    bound = _bound(exact, build)
    k = int((err / bound).argmax())
    print("instance_noise %s n=%d: largest |y - exact| / bound %.3f (|exact| %.3e)" % (build, n, float(err[k] / bound[k]),
                                                                                     float(exact[k].abs())))
    assert bool((err <= bound).all())
    first = y.cpu().clone()
    # the same step again: the same bits; the next step: others
    h.instance_noise(x, y, seed, step, s0, s1, steps)
    assert torch.equal(y.cpu(), first)
    h.instance_noise(x, y, seed, _step(t + 1), s0, s1, steps)
    assert not torch.equal(y.cpu(), first) and _canaries_intact(yb)
    # one element off 16-byte alignment (all-scalar path): the element -> (counter, lane) map is the same
    xb2 = torch.full((n + 2 * PAD + 1,), 7.0, dtype=edt, device=dev)
    yb2 = torch.full((n + 2 * PAD + 1,), 7.0, dtype=edt, device=dev)
    x2, y2 = xb2[PAD + 1:PAD + 1 + n], yb2[PAD + 1:PAD + 1 + n]
    x2.copy_(x0)
    h.instance_noise(x2, y2, seed, step, s0, s1, steps)
    assert torch.equal(y2.cpu(), first)
    assert bool((yb2[:PAD + 1] == 7.0).all()) and bool((yb2[PAD + 1 + n:] == 7.0).all())
    # sigma(t) == 0: a bitwise copy (signed zeros included), at the end of an anneal and as 0 -> 0
    for a, b, c, tt in ((0.5, 0.0, 3, 3), (0.5, 0.0, 3, 1 << 40), (0.0, 0.0, 1, 0)):
        y.fill_(3.0)
        h.instance_noise(x, y, seed, _step(tt), a, b, c)
        assert torch.equal(y.view(torch.int16 if build != "fp32" else torch.int32).cpu(),
                           x.view(torch.int16 if build != "fp32" else torch.int32).cpu())
    assert _canaries_intact(yb) and torch.equal(x.cpu(), x0)


def test_the_two_halves_carry_different_noise():
    h = H()
    B, per = 8, 28 * 28
    n = 2 * B * per
    x = torch.zeros(n, device=dev)
    y = torch.empty_like(x)
    h.instance_noise(x, y, SEEDS[0], _step(0), 1.0, 1.0, 1)
    real, fake = y[:B * per].cpu(), y[B * per:].cpu()
    assert not torch.equal(real, fake) and float(real.std()) > 0.9 and float(fake.std()) > 0.9
    c = float(torch.corrcoef(torch.stack([real, fake]))[0, 1])
    assert abs(c) * math.sqrt(B * per) <= 5
    assert torch.equal(y.cpu(), h.philox_normal(n, SEEDS[0], _step(0), 1).cpu())  # x = 0, sigma = 1: eps itself


def test_bindings_reject_null_pointers_and_bad_schedules():
    h = H()
    x = torch.zeros(64, device=dev, dtype=torch.bfloat16)
    y = torch.zeros(64, device=dev, dtype=torch.bfloat16)
    step = _step(0)
    P_ = lambda t: t.data_ptr()  # noqa: E731
    prog = h.ext().Program()
    for bad in ((0, P_(y), P_(step)), (P_(x), 0, P_(step)), (P_(x), P_(y), 0), (P_(x), P_(x), P_(step))):
        with pytest.raises(RuntimeError, match="instance_noise"):
            prog.instance_noise("n", bad[0], bad[1], 64, 1, bad[2], 1, 0.2, 0.1, 10)
    for s0, s1, steps in ((-0.1, 0.1, 10), (0.2, 2.5, 10), (float("nan"), 0.1, 10), (0.2, float("inf"), 10),
                          (0.2, 0.1, 0), (0.2, 0.1, M + 1)):
        with pytest.raises(RuntimeError, match="instance_noise"):
            prog.instance_noise("n", P_(x), P_(y), 64, 1, P_(step), 1, s0, s1, steps)
        with pytest.raises(RuntimeError, match="noise_sigma"):
            h.noise_sigma(torch.zeros(4, dtype=torch.int64, device=dev), s0, s1, steps)
    with pytest.raises(RuntimeError, match="philox_normal"):
        prog.philox_normal("p", 0, 8, 1, P_(step), 1)
    with pytest.raises(RuntimeError, match="philox_normal"):
        prog.philox_normal("p", P_(x), 8, 1, 0, 1)
    assert prog.size() == 0
    with pytest.raises(TypeError):
        h.instance_noise(x, y.float(), 1, step, 0.2, 0.1, 10)
    with pytest.raises(TypeError):
        h.instance_noise(x, y, 1, torch.zeros(1, device=dev), 0.2, 0.1, 10)
    with pytest.raises(TypeError):
        h.noise_sigma(torch.zeros(4, device=dev), 0.2, 0.1, 10)
    with pytest.raises(TypeError):
        h.philox_normal(8, 1, torch.zeros(2, dtype=torch.int64, device=dev))


# ------------------------------------------------------------------ 3. the engine's noisy buffer
def _check_noisy(eng, d_in, seed, t, dtype, oracle_err, tag):
    """d_noisy against d_in + sigma(t) * eps: eps from the device probe within the kernel's bound, and
    from the fp64 oracle within that bound + sigma x (the probe's own bound, 4 x the fp32 oracle's error)."""
    h = H()
    n = d_in.numel()
    step = _step(t)
    nz = eng.noise
    sig = float(h.noise_sigma(step, nz.sigma0, nz.sigma1, nz.steps))
    assert abs(sig - float(R.noise_sigma(t, nz.sigma0, nz.sigma1, nz.steps, dtype=torch.float64))) <= 2.0 ** -22
    x = d_in.flatten().cpu().double()
    y = eng.d_noisy.flatten().cpu().double()
    exact = x + sig * h.philox_normal(n, seed, step, 1).cpu().double()
    bound = _bound(exact, dtype)
    assert bool(((y - exact).abs() <= bound).all()), tag
    exact = x + sig * R.philox_normal(n, seed, t, 1)
    err = (y - exact).abs()
    assert bool((err <= _bound(exact, dtype) + sig * 4 * oracle_err).all()), tag
    assert float((y - x).std()) > 0.5 * sig > 0, tag
    return sig


@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 28, 1), ("fp16", 28, 1), ("fp32", 28, 1), ("bf16", 64, 3),
                                              ("fp32", 64, 3)])
def test_engine_noisy_buffer_is_the_oracles_and_z_is_untouched(dtype, size, c_dim, oracle_err):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = TD._engine(cfg, 8, 1, dtype=dtype, seed=3, **NOISE)
    off = TD._engine(cfg, 8, 1, dtype=dtype, seed=3)
    assert eng.d_noisy is not None and eng.d_noisy.shape == eng.d_in.shape and eng.d_noisy.dtype == eng.d_in.dtype
    assert off.d_noisy is None and off.noise_sigma() == 0.0
    assert [n for n in eng.op_names() if n != "d_noise"] == off.op_names() and eng.op_names().count("d_noise") == 1
    sigs = []
    for t in range(3):
        assert eng.global_step == t and eng.noise_sigma() == float(R.noise_sigma(t, 0.2, 0.05, 4))
        eng.train_step()
        off.train_step()
        torch.cuda.synchronize()
        sigs.append(_check_noisy(eng, eng.d_in, eng._zseed(None), t, dtype, oracle_err, "step %d" % t))
        assert torch.equal(eng.z, off.z)  # z keeps stream 0: bitwise what it is without the noise
        if t == 0:  # (same weights so far: the clean input is the same too, and the step differs after it)
            assert torch.equal(eng.d_in, off.d_in) and eng.last_losses() != off.last_losses()
    assert sigs[0] == float(torch.tensor(0.2)) and sigs[0] > sigs[1] > sigs[2] > 0.05


def test_sub_steps_draw_their_own_noise(oracle_err):
    eng = TD._engine(small(), 8, 3, seed=6, **NOISE)
    assert eng.op_names().count("d_noise") == 3 and all(eng.sub_op_names(k).count("d_noise") == 1 for k in range(2))
    seen = []
    for t in range(2):
        for k, run in ((0, lambda: eng.train_d_step(0)), (1, lambda: eng.train_d_step(1)), (None, eng.train_full_step)):
            run()
            torch.cuda.synchronize()
            d_in = eng.d_in if k is None else eng.d_ins[k]
            # (the sub-steps see the global step of the full step after them)
            _check_noisy(eng, d_in, eng._zseed(k), t, "bf16", oracle_err, "step %d piece %s" % (t, k))
            seen.append((eng.d_noisy.float() - d_in.float()).cpu())
        assert eng.global_step == t + 1
    for i in range(len(seen)):
        for j in range(i):
            assert not torch.equal(seen[i], seen[j]), (i, j)


# ------------------------------------------------------------------ 4. against ReferenceStep
class _WithNoise:
    """ReferenceStep behind the two calls ``_check_piece`` makes, the oracle's noise passed as noise=."""

    def __init__(self, ref):
        self.ref, self.noise = ref, None

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, noise=self.noise)

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z, noise=self.noise)


def _noisy_piece(eng, ref, ref_model, cfg, real, dtype, sn, k, run, tag, rdev):
    ref.noise = R.instance_noise(tuple(eng.d_in.shape), eng.noise, eng._zseed(k), eng.global_step).to(rdev)
    assert float(ref.noise.abs().max()) > 0
    TD._check_piece(eng, ref, ref_model, cfg, real, dtype, sn, k is None, run, tag)


@pytest.mark.parametrize("dtype,size,c_dim", [("fp32", 28, 1), ("bf16", 28, 1), ("fp16", 28, 1), ("bf16", 64, 3)])
def test_four_noisy_steps_track_the_reference(dtype, size, c_dim, seed=3):
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **NOISE)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False)
    ref = _WithNoise(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    for s in range(4):
        _noisy_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)
    assert eng.global_step == 4 and eng.noise_sigma() == float(torch.tensor(0.05))


def test_noisy_cycle_with_sub_steps_and_spectral_norm_tracks_the_reference(seed=4):
    cfg, B, dtype = DCGANConfig(output_size=28, c_dim=1, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, **NOISE)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2)
    ref = _WithNoise(ref)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    _noisy_piece(eng, ref, ref_model, cfg, reals[0], dtype, True, 0, lambda: eng.train_d_step(0), "sub-step", rdev)
    _noisy_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, None, eng.train_full_step, "full", rdev)
    assert eng.global_step == 1


# ------------------------------------------------------------------ 5. graph == eager, end of the anneal, 0 -> 0
@pytest.mark.parametrize("dtype,d_steps", [("bf16", 2), ("fp16", 1)])
def test_graph_replay_follows_the_live_counter(dtype, d_steps):
    """A step baked in at capture time would repeat the first replay's noise."""
    kw = dict(dtype=dtype, seed=1, **NOISE)
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    prev = None
    for _ in range(4):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
        assert torch.equal(e1.d_noisy, e2.d_noisy)
        eps = (e2.d_noisy.float() - e2.d_in.float()).cpu()
        assert prev is None or not torch.equal(eps[:8], prev[:8])  # (the real half: the same clean batch every step)
        prev = eps
    assert e2.graph_enabled and not e1.graph_enabled and e1.global_step == e2.global_step == 4


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_after_the_anneal_ends_at_zero_the_input_is_clean(dtype):
    eng = TD._engine(small(), 8, 1, dtype=dtype, seed=2, instance_noise=0.2, instance_noise_end=0.0,
                     instance_noise_steps=2)
    for t in range(4):
        eng.train_step()
        torch.cuda.synchronize()
        same = torch.equal(eng.d_noisy, eng.d_in)
        assert same == (t >= 2), t
    assert eng.noise_sigma() == 0.0 and eng.noise.active


def test_an_anneal_from_zero_to_zero_is_inactive():
    cfg = small()
    a = TD._engine(cfg, 8, 2, seed=2, instance_noise=0.0, instance_noise_end=0.0, instance_noise_steps=1000)
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    b = HipEngine(cfg, 8, dev, seed=2, graph=False, d_steps=2)  # built without the arguments
    for k, x in enumerate(TD._reals(8, cfg, "bf16", 2)):
        b.set_batch(x.to(dev), k)
    assert not a.noise.active and a.d_noisy is None and b.d_noisy is None
    assert a.op_names() == b.op_names() and "d_noise" not in a.op_names() and a.kernel_count() == b.kernel_count()
    assert a.sub_op_names(0) == b.sub_op_names(0)
    for _ in range(3):
        a.train_step()
        b.train_step()
    for x, y in zip(TD._snap(a), TD._snap(b)):
        assert torch.equal(x, y)


def test_eval_losses_stay_clean():
    cfg, B = small(), 8
    on = TD._engine(cfg, B, 1, seed=2, instance_noise=0.5, instance_noise_end=0.5)
    off = TD._engine(cfg, B, 1, seed=7)
    on.train_step()
    torch.cuda.synchronize()
    for name in ("g", "d"):
        getattr(off.model, name).flat.copy_(getattr(on.model, name).flat)
    off.after_state_load()
    real = TD._reals(B, cfg, "bf16", 3)[2]
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    noisy_before = on.d_noisy.clone()
    a, b = on.eval_losses(real, z), off.eval_losses(real, z)
    assert a == b and a["d_loss"] > 0
    assert torch.equal(on.d_noisy, noisy_before)  # no noise op ran
    names = [on.progEval.name(i) for i in range(on.progEval.size())]
    assert "d_noise" not in names and names == [off.progEval.name(i) for i in range(off.progEval.size())]


# ------------------------------------------------------------------ 6. one-rank RCCL DDP
STEPS = 3


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, **NOISE)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "pd": eng.opt_d.powers.cpu(), "pg": eng.opt_g.powers.cpu(),
            "losses": eng.losses.cpu(), "noisy": eng.d_noisy.cpu()}


def _rccl_worker(out_dir, schedule, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["DCGAN_FORCE_DDP"] = "1"
    os.environ["DCGAN_DDP_SCHEDULE"] = schedule
    os.environ["DCGAN_DDP_SHARD"] = "0"
    os.environ.pop("DCGAN_DIST_BACKEND", None)
    torch.cuda.set_device(0)
    from distributed_tensorflow_for_dcgan_amd.parallel import dist as D
    import torch.distributed as tdist
    D.init_distributed(1, 0, torch.device("cuda", 0))
    eng = _ddp_engine(True)
    assert eng.ddp and eng._schedule() == schedule and eng.noise.active
    for _ in range(STEPS):
        eng.train_step()
    out = _result(eng)
    out.update({"step": eng.global_step, "backend": tdist.get_backend(), "graph": eng.graph_enabled,
                "ops": eng.op_names()})
    torch.save(out, os.path.join(out_dir, "rccl.pt"))
    D.barrier()
    D.shutdown()


@pytest.fixture(scope="module")
def fused_run():
    old = {k: os.environ.pop(k, None) for k in ENV}
    try:
        eng = _ddp_engine(True)
        assert not eng.ddp and eng._schedule() == "fused"
        for _ in range(STEPS):
            eng.train_step()
        return _result(eng)
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("schedule", ["concurrent", "ddp"])
def test_rccl_single_rank_ddp_matches_fused_with_noise(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert r["ops"].count("d_noise") == 1
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k


# ------------------------------------------------------------------ 7. resume through the trainer
def test_trainer_resume_is_exact_mid_anneal(tmp_path, monkeypatch):
    """bf16: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more, with the anneal under
    way at the restart -- every saved tensor bitwise, and no key beyond the noise-free run's."""
    from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
    from distributed_tensorflow_for_dcgan_amd.data import pipeline as P
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    from distributed_tensorflow_for_dcgan_amd.utils import flags as F

    def source(flags, batch, shape, device, **kw):
        class Two:
            num_examples = 1 << 20

            def __init__(self):
                self.i = 0
                self.x = [P.SyntheticSource(batch, shape, device, seed=s).next().to(torch.bfloat16) for s in (1, 2)]

            def next(self):
                self.i += 1
                return self.x[self.i % 2]

            def stats(self):
                return {"source": "test"}

            def close(self):
                pass
        return Two()
    monkeypatch.setattr(T, "make_source", source)
    NF = ["--instance_noise=0.3", "--instance_noise_end=0.1", "--instance_noise_steps=6"]

    def run(ck, steps, nf=NF):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + nf)
        out = io.StringIO()
        assert T.run(fl, out=out) == 0, out.getvalue()
        return out.getvalue()

    def load(ck):
        from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
        eng = HipEngine(small(), 8, dev, seed=99, graph=False)
        info = CK.CheckpointManager(str(ck)).restore_latest(eng)
        torch.cuda.synchronize()
        return info, CK.collect_state(eng)
    text = run(tmp_path / "a", 4)
    assert "instance noise on D's inputs: sigma 0.3 to 0.1 over 6 steps" in text
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    run(tmp_path / "c", 4, nf=[])  # without the noise: another model, under the same keys
    ic, sc = load(tmp_path / "c")
    assert list(sc) == list(sa) and any(not (sa[k] == sc[k]).all() for k in sa)
