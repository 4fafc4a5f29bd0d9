"""GPU tests of DiffAugment's color policy on D's inputs (brightness, saturation, contrast): the kernel's
draws against the oracle, the forward and the transpose against ``ops.reference.color_augment`` /
``color_augment_transpose`` (bf16 / fp16 / fp32 builds, canary-padded buffers, the 16-byte and the element
path), the engine's colored buffer and recorded params (full step and D sub-steps), the three stages in
order, the g_loss chain stage by stage, steps against ``ReferenceStep`` with the oracle's draws passed in
(the comparison and tolerances of test_hip_d_steps.py, as test_hip_d_augment.py uses them), hipGraph
replay, the switch off, clean sample-time losses, one-rank RCCL DDP and resume through the trainer.

Exact-sum inputs (values k/128, |k| <= 128, at most 49,152 per image) sum exactly in fp32 in any order
(tests/test_d_color.py proves it on the CPU), so on them the whole definition is bitwise, the mean
included. On general inputs the recorded mean is held to Higham's bound for a sum in any order plus the
division's rounding, the forward is bitwise the oracle at the recorded mean, and the transpose -- whose
mean is not recorded -- to half an ulp of the element type plus the mean's bound scaled by |1 - c| plus
eight fp32 roundings of the largest value. Measured on an MI355X (profiles/r16/d_color_r16.txt)."""
import io
import itertools
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
ENV = TD.ENV + ("DCGAN_D_COLOR_AUGMENT", "DCGAN_D_AUGMENT", "DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END",
                "DCGAN_INSTANCE_NOISE_STEPS", "DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS",
                "DCGAN_LR_END", "DCGAN_LR_WARMUP")
SEEDS = [1000020, 0xFEDCBA9876543210]
STEPS_T = [0, 1, (1 << 32) + 3]
SHAPES = [(3, 8, 3), (1, 5, 3), (2, 6, 4), (2, 28, 1), (2, 28, 3), (2, 64, 3), (1, 128, 3)]  # (N, S, C)
ALL = R.DColor(True, True, True)
SUBSETS = [R.DColor(*bits) for bits in itertools.product((False, True), repeat=3) if any(bits)]
COLOR = dict(d_color_augment="brightness,saturation,contrast")
GEO = dict(d_augment="translation,cutout")
NOISE = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=4)
FILL = 7.0
MANT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}  # (fraction bits, min exponent)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def small():
    return DCGANConfig(output_size=28, c_dim=1)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _slot(shape, dtype, off=0):
    """A view of `shape` `off` elements past a 16-byte boundary, PAD canaries on both sides: (buffer, view)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * PAD + off,), FILL, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off:PAD + off + n].view(shape)


def _intact(buf, off=0):
    return bool((buf[:PAD + off] == FILL).all()) and bool((buf[-PAD:] == FILL).all())


def _exact(N, S, C, seed):
    """Values k/128, |k| <= 128: exact in every build, and their fp32 sum is exact in any order."""
    k = torch.randint(-128, 129, (N, S, S, C), generator=torch.Generator().manual_seed(seed))
    return k.float() / 128


def _ulp(v, dtype):
    """ulp of the element type at |v| (fp64 in, fp64 out)."""
    p, emin = MANT[dtype]
    e = torch.frexp(v.abs().double())[1].double() - 1  # floor(log2 |v|)
    e = torch.where(v == 0, torch.full_like(e, emin), e)
    return torch.exp2(e.clamp(min=emin) - p)


def _mean_bound(x64):
    """Higham's bound for an fp32 sum of n terms in any order, divided by n, plus the division's rounding:
    (n - 1) 2^-24 mean|x| + 2^-24 |Mx|, per image."""
    n = x64[0].numel()
    flat = x64.reshape(x64.shape[0], -1)
    return (n - 1) * 2.0 ** -24 * flat.abs().mean(1) + 2.0 ** -24 * flat.mean(1).abs()


# ------------------------------------------------------------------ 1. the draws
def test_draw_probe_equals_the_oracle_and_stays_in_range():
    h = H()
    for seed in SEEDS:
        for t in STEPS_T:
            got = h.color_params(64, seed, t)
            assert got.dtype == torch.float32 and tuple(got.shape) == (64, 4)
            assert torch.equal(got[:, :3].cpu(), R.color_params(64, seed, t)) and not bool(got[:, 3].any())
    a = h.color_params(16, SEEDS[0], torch.tensor([1], dtype=torch.int64, device=dev))  # a device counter
    assert torch.equal(a[:, :3].cpu(), R.color_params(16, SEEDS[0], 1))
    assert not torch.equal(a, h.color_params(16, SEEDS[0] + 1, 1))
    p = h.color_params(4096, SEEDS[1], 5).cpu()
    assert torch.equal(p[:, :3], R.color_params(4096, SEEDS[1], 5))
    b, s, c = p[:, 0], p[:, 1], p[:, 2]
    assert -0.5 <= float(b.min()) and float(b.max()) < 0.5 and 0 <= float(s.min()) and float(s.max()) < 2
    assert 0.5 <= float(c.min()) and float(c.max()) <= 1.5


# ------------------------------------------------------------------ 2. the kernel on exact-sum inputs: bitwise
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("build", list(BUILDS))
def test_kernels_are_bitwise_the_oracle_on_exact_sum_inputs(build, shape):
    h = H()
    dtype = BUILDS[build]
    N, S, C = shape
    full = (N, S, S, C)
    x0, g0 = _exact(N, S, C, 7).to(dtype), _exact(N, S, C, 8).to(dtype)
    seed, t = SEEDS[1], STEPS_T[2]
    drawn = R.color_params(N, seed, t)
    Mx = R.color_mean(x0.float())
    offs = (0, 1) if shape in ((3, 8, 3), (2, 64, 3)) else (0,)  # one element off 16-byte alignment: the element path
    for off in offs:
        xb, x = _slot(full, dtype, off)
        x.copy_(x0)
        gb, g = _slot(full, dtype, off)
        g.copy_(g0)
        for color in SUBSETS:
            yb, y = _slot(full, dtype, off)
            pb = torch.full((4 * N + 2 * PAD,), -3.0, dtype=torch.float32, device=dev)
            p = pb[PAD:PAD + 4 * N].view(N, 4)
            out, pout = h.color_draw(x, seed, t, color, out=y, params_out=p)
            assert out.data_ptr() == y.data_ptr() and pout.data_ptr() == p.data_ptr()
            assert torch.equal(p[:, :3].cpu(), drawn) and bool((pb[:PAD] == -3).all()) and bool((pb[-PAD:] == -3).all())
            assert torch.equal(p[:, 3].cpu(), Mx if color.contrast else torch.zeros(N)), (off, color)
            assert _same_bits(y, R.color_augment(x0, drawn, color)), (off, color)
            assert _intact(yb, off)
            # the probe entry under the same params: the same bytes, Mx written back
            yb2, y2 = _slot(full, dtype, off)
            p2 = torch.full((N, 4), -3.0, device=dev)
            h.color_apply(x, drawn, color.describe(), out=y2, params_out=p2)
            assert _same_bits(y2, y) and torch.equal(p2, p) and _intact(yb2, off)
            # the transpose
            tb, tg = _slot(full, dtype, off)
            h.color_apply(g, drawn, color, transpose=True, out=tg)
            assert _same_bits(tg, R.color_augment_transpose(g0, drawn, color)), (off, color)
            assert _intact(tb, off)
            if C == 1 and color == R.DColor(False, True, False):  # v - m == 0: the input's bits come back
                assert _same_bits(y, x0) and _same_bits(tg, g0)
        assert _same_bits(x, x0) and _intact(xb, off) and _same_bits(g, g0) and _intact(gb, off)  # only read
    if S > 6:  # the policies differ, and the colored image is not the input
        ys = [h.color_apply(x0.to(dev), drawn, c) for c in (SUBSETS[0], SUBSETS[3], ALL)]
        assert not _same_bits(ys[0], ys[1]) and not _same_bits(ys[0], ys[2]) and not _same_bits(ys[2], x0.to(dev))


def test_placement_and_batch_size_do_not_change_an_image():
    """The same image under the same (b, s, c) at n = 0 of N = 1 and at n = 2 of N = 3: identical bytes and an
    identical recorded Mx (general inputs: the order of the sum would show), forward and transpose; and
    two runs are identical."""
    h = H()
    gen = torch.Generator().manual_seed(4)
    for dtype, (S, C) in itertools.product(BUILDS.values(), [(28, 1), (64, 3), (128, 3), (5, 3)]):
        img = torch.tanh(torch.randn(1, S, S, C, generator=gen)).to(dtype).to(dev)
        three = torch.cat([torch.randn(2, S, S, C, generator=gen).to(dtype).to(dev), img], 0)
        row = torch.tensor([[0.25, 1.7, 0.6]])
        rows = torch.cat([torch.tensor([[-0.4, 0.3, 1.4], [0.1, 1.0, 1.0]]), row], 0)
        p1, p3 = torch.zeros(1, 4, device=dev), torch.zeros(3, 4, device=dev)
        y1 = h.color_apply(img, row, ALL, params_out=p1)
        y3 = h.color_apply(three, rows, ALL, params_out=p3)
        assert _same_bits(y1[0], y3[2]) and torch.equal(p1[0], p3[2]) and float(p1[0, 3]) != 0
        t1 = h.color_apply(img, row, ALL, transpose=True)
        t3 = h.color_apply(three, rows, ALL, transpose=True)
        assert _same_bits(t1[0], t3[2])
        p3b = torch.zeros(3, 4, device=dev)
        assert _same_bits(h.color_apply(three, rows, ALL, params_out=p3b), y3) and torch.equal(p3b, p3)
        assert _same_bits(h.color_apply(three, rows, ALL, transpose=True), t3)


# ------------------------------------------------------------------ 3. general inputs
@pytest.mark.parametrize("shape", [(2, 28, 1), (2, 64, 3), (1, 128, 3), (1, 5, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("build", list(BUILDS))
def test_general_inputs_mean_within_highams_bound_forward_bitwise_transpose_within_its_bound(build, shape):
    h = H()
    dtype = BUILDS[build]
    N, S, C = shape
    gen = torch.Generator().manual_seed(12)
    x0 = torch.tanh(torch.randn(N, S, S, C, generator=gen)).to(dtype)
    g0 = (torch.randn(N, S, S, C, generator=gen) * 1e-3).to(dtype)
    drawn = R.color_params(N, SEEDS[0], 3)
    n = S * S * C
    for color in SUBSETS:
        y, p = h.color_draw(x0.to(dev), SEEDS[0], 3, color)
        p = p.cpu()
        assert torch.equal(p[:, :3], drawn)
        if color.contrast:
            x64 = x0.double()
            dM = (p[:, 3].double() - x64.reshape(N, -1).mean(1)).abs()
            dM_ref = (R.color_mean(x0.float()).double() - x64.reshape(N, -1).mean(1)).abs()
            bound = _mean_bound(x64)
            print("Mx %s %s %s: kernel |dMx| %.3e, torch-fp32 oracle %.3e, bound %.3e" % (
                build, shape, color.describe(), float(dM.max()), float(dM_ref.max()), float(bound.min())))
            assert bool((dM <= bound).all()), (color, dM.tolist(), bound.tolist())
        else:
            assert not bool(p[:, 3].any())
        assert _same_bits(y, R.color_augment(x0, p, color).to(dev)), color  # bitwise at the recorded mean
        # the transpose against fp64
        tg = h.color_apply(g0.to(dev), drawn, color, transpose=True).cpu().double()
        g64 = g0.double()
        want = R.color_augment_transpose(g64, drawn, color)
        c = drawn[:, 2].double().reshape(N, 1, 1, 1) if color.contrast else torch.ones(N, 1, 1, 1, dtype=torch.float64)
        flat = g64.reshape(N, -1).abs()
        bound = (_ulp(want, dtype) / 2 + (1 - c).abs() * (n - 1) * 2.0 ** -24 * flat.mean(1).reshape(N, 1, 1, 1)
                 + 8 * 2.0 ** -24 * flat.max(1)[0].reshape(N, 1, 1, 1))
        err = (tg - want).abs()
        err_ref = (R.color_augment_transpose(g0, drawn, color).double() - want).abs()
        print("transpose %s %s %s: kernel max err %.3e (%.3f of its bound), torch-fp32 oracle %.3e" % (
            build, shape, color.describe(), float(err.max()), float((err / bound).max()), float(err_ref.max())))
        assert bool((err <= bound).all()), (color, float((err / bound).max()))


def test_non_finite_and_huge_params_complete():
    """The probe and the transpose take any floats: no index depends on them, nothing is written outside."""
    h = H()
    shape = (4, 28, 28, 3)
    x0 = _exact(4, 28, 3, 3).to(torch.bfloat16)
    xb, x = _slot(shape, torch.bfloat16)
    x.copy_(x0)
    inf, nan = float("inf"), float("nan")
    params = torch.tensor([[inf, -inf, nan], [3e38, -3e38, 3e38], [nan, nan, nan], [0.0, 1.0, 1.0]])
    for transpose in (False, True):
        yb, y = _slot(shape, torch.bfloat16)
        h.color_apply(x, params, ALL, transpose=transpose, out=y)
        torch.cuda.synchronize()
        assert _intact(yb) and _intact(xb) and _same_bits(x, x0)
        want = R.color_augment_transpose(x0, params, ALL) if transpose else R.color_augment(x0, params, ALL)
        assert _same_bits(y[3], want[3].to(dev))  # the finite row is served as ever
        assert not bool(torch.isfinite(y[:3].float()).all())


def test_bindings_reject_bad_calls_and_record_nothing():
    h = H()
    x = torch.zeros(2, 8, 8, 3, device=dev, dtype=torch.bfloat16)
    y = torch.zeros_like(x)
    p = torch.zeros(2, 4, device=dev, dtype=torch.float32)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    P_ = lambda t: t.data_ptr()  # noqa: E731
    prog = h.ext().Program()
    ok = (P_(x), P_(y), P_(p), 2, 8, 3, 7)
    bad = [(0,) + ok[1:], ok[:1] + (0,) + ok[2:], ok[:2] + (0,) + ok[3:], (P_(x), P_(x)) + ok[2:], ok[:6] + (0,),
           ok[:6] + (8,), ok[:4] + (0,) + ok[5:], ok[:4] + ((1 << 14) + 1,) + ok[5:], ok[:5] + (0, 7), ok[:5] + (5, 7),
           ok[:3] + (0,) + ok[4:]]
    for a in bad:
        with pytest.raises(RuntimeError, match="d_color"):
            prog.d_color("a", *a, 1, P_(step), 0)
        with pytest.raises(RuntimeError, match="d_color_bwd"):
            prog.d_color_bwd("b", *a, 0)
    assert prog.size() == 0
    with pytest.raises(TypeError):
        h.color_apply(x.double(), p, 7)
    with pytest.raises(TypeError):
        h.color_apply(x, p[:1], 7)
    with pytest.raises(TypeError):
        h.color_apply(x, p.int(), 7)
    with pytest.raises(TypeError):
        h.color_apply(x[:, :, :4], p, 7)
    with pytest.raises(TypeError):
        h.color_draw(x, 1, torch.zeros(1, device=dev), 7)
    with pytest.raises(ValueError, match="unknown policy"):
        h.color_apply(x, p, "hue")
    with pytest.raises(RuntimeError, match="policy"):
        h.color_apply(x, p, "")
    with pytest.raises(RuntimeError, match="buffer of its own"):
        h.color_apply(x, p, 7, out=x)
    assert not bool(y.any())


# ------------------------------------------------------------------ 4. the engine's buffers
def _check_colored(eng, d_in, k, t, tag):
    """color_params[:, :3] == the oracle's draws of (the piece's seed, step t), Mx inside its bound;
    d_colored == color_augment(d_in) bitwise at the recorded Mx."""
    want = R.color_params(2 * eng.B, eng._zseed(k), t)
    got = eng.color_params.cpu()
    assert torch.equal(got[:, :3], want), tag
    x = d_in.cpu()
    if eng.color.contrast:
        x64 = x.double()
        assert bool(((got[:, 3].double() - x64.reshape(x.shape[0], -1).mean(1)).abs() <= _mean_bound(x64)).all()), tag
    assert _same_bits(eng.d_colored, R.color_augment(x, got, eng.color).to(dev)), tag
    assert not _same_bits(eng.d_colored, d_in), tag
    return want


def _acc(prog, name):
    i = [j for j in range(prog.size()) if prog.name(j) == name]
    assert len(i) == 1, (name, i)
    return prog.op_info(i[0])[4]


@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 28, 1), ("fp16", 28, 1), ("fp32", 28, 1), ("bf16", 64, 3)])
def test_engine_colored_buffer_is_the_oracles_and_z_is_untouched(dtype, size, c_dim):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = TD._engine(cfg, 8, 1, dtype=dtype, seed=3, **COLOR)
    off = TD._engine(cfg, 8, 1, dtype=dtype, seed=3)
    assert eng.color == ALL and eng.d_colored.shape == eng.d_in.shape and eng.d_colored.dtype == eng.d_in.dtype
    assert eng.color_params.dtype == torch.float32 and tuple(eng.color_params.shape) == (16, 4)
    assert off.d_colored is None and off.color_params is None and off.img_grad_c is None
    assert eng.d_auged is None and eng.img_grad_t is None and eng._d_input() is eng.d_colored
    # the op list is today's but for d_color, d_color_bwd and the unfused image gradient + tanh backward
    want = off.op_names()
    f = [i for i, n in enumerate(want) if "dgrad_img+tanh_bwd" in n]
    if f:
        assert dtype != "fp32" and len(f) == 2
        want[f[0]:f[1] + 1] = [want[f[0]][:-len("+tanh_bwd")], "g_out.tanh_bwd"]
    names = eng.op_names()
    assert [n for n in names if n not in ("d_color", "d_color_bwd")] == want
    assert names.count("d_color") == 1 and names.count("d_color_bwd") == 1
    i = names.index("d_color_bwd")
    assert names[i - 1].endswith(".dgrad_img") and names[i + 1] == "g_out.tanh_bwd"
    seen = []
    for t in range(3):
        eng.train_step()
        off.train_step()
        torch.cuda.synchronize()
        seen.append(_check_colored(eng, eng.d_in, None, t, "step %d" % t))
        assert torch.equal(eng.z, off.z)  # z keeps stream 0: bitwise what it is without the switch
        if t == 0:  # (same weights so far: the clean input is the same too, and the step differs after it)
            assert torch.equal(eng.d_in, off.d_in) and eng.last_losses() != off.last_losses()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])  # a fresh draw per step


def test_sub_steps_draw_their_own_params():
    eng = TD._engine(small(), 8, 3, seed=6, **COLOR)
    assert eng.op_names().count("d_color") == 3 and eng.op_names().count("d_color_bwd") == 1
    assert all(eng.sub_op_names(k).count("d_color") == 1 and "d_color_bwd" not in eng.sub_op_names(k) for k in range(2))
    seen = []
    for t in range(2):
        for k, run in ((0, lambda: eng.train_d_step(0)), (1, lambda: eng.train_d_step(1)), (None, eng.train_full_step)):
            run()
            torch.cuda.synchronize()
            # (the sub-steps see the global step of the full step after them)
            seen.append(_check_colored(eng, eng.d_in if k is None else eng.d_ins[k], k, t, "step %d piece %s" % (t, k)))
        assert eng.global_step == t + 1
    for i in range(len(seen)):
        for j in range(i):
            assert not torch.equal(seen[i], seen[j]), (i, j)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_the_three_stages_land_in_order(dtype):
    """color, then translation / cutout of the colored copy, then the noise on that."""
    eng = TD._engine(small(), 8, 1, dtype=dtype, seed=3, **COLOR, **GEO, **NOISE)
    es = 4 if dtype == "fp32" else 2
    nb = eng.d_in.numel() * es
    step = (eng.step_counter.data_ptr(), 8, False)
    assert sorted(_acc(eng.progA, "d_color")) == sorted([(eng.d_in.data_ptr(), nb, False), step, (eng.d_colored.data_ptr(), nb, True),
                                                          (eng.color_params.data_ptr(), 256, True)])
    assert sorted(_acc(eng.progA, "d_aug")) == sorted([(eng.d_colored.data_ptr(), nb, False), step, (eng.d_auged.data_ptr(), nb, True),
                                                        (eng.aug_params.data_ptr(), 256, True)])
    assert sorted(_acc(eng.progA, "d_noise")) == sorted([(eng.d_auged.data_ptr(), nb, False), step, (eng.d_noisy.data_ptr(), nb, True)])
    names = eng.op_names()
    assert names.index("d_aug") == names.index("d_color") + 1 and names.index("d_noise") == names.index("d_aug") + 1
    assert eng._d_input() is eng.d_noisy and eng._d_input(noise=False) is eng.d_in
    eng.train_step()
    torch.cuda.synchronize()
    _check_colored(eng, eng.d_in, None, 0, "three stages")
    params = R.augment_params(16, 28, eng._zseed(None), 0)
    assert torch.equal(eng.aug_params.cpu().long(), params)
    assert _same_bits(eng.d_auged, R.augment(eng.d_colored.cpu(), params, eng.aug).to(dev))
    sig = eng.noise.sigma0
    diff = (eng.d_noisy.float() - eng.d_auged.float()).cpu()
    assert 0.5 * sig < float(diff.std()) < 2 * sig


# ------------------------------------------------------------------ 5. the g_loss chain, stage by stage
@pytest.mark.parametrize("dtype,size,c_dim,geo", [("bf16", 64, 3, True), ("fp16", 64, 3, False), ("bf16", 28, 1, False),
                                                  ("fp32", 28, 1, True)])
def test_the_g_loss_chain_stage_by_stage(dtype, size, c_dim, geo):
    """After one step: img_grad through the oracle's transposed gather is, bitwise, what d_color_bwd read
    (with translation / cutout on); d_color_bwd's output is the oracle's transpose of that within the
    kernel test's bound; img_g is the tanh backward of that buffer at the CLEAN fake (test_act_bwd_dbias's
    tolerance, as test_hip_d_augment.py takes it: 8e-3 x max |ref|); G's output bias gradient is the column
    sum of img_g (that test's bound)."""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=3, **COLOR, **(GEO if geo else {}))
    edt = BUILDS[dtype]
    nb = eng.img_grad.numel() * (4 if dtype == "fp32" else 2)
    src = eng.img_grad_t if geo else eng.img_grad
    acc = _acc(eng.progA, "g_out.tanh_bwd")
    assert (eng.img_grad_c.data_ptr(), nb, False) in acc and (eng.fake.data_ptr(), nb, False) in acc
    assert not any(a in (eng.img_grad.data_ptr(), src.data_ptr()) for a, _, _ in acc)
    assert sorted(_acc(eng.progA, "d_color_bwd")) == sorted([(src.data_ptr(), nb, False), (eng.img_grad_c.data_ptr(), nb, True),
                                                              (eng.color_params.data_ptr() + 16 * B, 16 * B, False)])
    names = eng.op_names()
    j = names.index("d_color_bwd")
    assert names[j + 1] == "g_out.tanh_bwd" and (names[j - 1] == "d_aug_bwd" and names[j - 2].endswith(".dgrad_img") if geo
                                                else names[j - 1].endswith(".dgrad_img"))
    eng.train_step()
    torch.cuda.synchronize()
    cp = eng.color_params.cpu()
    assert torch.equal(cp[:, :3], R.color_params(2 * B, eng._zseed(None), 0))
    ig = eng.img_grad.cpu()
    assert float(ig.float().abs().max()) > 0 and bool(torch.isfinite(ig.float()).all())
    if geo:
        params = R.augment_params(2 * B, size, eng._zseed(None), 0)
        assert torch.equal(eng.aug_params.cpu().long(), params)
        assert _same_bits(eng.img_grad_t, R.augment_transpose(ig, params[B:], eng.aug).to(dev))
    g64 = src.cpu().double()
    want = R.color_augment_transpose(g64, cp[B:], eng.color)
    n = size * size * c_dim
    flat = g64.reshape(B, -1).abs()
    c = cp[B:, 2].double().reshape(B, 1, 1, 1)
    bound = (_ulp(want, edt) / 2 + (1 - c).abs() * (n - 1) * 2.0 ** -24 * flat.mean(1).reshape(B, 1, 1, 1)
             + 8 * 2.0 ** -24 * flat.max(1)[0].reshape(B, 1, 1, 1))
    err = (eng.img_grad_c.cpu().double() - want).abs()
    print("d_color_bwd in the step (%s %dx%dx%d): max err %.3e, %.3f of its bound" % (dtype, size, size, c_dim, float(err.max()),
                                                                                   float((err / bound).max())))
    assert bool((err <= bound).all())
    assert not _same_bits(eng.img_grad_c, src)
    y = eng.fake.float().cpu()
    ref = (eng.img_grad_c.float().cpu() * (1 - y * y)).to(eng.edt).float()
    got = eng.img_g.float().cpu()
    e, scale = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-6
    print("tanh backward of the transposed gradient (%s %dx%dx%d): max err %.3e, scale %.3e" % (dtype, size, size, c_dim, e, scale))
    assert e <= 8e-3 * scale
    db = eng.grad_g[cfg.g_layers()[-1].name + "/biases"].double().cpu()
    cols = eng.img_g.double().cpu().reshape(-1, c_dim)
    assert float((db - cols.sum(0)).abs().max()) <= 1e-5 * (float(cols.abs().sum(0).max()) + 1)


# ------------------------------------------------------------------ 6. against ReferenceStep
class _WithColor:
    """ReferenceStep behind the two calls ``_check_piece`` makes, the oracle's draws (and noise) passed in."""

    def __init__(self, ref):
        self.ref, self.color, self.params, self.noise = ref, None, None, False

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, color=self.color, augment=self.params, noise=self.noise)

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z, color=self.color, augment=self.params, noise=self.noise)


def _color_piece(eng, ref, ref_model, cfg, real, dtype, sn, k, run, tag, rdev):
    ref.color = R.color_params(2 * eng.B, eng._zseed(k), eng.global_step)
    if eng.aug.active:
        ref.params = R.augment_params(2 * eng.B, cfg.output_size, eng._zseed(k), eng.global_step)
    if eng.noise.active:
        ref.noise = R.instance_noise(tuple(eng.d_in.shape), eng.noise, eng._zseed(k), eng.global_step).to(rdev)
    TD._check_piece(eng, ref, ref_model, cfg, real, dtype, sn, k is None, run, tag)
    assert torch.equal(eng.color_params[:, :3].cpu(), ref.color), tag
    if eng.aug.active:
        assert torch.equal(eng.aug_params.cpu().long(), ref.params), tag


@pytest.mark.parametrize("dtype,size,c_dim", [("fp32", 28, 1), ("bf16", 28, 1), ("fp16", 28, 1), ("bf16", 64, 3)])
def test_four_colored_steps_track_the_reference(dtype, size, c_dim, seed=3):
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **COLOR)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, **COLOR)
    ref = _WithColor(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    for s in range(4):
        _color_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)
    assert eng.global_step == 4


@pytest.mark.parametrize("dtype,size,c_dim", [("fp32", 28, 1), ("bf16", 64, 3)])
def test_four_colored_and_augmented_steps_track_the_reference(dtype, size, c_dim, seed=3):
    """Four steps after one warm-up step: with translation / cutout on, step 0 sits on the LeakyReLU kink
    over the zero-filled pixels (test_hip_d_augment.py documents and measures it)."""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **COLOR, **GEO)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, **COLOR, **GEO)
    ref = _WithColor(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    eng.train_step()
    for s in range(1, 5):
        _color_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)
    assert eng.global_step == 5


def test_colored_cycle_with_sub_steps_and_spectral_norm_tracks_the_reference(seed=4):
    cfg, B, dtype = DCGANConfig(output_size=28, c_dim=1, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, **COLOR)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2, **COLOR)
    ref = _WithColor(ref)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    _color_piece(eng, ref, ref_model, cfg, reals[0], dtype, True, 0, lambda: eng.train_d_step(0), "sub-step", rdev)
    _color_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, None, eng.train_full_step, "full", rdev)
    assert eng.global_step == 1


# ------------------------------------------------------------------ 7. graph == eager; 8. off == today
@pytest.mark.parametrize("dtype,d_steps,geo", [("bf16", 2, True), ("fp16", 1, False)])
def test_graph_replay_follows_the_live_counter(dtype, d_steps, geo):
    """A step baked in at capture time would repeat the first replay's draws."""
    kw = dict(dtype=dtype, seed=1, **COLOR, **(GEO if geo else {}))
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    prev = None
    for t in range(4):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
        assert _same_bits(e1.d_colored, e2.d_colored) and torch.equal(e1.color_params, e2.color_params)
        assert _same_bits(e1.img_grad_c, e2.img_grad_c)
        assert torch.equal(e2.color_params[:, :3].cpu(), R.color_params(16, e2._zseed(None), t))
        assert prev is None or not torch.equal(e2.color_params.cpu(), prev)
        prev = e2.color_params.cpu().clone()
    assert e2.graph_enabled and not e1.graph_enabled and e1.global_step == e2.global_step == 4


def test_the_switch_off_is_todays_engine():
    cfg = small()
    a = TD._engine(cfg, 8, 2, seed=2, d_color_augment="")
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    b = HipEngine(cfg, 8, dev, seed=2, graph=False, d_steps=2)  # built without the argument
    for k, x in enumerate(TD._reals(8, cfg, "bf16", 2)):
        b.set_batch(x.to(dev), k)
    assert not a.color.active and a.d_colored is None and b.d_colored is None and b.color_params is None
    assert a.op_names() == b.op_names() and not any("d_color" in n for n in a.op_names())
    assert a.kernel_count() == b.kernel_count() and a.sub_op_names(0) == b.sub_op_names(0)
    assert any(n.endswith("dgrad_img+tanh_bwd") for n in a.op_names())  # the fused kernel stays
    for _ in range(3):
        a.train_step()
        b.train_step()
    for x, y in zip(TD._snap(a), TD._snap(b)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 9. eval_losses
def test_eval_losses_stay_clean():
    cfg, B = small(), 8
    on = TD._engine(cfg, B, 1, seed=2, **COLOR, **NOISE)
    off = TD._engine(cfg, B, 1, seed=7)
    on.train_step()
    torch.cuda.synchronize()
    for name in ("g", "d"):
        getattr(off.model, name).flat.copy_(getattr(on.model, name).flat)
    off.after_state_load()
    real = TD._reals(B, cfg, "bf16", 3)[2]
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    before = (on.d_colored.clone(), on.color_params.clone(), on.d_noisy.clone())
    a, b = on.eval_losses(real, z), off.eval_losses(real, z)
    assert a == b and a["d_loss"] > 0
    assert _same_bits(on.d_colored, before[0]) and torch.equal(on.color_params, before[1]) and _same_bits(on.d_noisy, before[2])
    names = [on.progEval.name(i) for i in range(on.progEval.size())]
    assert "d_color" not in names and "d_noise" not in names
    assert names == [off.progEval.name(i) for i in range(off.progEval.size())]


# ------------------------------------------------------------------ 10. one-rank RCCL DDP
STEPS = 3


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, **COLOR, **GEO)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "pd": eng.opt_d.powers.cpu(), "pg": eng.opt_g.powers.cpu(),
            "losses": eng.losses.cpu(), "colored": eng.d_colored.cpu(), "params": eng.color_params.cpu(),
            "auged": eng.d_auged.cpu(), "img_grad_c": eng.img_grad_c.cpu()}


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
    assert eng.ddp and eng._schedule() == schedule and eng.color.active
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
def test_rccl_single_rank_ddp_matches_fused_with_the_color_policy(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert r["ops"].count("d_color") == 1 and r["ops"].count("d_color_bwd") == 1
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k


# ------------------------------------------------------------------ 11. resume through the trainer
def test_trainer_resume_is_exact(tmp_path, monkeypatch):
    """bf16: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more -- every saved tensor
    bitwise, and no key beyond the run's without the switch (the draws are a function of seed and step)."""
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
    AF = ["--d_color_augment=contrast,saturation,brightness"]

    def run(ck, steps, af=AF):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + af)
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
    assert "color augmentation of D's inputs: brightness,saturation,contrast" in text
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    text = run(tmp_path / "c", 4, af=[])  # without the switch: another model, under the same keys
    assert "color augmentation" not in text
    ic, sc = load(tmp_path / "c")
    assert list(sc) == list(sa) and any(not (sa[k] == sc[k]).all() for k in sa)
