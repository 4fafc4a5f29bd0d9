"""GPU tests of DiffAugment on D's inputs (translation, cutout): the kernel's draws against the oracle,
the forward and the transposed gather bitwise against ``ops.reference.augment`` and its autograd (bf16 /
fp16 / fp32 builds, canary-padded buffers, the 16-byte and the element store path), the engine's
augmented buffer and recorded draws (full step and D sub-steps), the g_loss chain stage by stage, steps
against ``ReferenceStep`` with the oracle's draws passed in (the comparison and tolerances of
test_hip_d_steps.py, unchanged), hipGraph replay, the switch off, clean sample-time losses, one-rank
RCCL DDP and resume through the trainer.

The transform moves bits and does no arithmetic, so every kernel comparison is an equality of bit
patterns. Shapes: [3,6,6,2] (rows shorter than one 16-byte access), [16,28,28,1] (56-byte rows: element
stores), [4,64,64,3] (16-byte stores, several workgroups per image), and views one element off 16-byte
alignment (element stores on the same data). Engines at 28x28x1 and 64x64x3, B = 8."""
import io
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
ENV = TD.ENV + ("DCGAN_D_AUGMENT", "DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS",
                "DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP")
SEEDS = [1000020, 0xFEDCBA9876543210]
STEPS_T = [0, 1, (1 << 32) + 3]
SHAPES = [(3, 6, 6, 2), (16, 28, 28, 1), (4, 64, 64, 3)]
BOTH = R.DAugment(True, True)
POLICIES = (R.DAugment(True, False), R.DAugment(False, True), BOTH)
AUG = dict(d_augment="translation,cutout")
NOISE = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=4)
FILL = 7.0


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
    """A [N,S,S,C] view `off` elements past a 16-byte boundary, PAD canaries on both sides: (buffer, view)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * PAD + off,), FILL, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off:PAD + off + n].view(shape)


def _intact(buf, off=0):
    return bool((buf[:PAD + off] == FILL).all()) and bool((buf[-PAD:] == FILL).all())


def _data(shape, dtype, seed):
    """Normals with signed zeros and an infinity planted: the kernel copies bits, whatever they say."""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    f = x.flatten()
    f[::37] = -0.0
    f[5] = float("inf")
    return x.to(dtype)


def _edge_params(S, N):
    """(+-s, +-s) shifts, a box at offsets 0 and r - 1, a zero shift: N rows, every case within any 6."""
    s, k = (S + 4) // 8, (S + 1) // 2
    r = S + (1 - k % 2)
    rows = torch.tensor([[s, s, 0, 0], [-s, -s, r - 1, r - 1], [s, -s, 0, r - 1], [-s, s, r - 1, 0], [0, 0, k // 2, k // 2],
                         [0, 0, 0, 0]], dtype=torch.int64)
    return [rows[(torch.arange(N) + o) % 6] for o in (0, 3)]


# ------------------------------------------------------------------ 1. the draws
def test_draw_probe_equals_the_oracle():
    h = H()
    for S in (28, 64):
        for seed in SEEDS:
            for t in STEPS_T:
                got = h.augment_params(16, S, seed, t)
                assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), R.augment_params(16, S, seed, t))
    a = h.augment_params(16, 28, SEEDS[0], torch.tensor([1], dtype=torch.int64, device=dev))  # a device counter
    assert torch.equal(a.cpu().long(), R.augment_params(16, 28, SEEDS[0], 1))
    assert not torch.equal(a, h.augment_params(16, 28, SEEDS[0] + 1, 1))


# ------------------------------------------------------------------ 2. the forward kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("build", list(BUILDS))
def test_forward_kernel_is_bitwise_the_oracle(build, shape):
    h = H()
    dtype = BUILDS[build]
    N, S = shape[0], shape[1]
    x0 = _data(shape, dtype, 7)
    seed, t = SEEDS[1], STEPS_T[2]
    drawn = R.augment_params(N, S, seed, t)
    for off in (0, 1):  # 16-byte aligned; one element off: element stores, the same bits
        xb, x = _slot(shape, dtype, off)
        x.copy_(x0)
        for aug in POLICIES:
            # draws from the kernel, recorded next to the output
            yb, y = _slot(shape, dtype, off)
            pb = torch.full((4 * N + 2 * PAD,), -3, dtype=torch.int32, device=dev)
            p = pb[PAD:PAD + 4 * N].view(N, 4)
            out, pout = h.augment_draw(x, seed, t, aug, out=y, params_out=p)
            assert out.data_ptr() == y.data_ptr() and pout.data_ptr() == p.data_ptr()
            assert torch.equal(p.cpu().long(), drawn) and bool((pb[:PAD] == -3).all()) and bool((pb[-PAD:] == -3).all())
            assert _same_bits(y, R.augment(x0, drawn, aug)), (off, aug)
            assert _intact(yb, off)
            # hand-made params through the probe entry
            for params in _edge_params(S, N):
                yb, y = _slot(shape, dtype, off)
                h.augment_apply(x, params, aug, out=y)
                assert _same_bits(y, R.augment(x0, params, aug)), (off, aug, params.tolist())
                assert _intact(yb, off)
            assert _same_bits(h.augment_apply(x, drawn.to(dev), aug.describe()), R.augment(x0, drawn, aug))  # a fresh output
        assert _same_bits(x, x0) and _intact(xb, off)  # x is only read
    if shape[1] > 6:  # the policies differ, and the augmented image is not the input
        ys = [h.augment_apply(x, drawn, a) for a in POLICIES]
        assert not _same_bits(ys[0], ys[1]) and not _same_bits(ys[0], ys[2]) and not _same_bits(ys[2], x)


def test_far_out_params_are_safe():
    """Rows far outside the drawn ranges (the probe takes any integers): an empty image or an untouched
    one, never an access outside the buffers."""
    h = H()
    shape = (4, 28, 28, 1)
    x0 = _data(shape, torch.bfloat16, 3)
    xb, x = _slot(shape, torch.bfloat16)
    x.copy_(x0)
    big = 2 ** 31 - 1
    params = torch.tensor([[big, -big, 0, 0], [0, 0, big, -big - 1], [28, 0, -big, big], [-28, 27, 500, 500]])
    yb, y = _slot(shape, torch.bfloat16)
    h.augment_apply(x, params, BOTH, out=y)
    assert _same_bits(y, R.augment(x0, params, BOTH)) and _intact(yb) and _intact(xb)
    assert _same_bits(y[1], x0[1]) and not bool(y[0].any()) and not bool(y[2].any())
    gb, g = _slot(shape, torch.bfloat16)
    h.augment_apply(x, params, BOTH, transpose=True, out=g)
    assert _same_bits(g, R.augment_transpose(x0, params, BOTH)) and _intact(gb)


# ------------------------------------------------------------------ 3. the backward kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("build", list(BUILDS))
def test_backward_kernel_is_bitwise_the_oracles_autograd(build, shape):
    h = H()
    dtype = BUILDS[build]
    N, S = shape[0], shape[1]
    g0 = torch.randn(shape, generator=torch.Generator().manual_seed(9)).to(dtype)
    xi = torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(10)).to(dtype)  # integer-valued
    gi = torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(11)).to(dtype)
    cases = [R.augment_params(N, S, SEEDS[0], 1)] + _edge_params(S, N)
    for off in (0, 1):
        gb, g = _slot(shape, dtype, off)
        g.copy_(g0)
        for aug in POLICIES:
            for params in cases:
                x64 = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
                want, = torch.autograd.grad(R.augment(x64, params, aug), x64, g0.double())  # (copies: exact in any dtype)
                tb, tg = _slot(shape, dtype, off)
                h.augment_apply(g, params, aug, transpose=True, out=tg)
                assert _same_bits(tg, want.to(dtype)), (off, aug, params.tolist())
                assert _same_bits(tg, R.augment_transpose(g0, params, aug))
                assert _intact(tb, off)
        assert _same_bits(g, g0) and _intact(gb, off)
    # <T x, g> == <x, T^T g>, exactly, on integer-valued inputs through both kernels
    for aug in POLICIES:
        for params in cases:
            y = h.augment_apply(xi.to(dev), params, aug).cpu().double()
            tg = h.augment_apply(gi.to(dev), params, aug, transpose=True).cpu().double()
            assert float((y * gi.double()).sum()) == float((xi.double() * tg).sum())


# ------------------------------------------------------------------ 4. the engine's buffers
def _check_auged(eng, d_in, k, t, tag):
    """aug_params == the oracle's draws of (the piece's seed, step t); d_auged == augment(d_in) bitwise."""
    S = eng.cfg.output_size
    params = R.augment_params(2 * eng.B, S, eng._zseed(k), t)
    assert torch.equal(eng.aug_params.cpu().long(), params), tag
    assert _same_bits(eng.d_auged, R.augment(d_in.cpu(), params, eng.aug)), tag
    assert not _same_bits(eng.d_auged, d_in), tag
    return params


def _acc(prog, name):
    i = [j for j in range(prog.size()) if prog.name(j) == name]
    assert len(i) == 1, (name, i)
    return prog.op_info(i[0])[4]


@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 28, 1), ("fp16", 28, 1), ("fp32", 28, 1), ("bf16", 64, 3),
                                              ("fp32", 64, 3)])
def test_engine_augmented_buffer_is_the_oracles_and_z_is_untouched(dtype, size, c_dim):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = TD._engine(cfg, 8, 1, dtype=dtype, seed=3, **AUG)
    off = TD._engine(cfg, 8, 1, dtype=dtype, seed=3)
    assert eng.aug == BOTH and eng.d_auged.shape == eng.d_in.shape and eng.d_auged.dtype == eng.d_in.dtype
    assert eng.aug_params.dtype == torch.int32 and tuple(eng.aug_params.shape) == (16, 4)
    assert off.d_auged is None and off.aug_params is None and off.img_grad_t is None
    # the op list is today's but for d_aug, d_aug_bwd and the unfused image gradient + tanh backward
    want = off.op_names()
    f = [i for i, n in enumerate(want) if "dgrad_img+tanh_bwd" in n]
    if f:
        assert dtype != "fp32" and len(f) == 2
        want[f[0]:f[1] + 1] = [want[f[0]][:-len("+tanh_bwd")], "g_out.tanh_bwd"]
    names = eng.op_names()
    assert [n for n in names if n not in ("d_aug", "d_aug_bwd")] == want
    assert names.count("d_aug") == 1 and names.count("d_aug_bwd") == 1
    i = names.index("d_aug_bwd")
    assert names[i - 1].endswith(".dgrad_img") and names[i + 1] == "g_out.tanh_bwd"
    seen = []
    for t in range(3):
        eng.train_step()
        off.train_step()
        torch.cuda.synchronize()
        seen.append(_check_auged(eng, eng.d_in, None, t, "step %d" % t))
        assert torch.equal(eng.z, off.z)  # z keeps stream 0: bitwise what it is without the switch
        if t == 0:  # (same weights so far: the clean input is the same too, and the step differs after it)
            assert torch.equal(eng.d_in, off.d_in) and eng.last_losses() != off.last_losses()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])  # a fresh draw per step


def test_sub_steps_draw_their_own_augmentation():
    eng = TD._engine(small(), 8, 3, seed=6, **AUG)
    assert eng.op_names().count("d_aug") == 3 and eng.op_names().count("d_aug_bwd") == 1
    assert all(eng.sub_op_names(k).count("d_aug") == 1 and "d_aug_bwd" not in eng.sub_op_names(k) for k in range(2))
    seen = []
    for t in range(2):
        for k, run in ((0, lambda: eng.train_d_step(0)), (1, lambda: eng.train_d_step(1)), (None, eng.train_full_step)):
            run()
            torch.cuda.synchronize()
            # (the sub-steps see the global step of the full step after them)
            seen.append(_check_auged(eng, eng.d_in if k is None else eng.d_ins[k], k, t, "step %d piece %s" % (t, k)))
        assert eng.global_step == t + 1
    for i in range(len(seen)):
        for j in range(i):
            assert not torch.equal(seen[i], seen[j]), (i, j)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_with_noise_on_the_noise_lands_on_the_augmented_copy(dtype):
    eng = TD._engine(small(), 8, 1, dtype=dtype, seed=3, **AUG, **NOISE)
    es = 4 if dtype == "fp32" else 2
    nb = eng.d_in.numel() * es
    assert sorted(_acc(eng.progA, "d_noise")) == sorted([(eng.d_auged.data_ptr(), nb, False), (eng.step_counter.data_ptr(), 8, False),
                                                          (eng.d_noisy.data_ptr(), nb, True)])
    assert sorted(_acc(eng.progA, "d_aug")) == sorted([(eng.d_in.data_ptr(), nb, False), (eng.step_counter.data_ptr(), 8, False),
                                                        (eng.d_auged.data_ptr(), nb, True), (eng.aug_params.data_ptr(), 256, True)])
    names = eng.op_names()
    assert names.index("d_noise") == names.index("d_aug") + 1
    eng.train_step()
    torch.cuda.synchronize()
    params = _check_auged(eng, eng.d_in, None, 0, "with noise")
    # d_noisy = augmented + sigma * eps: away from it by the noise, and the cut-out box is no longer zero
    sig = eng.noise.sigma0
    diff = (eng.d_noisy.float() - eng.d_auged.float()).cpu()
    assert 0.5 * sig < float(diff.std()) < 2 * sig
    hole = (R.augment(torch.ones(eng.d_in.shape), params, eng.aug) == 0)
    assert bool(hole.any()) and float(eng.d_noisy.float().cpu()[hole].std()) > 0.5 * sig


# ------------------------------------------------------------------ 5. the g_loss chain, stage by stage
@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 64, 3), ("fp16", 64, 3), ("bf16", 28, 1), ("fp32", 28, 1)])
def test_the_g_loss_chain_stage_by_stage(dtype, size, c_dim):
    """After one step: img_grad through the oracle's transposed gather is, bitwise, the buffer G's tanh
    backward read; img_g is the tanh backward of that buffer at the CLEAN fake (test_act_bwd_dbias's
    tolerance: one 16-bit ulp of the largest value, 8e-3 x max |ref|); G's output bias gradient is the
    column sum of img_g (that test's bound)."""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=3, **AUG)
    nb = eng.img_grad.numel() * (4 if dtype == "fp32" else 2)
    acc = _acc(eng.progA, "g_out.tanh_bwd")
    assert (eng.img_grad_t.data_ptr(), nb, False) in acc and (eng.fake.data_ptr(), nb, False) in acc
    assert not any(a == eng.img_grad.data_ptr() for a, _, _ in acc)
    assert sorted(_acc(eng.progA, "d_aug_bwd")) == sorted([(eng.img_grad.data_ptr(), nb, False), (eng.img_grad_t.data_ptr(), nb, True),
                                                            (eng.aug_params.data_ptr() + 16 * B, 16 * B, False)])
    eng.train_step()
    torch.cuda.synchronize()
    params = R.augment_params(2 * B, size, eng._zseed(None), 0)
    assert torch.equal(eng.aug_params.cpu().long(), params)
    ig = eng.img_grad.cpu()
    assert float(ig.float().abs().max()) > 0 and bool(torch.isfinite(ig.float()).all())
    want_t = R.augment_transpose(ig, params[B:], eng.aug)
    assert _same_bits(eng.img_grad_t, want_t)
    assert not _same_bits(eng.img_grad_t, eng.img_grad)
    y = eng.fake.float().cpu()
    ref = (want_t.float() * (1 - y * y)).to(eng.edt).float()
    got = eng.img_g.float().cpu()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-6
    print("tanh backward of the transposed gradient (%s %dx%dx%d): max err %.3e, scale %.3e" % (dtype, size, size, c_dim, err, scale))
    assert err <= 8e-3 * scale
    db = eng.grad_g[cfg.g_layers()[-1].name + "/biases"].double().cpu()
    cols = eng.img_g.double().cpu().reshape(-1, c_dim)
    assert float((db - cols.sum(0)).abs().max()) <= 1e-5 * (float(cols.abs().sum(0).max()) + 1)


# ------------------------------------------------------------------ 6. against ReferenceStep
class _WithAug:
    """ReferenceStep behind the two calls ``_check_piece`` makes, the oracle's draws (and noise) passed in."""

    def __init__(self, ref):
        self.ref, self.params, self.noise = ref, None, False

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, augment=self.params, noise=self.noise)

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z, augment=self.params, noise=self.noise)


def _aug_piece(eng, ref, ref_model, cfg, real, dtype, sn, k, run, tag, rdev):
    ref.params = R.augment_params(2 * eng.B, cfg.output_size, eng._zseed(k), eng.global_step)
    if eng.noise.active:
        ref.noise = R.instance_noise(tuple(eng.d_in.shape), eng.noise, eng._zseed(k), eng.global_step).to(rdev)
    TD._check_piece(eng, ref, ref_model, cfg, real, dtype, sn, k is None, run, tag)
    assert torch.equal(eng.aug_params.cpu().long(), ref.params), tag


def test_from_zero_biases_the_step_differs_from_autograd_only_in_the_derivative_at_exact_zeros(seed=3):
    """Why the comparisons below start after one warm-up step. D's layer 0 has no BN, so over the
    zero-filled pixels its pre-activation is its bias exactly, and a fresh model's biases are 0: the
    LeakyReLU sits exactly on its kink there. The reference's maximum(x, 0.2 x) has derivative 0.6 at
    x == 0 under autograd (the tie is split), the kernels take 0.2 (the mask is y > 0); TensorFlow's
    maximum gives 1. All are subgradients. Only layer 0's bias gradient sees it (the inputs there are
    0, so the weight gradient does not): measured on an MI355X, fp32, its relative error is 0.396 against
    plain autograd and below the 1e-3 bound of ``_check_piece`` against the reference with the engine's
    derivative at those zeros (``_engine_masks``, as ``_check_piece`` itself uses at kinks); every
    other gradient is inside the bound either way. One Adam step moves every bias off 0."""
    cfg, B, dtype = small(), 8, "fp32"
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **AUG)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, **AUG)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    TD._sync_ref(ref_model, eng, False)
    eng.train_full_step()
    torch.cuda.synchronize()
    params = R.augment_params(2 * B, 28, eng._zseed(None), 0)
    z = eng.z.to(rdev)
    ins = []
    with SNT._recording(ins):
        plain = ref.compute_grads(real, z, update_ema=False, augment=params)
    d0 = ins[len(cfg.g_layers())]  # layer 0 of D: the first LeakyReLU after G's ReLUs
    assert tuple(d0.shape[:1]) == (2 * B,) and int((d0 == 0).sum()) > 1000
    with SNT._engine_masks(eng, cfg):
        masked = ref.compute_grads(real, z, update_ema=False, augment=params)
    dead = {L_.name + "/biases" for L_ in cfg.d_layers() if L_.bn} | {L_.name + "/biases" for L_ in cfg.g_layers() if L_.bn}

    def errs(gd, gg):
        gdref, ggref = ref_model.d.like(), ref_model.g.like()
        gdref.flat.copy_(gd)
        ggref.flat.copy_(gg)
        e = {n: TD.rel(eng.grad_d[n], gdref[n]) for n in ref_model.d.names() if n not in dead}
        e.update({n: TD.rel(eng.grad_g[n], ggref[n]) for n in ref_model.g.names() if n not in dead and n != "g_h0_lin/bias"})
        return e
    e_plain, e_masked = errs(plain[1], plain[2]), errs(masked[1], masked[2])
    print("step 0 from zero biases, fp32: d_h0_conv/biases rel error %.3e against autograd, %.3e with the engine's "
          "derivative at zeros; largest other %.3e" % (e_plain["d_h0_conv/biases"], e_masked["d_h0_conv/biases"],
                                                      max(v for k, v in e_masked.items() if k != "d_h0_conv/biases")))
    assert {k for k, v in e_masked.items() if v > 1e-3} == set()
    assert {k for k, v in e_plain.items() if v > 1e-3} <= {"d_h0_conv/biases"}


@pytest.mark.parametrize("dtype,size,c_dim", [("fp32", 28, 1), ("bf16", 28, 1), ("fp16", 28, 1), ("bf16", 64, 3)])
def test_four_augmented_steps_track_the_reference(dtype, size, c_dim, seed=3):
    """Four steps after one warm-up step (the test above says why), each against ReferenceStep."""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **AUG)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, **AUG)
    ref = _WithAug(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    eng.train_step()
    for s in range(1, 5):
        _aug_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)
    assert eng.global_step == 5


def test_augmented_cycle_with_sub_steps_and_spectral_norm_tracks_the_reference(seed=4):
    cfg, B, dtype = DCGANConfig(output_size=28, c_dim=1, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, **AUG)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2, **AUG)
    ref = _WithAug(ref)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    eng.train_step()  # (one warm-up cycle: biases off 0, see the test above)
    _aug_piece(eng, ref, ref_model, cfg, reals[0], dtype, True, 0, lambda: eng.train_d_step(0), "sub-step", rdev)
    _aug_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, None, eng.train_full_step, "full", rdev)
    assert eng.global_step == 2


def test_augmented_steps_with_instance_noise_track_the_reference(seed=5):
    cfg, B, dtype = small(), 8, "bf16"
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **AUG, **NOISE)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, **AUG, **NOISE)
    ref = _WithAug(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    for s in range(2):
        _aug_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)


# ------------------------------------------------------------------ 7. graph == eager; 8. off == today
@pytest.mark.parametrize("dtype,d_steps", [("bf16", 2), ("fp16", 1)])
def test_graph_replay_follows_the_live_counter(dtype, d_steps):
    """A step baked in at capture time would repeat the first replay's draws."""
    kw = dict(dtype=dtype, seed=1, **AUG)
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    prev = None
    for t in range(4):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
        assert _same_bits(e1.d_auged, e2.d_auged) and torch.equal(e1.aug_params, e2.aug_params)
        assert _same_bits(e1.img_grad_t, e2.img_grad_t)
        assert torch.equal(e2.aug_params.cpu().long(), R.augment_params(16, 28, e2._zseed(None), t))
        assert prev is None or not torch.equal(e2.aug_params.cpu(), prev)
        prev = e2.aug_params.cpu().clone()
    assert e2.graph_enabled and not e1.graph_enabled and e1.global_step == e2.global_step == 4


def test_the_switch_off_is_todays_engine():
    cfg = small()
    a = TD._engine(cfg, 8, 2, seed=2, d_augment="")
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    b = HipEngine(cfg, 8, dev, seed=2, graph=False, d_steps=2)  # built without the argument
    for k, x in enumerate(TD._reals(8, cfg, "bf16", 2)):
        b.set_batch(x.to(dev), k)
    assert not a.aug.active and a.d_auged is None and b.d_auged is None and b.aug_params is None
    assert a.op_names() == b.op_names() and not any("d_aug" in n for n in a.op_names())
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
    on = TD._engine(cfg, B, 1, seed=2, **AUG, **NOISE)
    off = TD._engine(cfg, B, 1, seed=7)
    on.train_step()
    torch.cuda.synchronize()
    for name in ("g", "d"):
        getattr(off.model, name).flat.copy_(getattr(on.model, name).flat)
    off.after_state_load()
    real = TD._reals(B, cfg, "bf16", 3)[2]
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    before = (on.d_auged.clone(), on.aug_params.clone(), on.d_noisy.clone())
    a, b = on.eval_losses(real, z), off.eval_losses(real, z)
    assert a == b and a["d_loss"] > 0
    assert _same_bits(on.d_auged, before[0]) and torch.equal(on.aug_params, before[1]) and _same_bits(on.d_noisy, before[2])
    names = [on.progEval.name(i) for i in range(on.progEval.size())]
    assert "d_aug" not in names and "d_noise" not in names
    assert names == [off.progEval.name(i) for i in range(off.progEval.size())]


# ------------------------------------------------------------------ 10. one-rank RCCL DDP
STEPS = 3


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, **AUG)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "pd": eng.opt_d.powers.cpu(), "pg": eng.opt_g.powers.cpu(),
            "losses": eng.losses.cpu(), "auged": eng.d_auged.cpu(), "params": eng.aug_params.cpu(),
            "img_grad_t": eng.img_grad_t.cpu()}


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
    assert eng.ddp and eng._schedule() == schedule and eng.aug.active
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
def test_rccl_single_rank_ddp_matches_fused_with_augmentation(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert r["ops"].count("d_aug") == 1 and r["ops"].count("d_aug_bwd") == 1
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
    AF = ["--d_augment=translation,cutout"]

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
    assert "differentiable augmentation of D's inputs: translation,cutout" in text
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    text = run(tmp_path / "c", 4, af=[])  # without the switch: another model, under the same keys
    assert "augmentation" not in text
    ic, sc = load(tmp_path / "c")
    assert list(sc) == list(sa) and any(not (sa[k] == sc[k]).all() for k in sa)


# ------------------------------------------------------------------ 12. the bindings' rejections
def test_bindings_reject_bad_calls_and_record_nothing():
    h = H()
    x = torch.zeros(2, 8, 8, 3, device=dev, dtype=torch.bfloat16)
    y = torch.zeros_like(x)
    p = torch.zeros(2, 4, device=dev, dtype=torch.int32)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    P_ = lambda t: t.data_ptr()  # noqa: E731
    prog = h.ext().Program()
    ok = (P_(x), P_(y), P_(p), 2, 8, 3, 3)
    bad = [(0,) + ok[1:], ok[:1] + (0,) + ok[2:], ok[:2] + (0,) + ok[3:], (P_(x), P_(x)) + ok[2:], ok[:6] + (0,),
           ok[:6] + (4,), ok[:4] + (0,) + ok[5:], ok[:5] + (0, 3), ok[:5] + (5, 3), ok[:3] + (0,) + ok[4:]]
    for a in bad:
        with pytest.raises(RuntimeError, match="d_augment"):
            prog.d_augment("a", *a, 1, P_(step), 0)
        with pytest.raises(RuntimeError, match="d_augment_bwd"):
            prog.d_augment_bwd("b", *a, 0)
    assert prog.size() == 0
    with pytest.raises(TypeError):
        h.augment_apply(x.double(), p, 3)
    with pytest.raises(TypeError):
        h.augment_apply(x, p[:1], 3)
    with pytest.raises(TypeError):
        h.augment_apply(x, p.float(), 3)
    with pytest.raises(TypeError):
        h.augment_apply(x[:, :, :4], p, 3)
    with pytest.raises(TypeError):
        h.augment_draw(x, 1, torch.zeros(1, device=dev), 3)
    with pytest.raises(ValueError, match="unknown policy"):
        h.augment_apply(x, p, "flip")
    with pytest.raises(RuntimeError, match="policy"):
        h.augment_apply(x, p, "")
    with pytest.raises(RuntimeError, match="buffer of its own"):
        h.augment_apply(x, p, 3, out=x)
    assert not bool(y.any())
