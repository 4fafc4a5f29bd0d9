"""DiffAugment on D's inputs (--d_augment: translation, cutout), CPU side: the draws from the Philox
counter layout, the transform against a plain loop and against the published pad-and-gather code, its
autograd against the explicit transposed gather, validation and precedence at every entry point,
``ReferenceStep`` against hand-written autograd, the dry-run HIP schedules (hazards, where ``d_aug``
and ``d_aug_bwd`` sit, a planted race), and the CLI."""
import io
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
ENV = ("DCGAN_D_AUGMENT", "DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS",
       "DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP",
       "DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_DDP_SHARD", "DCGAN_DDP_SCHEDULE",
       "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM", "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS", "DCGAN_D_UPDATE")
SEED = 1000020  # HipEngine._zseed of z_seed = 1, rank 0
SEEDS = (SEED, 0xFEDCBA9876543210)
STEPS = (0, 1, 2 ** 32 + 3)
BOTH = R.DAugment(True, True)
POLICIES = (R.DAugment(True, False), R.DAugment(False, True), BOTH)


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


# ------------------------------------------------------------------ 1. the draws
def test_draws_by_hand_from_the_philox_block_of_each_sample():
    """Sample n: the block at counter (lo32(n), hi32(n), lo32(t), hi32(t) ^ 2) under the 64-bit seed."""
    for S in (28, 64, 7):
        s, k = (S + 4) // 8, (S + 1) // 2
        r = S + (1 - k % 2)
        assert s == int(S * 0.125 + 0.5) and k == int(S * 0.5 + 0.5)
        for seed in SEEDS:
            for t in STEPS:
                got = R.augment_params(5, S, seed, t)
                assert got.dtype == torch.int64 and tuple(got.shape) == (5, 4)
                for n in range(5):
                    ctr = np.array([n & 0xFFFFFFFF, n >> 32, t & 0xFFFFFFFF, ((t >> 32) ^ 2) & 0xFFFFFFFF], dtype=np.uint64)
                    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
                    w = [int(v) for v in R.philox4x32_10(ctr, key)]
                    want = [((w[0] * (2 * s + 1)) >> 32) - s, ((w[1] * (2 * s + 1)) >> 32) - s,
                            (w[2] * r) >> 32, (w[3] * r) >> 32]
                    assert got[n].tolist() == want
    assert R.AUG_STREAM == 2 and R.AUG_STREAM != R.NOISE_STREAM


def test_draws_stay_in_range_and_cover_every_shift():
    S, s, r = 28, 4, 29
    seen = set()
    rows = []
    for seed in SEEDS:
        for t in STEPS:
            p = R.augment_params(16, S, seed, t)
            rows.append(p)
            assert int(p[:, :2].min()) >= -s and int(p[:, :2].max()) <= s
            assert int(p[:, 2:].min()) >= 0 and int(p[:, 2:].max()) < r
            seen |= set(p[:, 0].tolist())
    assert seen == set(range(-s, s + 1))  # 96 samples: every ty in [-4, 4] occurs
    assert len({tuple(p.flatten().tolist()) for p in rows}) == len(rows)  # seed and step both decide
    assert torch.equal(R.augment_params(16, S, SEED, 1)[:7], R.augment_params(7, S, SEED, 1))
    p64 = R.augment_params(64, 64, SEED, 0)
    assert int(p64[:, :2].abs().max()) <= 8 and int(p64[:, 2:].max()) < 65  # k = 32 even: r = 65


# ------------------------------------------------------------------ 2. the transform
def _loop(x, params, aug):
    N, S, _, C = x.shape
    k = (S + 1) // 2
    y = torch.zeros_like(x)
    for n in range(N):
        ty, tx, oy, ox = (int(v) for v in params[n])
        if not aug.translation:
            ty = tx = 0
        for i in range(S):
            for j in range(S):
                if aug.cutout and oy - k // 2 <= i < oy - k // 2 + k and ox - k // 2 <= j < ox - k // 2 + k:
                    continue
                if 0 <= i + ty < S and 0 <= j + tx < S:
                    y[n, i, j] = x[n, i + ty, j + tx]
    return y


def _loop_transpose(g, params, aug):
    N, S, _, C = g.shape
    k = (S + 1) // 2
    gx = torch.zeros_like(g)
    for n in range(N):
        ty, tx, oy, ox = (int(v) for v in params[n])
        if not aug.translation:
            ty = tx = 0
        for p in range(S):
            for q in range(S):
                i, j = p - ty, q - tx
                if not (0 <= i < S and 0 <= j < S):
                    continue
                if aug.cutout and oy - k // 2 <= i < oy - k // 2 + k and ox - k // 2 <= j < ox - k // 2 + k:
                    continue
                gx[n, p, q] = g[n, i, j]
    return gx


def _published(x, params, aug):
    """rand_translation then rand_cutout of the DiffAugment paper's code, NCHW, with the draws given:
    translation pads by one pixel and gathers at clamp(i + t + 1, 0, S + 1); cutout builds a mask from
    the clamped grid oy - k // 2 + [0, k)."""
    import torch.nn.functional as Fn
    x = x.permute(0, 3, 1, 2)
    N, _, S, _ = x.shape
    ty, tx, oy, ox = (params[:, i].view(N, 1, 1) for i in range(4))
    if aug.translation:
        gb, gy, gx = torch.meshgrid(torch.arange(N), torch.arange(S), torch.arange(S), indexing="ij")
        gy = torch.clamp(gy + ty + 1, 0, S + 1)
        gx = torch.clamp(gx + tx + 1, 0, S + 1)
        xp = Fn.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
        x = xp.permute(0, 2, 3, 1).contiguous()[gb, gy, gx].permute(0, 3, 1, 2)
    if aug.cutout:
        k = int(S * 0.5 + 0.5)
        gb, gy, gx = torch.meshgrid(torch.arange(N), torch.arange(k), torch.arange(k), indexing="ij")
        gy = torch.clamp(gy + oy - k // 2, min=0, max=S - 1)
        gx = torch.clamp(gx + ox - k // 2, min=0, max=S - 1)
        mask = torch.ones(N, S, S, dtype=x.dtype)
        mask[gb, gy, gx] = 0
        x = x * mask.unsqueeze(1)
    return x.permute(0, 2, 3, 1)


def _ints(shape, seed):
    """Integer-valued fp64, nonzero: sums and products stay exact, and a zero in y is a zero of the transform."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(1, 9, shape, generator=g).double()
    return v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def _edge_params(S):
    s, k = (S + 4) // 8, (S + 1) // 2
    r = S + (1 - k % 2)
    return torch.tensor([[s, s, 0, 0], [-s, -s, r - 1, r - 1], [s, -s, 0, r - 1], [-s, s, r - 1, 0], [0, 0, k // 2, k // 2],
                         [0, 0, 0, 0]], dtype=torch.int64)


@pytest.mark.parametrize("S,C", [(6, 2), (7, 3)])
@pytest.mark.parametrize("aug", POLICIES, ids=lambda a: a.describe())
def test_augment_is_the_plain_loop(S, C, aug):
    for params in (R.augment_params(6, S, SEED, 3), _edge_params(S)):
        x = _ints((6, S, S, C), S)
        y = R.augment(x, params, aug)
        assert torch.equal(y, _loop(x, params, aug))
        assert not torch.signbit(y[y == 0]).any()  # every zero is +0
        xm = -x.abs()  # all negative: a product with a mask would leave -0 behind
        ym = R.augment(xm.float(), params, aug)
        assert torch.equal(ym.double(), _loop(xm, params, aug)) and not torch.signbit(ym[ym == 0]).any()
    if aug.cutout:
        assert (R.augment(x, _edge_params(S), aug) == 0).any()


@pytest.mark.parametrize("S", [28, 64])
@pytest.mark.parametrize("aug", POLICIES, ids=lambda a: a.describe())
def test_augment_is_the_published_pad_and_gather(S, aug):
    N = 12
    x = _ints((N, S, S, 3), S)
    for params in (R.augment_params(N, S, SEEDS[1], 5), torch.cat([_edge_params(S), _edge_params(S)])):
        assert torch.equal(R.augment(x, params, aug), _published(x, params, aug))
    off = R.DAugment()
    assert torch.equal(R.augment(x, params, off), x) and not off.active


@pytest.mark.parametrize("S,C", [(6, 2), (7, 3), (28, 1)])
@pytest.mark.parametrize("aug", POLICIES, ids=lambda a: a.describe())
def test_autograd_is_the_transposed_gather_and_the_adjoint_identity_is_exact(S, C, aug):
    N = 6
    for params in (R.augment_params(N, S, SEED, 2 ** 32 + 3), _edge_params(S)):
        x = _ints((N, S, S, C), 1).requires_grad_(True)
        g = _ints((N, S, S, C), 2)
        y = R.augment(x, params, aug)
        gx, = torch.autograd.grad(y, x, g)
        t = R.augment_transpose(g, params, aug)
        assert torch.equal(gx, t)
        if S < 28:
            assert torch.equal(t, _loop_transpose(g, params, aug))
        assert float((y.detach() * g).sum()) == float((x.detach() * t).sum())  # <T x, g> == <x, T^T g>
        assert not torch.signbit(t[t == 0]).any()


def test_augment_rejects_malformed_inputs():
    x = torch.zeros(2, 4, 4, 1)
    with pytest.raises(ValueError, match=r"\[N, S, S, C\]"):
        R.augment(torch.zeros(2, 4, 5, 1), torch.zeros(2, 4, dtype=torch.int64), BOTH)
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        R.augment(x, torch.zeros(3, 4, dtype=torch.int64), BOTH)


# ------------------------------------------------------------------ 3. validation, every entry point
GOOD = {"": R.DAugment(), "none": R.DAugment(), "translation": R.DAugment(True, False), "cutout": R.DAugment(False, True),
        "translation,cutout": BOTH, "cutout,translation": BOTH, " Cutout , TRANSLATION ": BOTH}
BAD = {"color": "color", "translation,colour": "colour", "cutout;translation": "cutout;translation",
       "none,cutout": "none", "translate": "translate"}


def test_check_d_augment_and_describe():
    for spec, want in GOOD.items():
        assert R.check_d_augment(spec) == want
    for spec, tok in BAD.items():
        with pytest.raises(ValueError, match="unknown policy %r" % tok):
            R.check_d_augment(spec)
    with pytest.raises(ValueError, match="d_augment"):
        R.check_d_augment(3)
    assert R.check_d_augment(BOTH) == BOTH and R.check_d_augment(None) == R.DAugment()
    assert [a.describe() for a in POLICIES] == ["translation", "cutout", "translation,cutout"]
    assert R.DAugment().describe() == "off" and [a.mask for a in POLICIES] == [1, 2, 3] and R.DAugment().mask == 0
    assert all(a.active for a in POLICIES)


def test_every_entry_point_validates_and_an_explicit_argument_wins(monkeypatch):
    makers = (lambda **kw: ReferenceEngine(small(), 4, CPU, **kw), lambda **kw: _hip(**kw),
              lambda **kw: ReferenceStep(DCGAN(small(), seed=1), **{"d_augment": "", **kw}))
    for mk in makers:
        with pytest.raises(ValueError, match="unknown policy 'color'"):
            mk(d_augment="translation,color")
        assert mk(d_augment="cutout").aug == R.DAugment(False, True)
    with pytest.raises(SystemExit):
        F.parse_flags(["--d_augment=color"])
    assert F.parse_flags([]).d_augment == "" and F.parse_flags(["--d_augment=cutout,translation"]).d_augment == "cutout,translation"
    monkeypatch.setenv("DCGAN_D_AUGMENT", "translation")
    assert R.resolve_d_augment() == R.DAugment(True, False)
    for mk in makers[:2]:
        assert mk().aug == R.DAugment(True, False)
        assert mk(d_augment="cutout").aug == R.DAugment(False, True)
        assert not mk(d_augment="").aug.active and not mk(d_augment="none").aug.active
    monkeypatch.setenv("DCGAN_D_AUGMENT", "flip")
    with pytest.raises(ValueError, match="unknown policy 'flip'"):
        R.resolve_d_augment()
    monkeypatch.delenv("DCGAN_D_AUGMENT")
    e = _hip()
    assert not e.aug.active and e.d_auged is None and e.aug_params is None and e.img_grad_t is None


def test_the_bindings_reject_bad_calls_and_record_nothing():
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    x, y, p, st = 0x1000, 0x9000, 0x20000, 0x30000
    ok = dict(N=2, S=8, C=3, policy=3)

    def fwd(**kw):
        a = dict(ok, x=x, y=y, params=p, seed=5, step=st)
        a.update(kw)
        return prog.d_augment("a", a["x"], a["y"], a["params"], a["N"], a["S"], a["C"], a["policy"], a["seed"], a["step"], 0)

    def bwd(**kw):
        a = dict(ok, x=x, y=y, params=p)
        a.update(kw)
        return prog.d_augment_bwd("b", a["x"], a["y"], a["params"], a["N"], a["S"], a["C"], a["policy"], 0)
    for call in (fwd, bwd):
        for kw, msg in ((dict(x=0), "non-null"), (dict(y=0), "non-null"), (dict(params=0), "non-null"),
                        (dict(y=x), "buffer of its own"), (dict(policy=0), "policy"), (dict(policy=4), "policy"),
                        (dict(policy=-1), "policy"), (dict(S=0), "S must"), (dict(S=(1 << 14) + 1), "S must"),
                        (dict(C=0), "C must"), (dict(C=5), "C must"), (dict(N=0), "N must")):
            with pytest.raises(RuntimeError, match=msg):
                call(**kw)
    assert prog.size() == 0
    nb = 2 * 8 * 8 * 3 * 2
    fwd()
    fwd(step=0)
    bwd()
    assert sorted(prog.op_info(0)[4]) == sorted([(x, nb, False), (st, 8, False), (y, nb, True), (p, 32, True)])
    assert sorted(prog.op_info(1)[4]) == sorted([(x, nb, False), (p, 32, False), (y, nb, True)])  # the probe entry
    assert sorted(prog.op_info(2)[4]) == sorted([(x, nb, False), (p, 32, False), (y, nb, True)])
    assert H.ext().Program(2, True).d_augment("a", x, y, p, 2, 8, 3, 1, 5, st, 0) == 0


# ------------------------------------------------------------------ 4. ReferenceStep
def _hand_step(model, real, z, params, aug, full):
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in model.g.tensors.items()}
    Pd = {k: v.detach().clone().requires_grad_(True) for k, v in model.d.tensors.items()}
    fake = model.generator(z, train=True, P=Pg, update_ema=False)
    both = _loop(torch.cat([real, fake], 0), params, aug)  # (pixel by pixel, not the oracle under test)
    _, logits = model.discriminator(both, groups=2, slots=(0, 1), train=True, P=Pd, update_ema=False)
    B = real.shape[0]
    _, _, g_loss, d_loss = R.gan_losses(logits[:B], logits[B:], "bce", 0.0)
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


def test_reference_step_with_augmentation_is_autograd_on_the_augmented_input():
    cfg, B = small(), 4
    st = ReferenceStep(DCGAN(cfg, seed=3), d_augment="translation,cutout", noise_seed=SEED, d_steps=2)
    assert st.aug == BOTH
    st.global_step = 2
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    shape = (2 * B, 28, 28, 1)
    params = R.augment_params(2 * B, 28, SEED, 2)
    assert torch.equal(st.draw_augment(shape), params)
    d_loss, g_loss, gd, gg = _hand_step(st.model, real, z, params, BOTH, True)
    out, fd, fg = st.compute_grads(real, z, update_ema=False)
    assert float(out["d_loss"].detach()) == float(d_loss.detach()) and float(out["g_loss"].detach()) == float(g_loss.detach())
    assert torch.equal(fd, _flat_grads(st.model.d, gd)) and torch.equal(fg, _flat_grads(st.model.g, gg))
    out2, fd2, fg2 = st.compute_grads(real, z, update_ema=False, augment=params)  # passed in: the same step
    assert torch.equal(fd2, fd) and torch.equal(fg2, fg)
    clean = st.forward_losses(real, z, update_ema=False, augment=False)
    assert float(clean["d_loss"].detach()) != float(out["d_loss"].detach())
    plain = ReferenceStep(DCGAN(cfg, seed=3)).forward_losses(real, z, update_ema=False)
    assert float(clean["d_loss"].detach()) == float(plain["d_loss"].detach())
    # the D sub-step: the sub-step's seed, the global step of the full step after it
    params_k = R.augment_params(2 * B, 28, R.substep_seed(SEED, 0), 2)
    assert not torch.equal(params_k, params)
    d_loss_k, _, _, _ = _hand_step(st.model, real, z, params_k, BOTH, False)
    got = st.d_step(real, z)
    assert got["d_loss"] == float(d_loss_k.detach()) and st.global_step == 2 and st._sub_k == 1
    st.step(real, z)
    assert st.global_step == 3 and st._sub_k == 0


def test_augmentation_comes_before_the_noise_and_off_is_bitwise_todays_step():
    cfg, B = small(), 4
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    kw = dict(instance_noise=0.3, instance_noise_end=0.3, noise_seed=SEED)
    st = ReferenceStep(DCGAN(cfg, seed=3), d_augment="translation", **kw)
    seen = {}
    orig = st.model.discriminator

    def spy(x, **k):
        seen["x"] = x.detach().clone()
        return orig(x, **k)
    st.model.discriminator = spy
    out = st.forward_losses(real, z, update_ema=False)
    both = torch.cat([real, out["fake"].detach()], 0)
    want = R.augment(both, R.augment_params(2 * B, 28, SEED, 0), st.aug) + st.draw_noise(both.shape)
    assert torch.equal(seen["x"], want)
    a, b = ReferenceStep(DCGAN(cfg, seed=3), d_augment=""), ReferenceStep(DCGAN(cfg, seed=3))
    for _ in range(2):
        assert a.step(real, z) == b.step(real, z)
    assert torch.equal(a.model.d.flat, b.model.d.flat) and torch.equal(a.model.g.flat, b.model.g.flat)


def test_reference_engine_uses_the_hip_engines_seed_and_clean_eval_losses():
    cfg, B = small(), 4
    e = ReferenceEngine(cfg, B, CPU, seed=3, rank=2, z_seed=1, d_augment="cutout")
    h = _hip(seed=3, rank=2, z_seed=1, world=4, d_augment="cutout")
    assert e.step_impl.noise_seed == h._zseed(None) == 1 * 1000003 + 17 + 7919 * 2
    plain = ReferenceEngine(cfg, B, CPU, seed=3)
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    assert e.eval_losses(real, z) == plain.eval_losses(real, z)  # sample-time losses stay clean
    e.set_synthetic_batch(real)
    plain.set_synthetic_batch(real)
    e.train_step()
    plain.train_step()
    assert e.last_losses() != plain.last_losses()


# ------------------------------------------------------------------ 5. schedules (dry-run HIP engines)
ON = dict(d_augment="translation,cutout")
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


def _check_aug_ops(eng, d_steps):
    """One d_aug per forward, on the main stream, right behind the op writing the fake half; one d_aug_bwd
    per full step between the image-gradient op and G's tanh backward. What each reads and writes."""
    ex = _record(eng)
    es = 4 if eng.f32 else 2
    nbytes = eng.d_in.numel() * es
    B2 = 2 * eng.B
    idx = [i for i, op in enumerate(ex.ops) if _name(op) == "d_aug"]
    assert len(idx) == d_steps
    for k, i in enumerate(idx):
        op, d_in = ex.ops[i], eng.d_ins[k]
        assert op.stream == "main"
        assert sorted(op.acc) == sorted([(d_in.data_ptr(), nbytes, False), (eng.step_counter.data_ptr(), 8, False),
                                         (eng.d_auged.data_ptr(), nbytes, True), (eng.aug_params.data_ptr(), B2 * 16, True)])
        assert "g_h" in _name(ex.ops[i - 1]) and any(w for _, _, w in ex.ops[i - 1].acc)
        nxt = ex.ops[i + 1]
        if eng.noise.active:  # the noise lands on the augmented copy
            assert _name(nxt) == "d_noise"
            assert sorted(nxt.acc) == sorted([(eng.d_auged.data_ptr(), nbytes, False), (eng.step_counter.data_ptr(), 8, False),
                                              (eng.d_noisy.data_ptr(), nbytes, True)])
            nxt = ex.ops[i + 2]
        assert _name(nxt).startswith(("d0.", "d_h0")), _name(nxt)
        assert any(a == eng._d_input().data_ptr() and not w for a, _, w in nxt.acc)
    # D's layer 0 (forward and weight gradient) reads the perturbed copy only; the clean input has one reader
    # per forward besides G's tanh backward
    lo, hi = eng.d_auged.data_ptr(), eng.d_auged.data_ptr() + nbytes
    readers = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
    if eng.noise.active:
        assert readers == {"d_noise"}
    else:
        assert readers and all(r.startswith(("d0.", "d_h0")) for r in readers), readers
    for d_in in eng.d_ins:
        lo, hi = d_in.data_ptr(), d_in.data_ptr() + nbytes
        clean = {_name(o) for o in ex.ops if any(not w and lo <= a < hi for a, _, w in o.acc)}
        assert "d_aug" in clean and "d_noise" not in clean and not any(r.startswith(("d0.", "d_h0")) for r in clean), clean
    # the backward
    names = [_name(o) for o in ex.ops]
    assert names.count("d_aug_bwd") == 1 and names.count("g_out.tanh_bwd") == 1
    assert not any("dgrad_img+tanh_bwd" in n for n in names)
    j = names.index("d_aug_bwd")
    op = ex.ops[j]
    half = nbytes // 2
    assert sorted(op.acc) == sorted([(eng.img_grad.data_ptr(), half, False), (eng.aug_params.data_ptr() + eng.B * 16, eng.B * 16, False),
                                     (eng.img_grad_t.data_ptr(), half, True)])
    assert names[j - 1].endswith(".dgrad_img") and any(a == eng.img_grad.data_ptr() and w for a, _, w in ex.ops[j - 1].acc)
    assert ex.ops[j - 1].stream == op.stream
    t = names.index("g_out.tanh_bwd")
    assert t > j and ex.ops[t].stream == op.stream
    acc = ex.ops[t].acc
    assert any(a == eng.img_grad_t.data_ptr() and not w for a, _, w in acc)
    assert any(a == eng.fake.data_ptr() and not w for a, _, w in acc)  # tanh' at the clean fake
    assert not any(a == eng.img_grad.data_ptr() for a, _, _ in acc)


@pytest.mark.parametrize("noise", [False, True], ids=["aug", "aug+noise"])
@pytest.mark.parametrize("world,schedule,wire,d_steps", CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in CASES])
def test_schedules_are_hazard_free_with_the_augment_ops(world, schedule, wire, d_steps, noise):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **ON, **(NOISE if noise else {}))
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_aug_ops(eng, d_steps)
    assert eng.op_names().count("d_aug") == d_steps and eng.op_names().count("d_aug_bwd") == 1
    assert all(eng.sub_op_names(k).count("d_aug") == 1 and "d_aug_bwd" not in eng.sub_op_names(k)
               for k in range(d_steps - 1))


@pytest.mark.parametrize("dtype,size,c_dim", [("fp16", 28, 1), ("fp32", 28, 1), ("fp32", 64, 3), ("bf16", 64, 3),
                                              ("bf16", 128, 3)])
@pytest.mark.parametrize("d_steps", [1, 3])
def test_other_dtypes_and_sizes_are_hazard_free_with_the_augment_ops(dtype, size, c_dim, d_steps):
    for world in (1, 2):
        for extra in ({}, NOISE):
            eng = _hip(DCGANConfig(output_size=size, c_dim=c_dim), dtype=dtype, world=world, d_steps=d_steps, **ON, **extra)
            hz, _ = SC.check_engine(eng)
            assert hz == [], "\n".join(map(str, hz[:10]))
            _check_aug_ops(eng, d_steps)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free_with_the_augment_ops(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    for extra in ({}, NOISE):
        eng = _hip(world=world, **ON, **extra)
        assert eng._sharded()
        hz, n = SC.check_engine(eng)
        assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
        _check_aug_ops(eng, 1)


def test_checker_finds_d_aug_bwd_moved_ahead_of_the_image_gradient():
    """d_aug_bwd issued on another stream before the op that writes img_grad, with nothing ordering the
    two: a race on img_grad (and on what tanh_bwd reads). Only the accesses to the two image-gradient
    buffers are kept, so the new op alone decides."""
    eng = _hip(**ON)
    assert SC.check_engine(eng)[0] == []
    ex = _record(eng, steps=2)
    names = [_name(o) for o in ex.ops]
    j = names.index("d_aug_bwd")
    op = ex.ops.pop(j)
    op.stream = "planted"  # (a stream nothing waits for)
    op.vc = {"planted": 1}
    ex.ops.insert(j - 1, op)
    bufs = [(b.data_ptr(), b.data_ptr() + b.numel() * 2) for b in (eng.img_grad, eng.img_grad_t)]
    for o in ex.ops:
        o.acc = [a for a in o.acc if any(lo <= a[0] < hi for lo, hi in bufs)]
    hz = SC.find_hazards(ex.ops)
    assert hz and all("d_aug_bwd" in h.a + h.b for h in hz), "\n".join(map(str, hz))
    assert any("dgrad_img" in h.a + h.b for h in hz) and any("tanh_bwd" in h.a + h.b for h in hz)


def test_with_the_switch_off_the_recorded_ops_are_todays():
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16"),
               dict(dtype="fp32"), NOISE):
        off, bare = _hip(d_augment="", **kw), _hip(**kw)
        assert off.d_auged is None and off.aug_params is None
        assert off.op_names() == bare.op_names() and not any("d_aug" in n for n in bare.op_names())
        assert off.kernel_count() == bare.kernel_count()
        a, b = _record(off), _record(bare)
        assert [(_name(x), x.stream, len(x.acc)) for x in a.ops] == [(_name(x), x.stream, len(x.acc)) for x in b.ops]
        on = _hip(**ON, **kw)
        names = on.op_names()
        if bare._img_dact():  # the fused image gradient + tanh backward (+ its bias-gradient sum) gives way to
            # the unfused image gradient, the transposed gather and G's tanh backward + bias gradient
            want = bare.op_names()
            f = [i for i, n in enumerate(want) if "dgrad_img+tanh_bwd" in n]
            assert f == [f[0], f[0] + 1] and want[f[1]] == want[f[0]] + ".dbias"
            want[f[0]:f[1] + 1] = [want[f[0]][:-len("+tanh_bwd")], "d_aug_bwd", "g_out.tanh_bwd"]
            assert [n for n in names if n != "d_aug"] == want
            assert on.kernel_count() == bare.kernel_count() + on.d_steps + 1
        else:
            assert [n for n in names if n not in ("d_aug", "d_aug_bwd")] == bare.op_names()
            assert on.kernel_count() == bare.kernel_count() + on.d_steps + 1


# ------------------------------------------------------------------ 6. trainer / CLI
def test_cli_runs_with_augmentation_on_the_reference_engine(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=2", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=4", "--sample_every=0", "--nosummaries", "--epoch=0", "--d_augment=cutout,translation",
            "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "differentiable augmentation of D's inputs: translation,cutout" in p.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--d_augment=color"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "unknown policy 'color'" in bad.stdout


def test_trainer_prints_nothing_with_the_switch_off(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32", "--max_steps=1",
                        "--epoch=0", "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
                        "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0 and "augmentation" not in out.getvalue()
