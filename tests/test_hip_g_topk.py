"""GPU tests of the top-k generator updates (``g_topk`` < 1): the selection kernel (misc.hip
g_topk_kernel) and its k(t) probe against the oracle of ops/reference.py, the engine's recorded
selection on its own logits, whole steps against ``ReferenceStep`` with the engine's mask passed in
(bf16 / fp16 / fp32, bce / lsgan / hinge), D sub-steps, the other switches composed, hipGraph replay on
the live counter, one-rank RCCL DDP, checkpoint resume through the trainer, and that the defaults change
nothing.

Bounds. The selection, the threshold, k, the scale B / k and the seeds are bitwise the oracle's (the
scale: one correctly rounded fp32 divide -- it equalled numpy's float32(B) / float32(k) in every case,
largest difference seen 0, so no ulp is allowed). g_loss_topk: per objective, the device's largest
error against the fp64 oracle over all the kernel cases with a finite loss, |got - want| / max(1,
|want|), is at most 4 x that of the fp32 oracle on the same inputs; where the fp64 loss is not finite
(a selected +-inf or NaN) the device's is the same infinity or NaN.

The step comparison is ``_check_piece`` of tests/test_hip_d_steps.py with its tolerances, unchanged; a
sample the reference itself would have selected differently must lie within the comparison's loss
tolerance (relative to max(1, |threshold|)) of the reference's threshold logit."""
import io
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_hip_d_spectral_norm as SNT
import test_hip_d_steps as TD
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
PAD = SNT.PAD
_padded, _canaries_intact = SNT._padded, SNT._canaries_intact
ENV = TD.ENV + ("DCGAN_G_TOPK", "DCGAN_G_TOPK_STEPS", "DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END",
                "DCGAN_INSTANCE_NOISE_STEPS", "DCGAN_D_AUGMENT", "DCGAN_D_COLOR_AUGMENT", "DCGAN_LR_DECAY")
TOPK = dict(g_topk=0.5, g_topk_steps=4)
BS = [1, 2, 5, 256, 257, 1000]
KINDS = ("bce", "lsgan", "hinge")
INPUTS = ("normal", "equal", "dups", "zeros", "special", "up", "down")


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


def _ks(B):
    return sorted({min(B, max(1, k)) for k in (1, 2, B // 2, B - 1, B)})


def _logits(kind, B):
    g = torch.Generator().manual_seed(1000 * INPUTS.index(kind) + B)
    if kind == "normal":
        return 4 * torch.randn(B, generator=g)
    if kind == "equal":
        return torch.full((B,), 0.75)
    if kind == "dups":
        return torch.tensor([-1.5, 0.25, 2.0])[torch.randint(0, 3, (B,), generator=g)]
    if kind == "zeros":
        return torch.where(torch.rand(B, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    if kind == "special":
        x = 4 * torch.randn(B, generator=g)
        for i, v in zip(torch.randperm(B, generator=g)[:3].tolist(), (float("inf"), float("-inf"), float("nan"))):
            x[i] = v
        return x
    ramp = torch.arange(B, dtype=torch.float32) * 0.01 - 0.005 * B
    return ramp if kind == "up" else ramp.flip(0)


def _loss_err(got, want):
    return abs(float(got) - float(want)) / max(1.0, abs(float(want)))


def _same_nonfinite(got, want):
    got, want = float(got), float(want)
    return (got != got) if want != want else got == want


# ------------------------------------------------------------------ 1. the kernel
@pytest.fixture(scope="module")
def cases():
    """Per (input, B): the fp32 logits and an all-sample seed (computed once, shared, never modified)."""
    out = {}
    for kind in INPUTS:
        for B in BS:
            x = _logits(kind, B)
            dl_g = torch.randn(B, generator=torch.Generator().manual_seed(B)) / B
            out[kind, B] = (x, dl_g)
    return out


@pytest.mark.parametrize("obj", KINDS)
def test_kernel_matches_the_oracle(obj, cases):
    """Every (input, B, k): sel, threshold, k, scale and the seeds bitwise; the loss within 4 x the fp32
    oracle's error, aggregated over the cases of this objective.
    Measured on an MI355X (largest |got - fp64| / max(1, |fp64|), device / fp32 oracle): bce 1.04e-7 /
    1.81e-7, lsgan 1.06e-7 / 1.18e-7, hinge 1.18e-7 / 1.13e-7; the scale never differed from numpy's divide."""
    h = H()
    worst_dev = worst_ref = worst_scale = 0.0
    nonfinite = 0
    for (kind, B), (x, dl_g) in cases.items():
        xd, gd = x.to(dev), dl_g.to(dev)
        for k in _ks(B):
            bufs = [_padded(torch.zeros(B)), _padded(torch.zeros(B, dtype=torch.int32), fill=7),
                    _padded(torch.zeros(4))]
            out = tuple(v for _, v in bufs)
            h.g_topk(xd, gd, k, obj, out=out)
            torch.cuda.synchronize()
            tag = (kind, B, k)
            assert all(_canaries_intact(b, fill=7) for b, _ in bufs), tag
            dl_g_k, sel, info = (v.cpu() for v in out)
            want_sel = R.topk_select(x, k)
            assert int(want_sel.sum()) == k and torch.equal(sel, want_sel.to(torch.int32)), tag
            assert float(info[3]) == float(k), tag
            thr = R.topk_threshold(x, k)
            assert torch.equal(info[1:2].view(torch.int32), thr.reshape(1).view(torch.int32)), tag
            scale = np.float32(B) / np.float32(k)
            worst_scale = max(worst_scale, abs(float(info[2]) - float(scale)))
            assert float(info[2]) == float(scale), tag
            want = R.topk_seed(dl_g, want_sel, B, k)
            assert torch.equal(dl_g_k.view(torch.int32), want.view(torch.int32)), tag  # (+0 on the others: sign bit too)
            assert torch.equal(dl_g_k[want_sel], dl_g[want_sel] * info[2]), tag
            assert not bool(dl_g_k[~want_sel].view(torch.int32).ne(0).any()), tag
            w64 = R.topk_g_loss(x.double(), want_sel, obj)
            w32 = R.topk_g_loss(x, want_sel, obj)
            if bool(torch.isfinite(w64)):
                worst_dev = max(worst_dev, _loss_err(info[0], w64))
                worst_ref = max(worst_ref, _loss_err(w32, w64))
            else:
                nonfinite += 1
                assert _same_nonfinite(info[0], w64), (tag, float(info[0]), float(w64))
    print("g_topk %s: largest loss error device %.3e, fp32 oracle %.3e (bound 4 x); scale: largest difference "
          "from numpy's divide %.1e; %d cases with a non-finite loss" % (obj, worst_dev, worst_ref, worst_scale,
                                                                         nonfinite))
    assert 0 < worst_ref < 1e-5 and worst_dev <= 4 * worst_ref and nonfinite > 0


def test_kernel_known_answers_and_loss_scale():
    """The issue's selection example; and with the fp16 loss-scale state given to the loss kernel, the
    top-k seeds carry it (dl_g does, the kernel multiplies dl_g)."""
    h = H()
    x = torch.tensor([0.5, -1, 0.5, 2, -0.0, +0.0])
    ones = torch.ones(6, device=dev)
    for k, want in ((2, {3, 0}), (3, {3, 0, 2}), (4, {3, 0, 2, 5})):
        _, sel, info = h.g_topk(x.to(dev), ones, k, "hinge")
        assert set(sel.nonzero().flatten().tolist()) == want and float(info[3]) == k
    B = 8
    logits = 2 * torch.randn(2 * B, generator=torch.Generator().manual_seed(3))
    ls = torch.tensor([1024.0, 0.0, 0.0], device=dev)
    for kind in KINDS:
        _, _, plain, _ = h.gan_loss(logits.to(dev), kind)
        _, _, scaled, _ = h.gan_loss(logits.to(dev), kind, ls=ls)
        a, sa, ia = h.g_topk(logits[B:].to(dev), plain, 4, kind)
        b, sb, ib = h.g_topk(logits[B:].to(dev), scaled, 4, kind)
        assert torch.equal(sa, sb) and torch.equal(ia, ib)  # the loss and the scale B / k do not carry it
        assert torch.equal(b, a * 1024.0) and float(b.abs().sum()) > 0
        # ... and the seed is the gradient of the mean over the selected k (fp64 autograd)
        xf = logits[B:].double().requires_grad_(True)
        R.topk_g_loss(xf, sa.cpu().bool(), kind).backward()
        assert torch.allclose(a.cpu().double(), xf.grad, rtol=1e-5, atol=1e-7), kind


def test_kernel_reads_k_from_the_schedule_and_the_counter():
    h = H()
    B, kmin, n = 128, R.topk_kmin(128, 0.5), 1000
    x = torch.randn(B, generator=torch.Generator().manual_seed(5)).to(dev)
    g = torch.ones(B, device=dev)
    for t, k in ((0, 128), (500, 96), (999, 65), (1000, 64), ((1 << 40) + 1, 64)):
        step = _step(t)
        _, sel, info = h.g_topk(x, g, (kmin, n), "bce", step)
        assert int(sel.sum()) == k == int(info[3]) and int(step) == t


def test_k_probe_equals_the_oracle_exactly():
    h = H()
    for B, nu, n in ((128, 0.5, 1000), (8, 0.5, 4), (4096, 1e-6, 1 << 24), (1000, 0.1, 7), (5, 1.0, 3), (1, 0.5, 9)):
        kmin = R.topk_kmin(B, nu)
        ts = sorted({0, 1, 2, n // 2, n - 1, n, n + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, 1 << 40, (1 << 62) + 1}
                    | {int(v) for v in torch.randint(0, n + 1, (64,), generator=torch.Generator().manual_seed(B))})
        buf, view = _padded(torch.zeros(len(ts), dtype=torch.int32), fill=7)
        got = h.topk_k(torch.tensor(ts, dtype=torch.int64, device=dev), B, kmin, n)
        view.copy_(got)
        assert _canaries_intact(buf, fill=7)
        want = [R.topk_k(t, B, kmin, n) for t in ts]
        assert got.tolist() == want and want[0] == B and want[-1] == kmin, (B, nu, n)


def test_binding_rejects_bad_arguments():
    h = H()
    B = 16
    x, g, o = (torch.zeros(B, device=dev) for _ in range(3))
    sel, info, step = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(4, device=dev), _step(0)
    P_ = lambda t: t.data_ptr()  # noqa: E731
    prog = h.ext().Program()
    good = [P_(x), P_(g), P_(o), P_(sel), P_(info), B, 8, 10, P_(step), 0]
    for i in (0, 1, 2, 3, 4, 8):  # a null pointer
        bad = list(good)
        bad[i] = 0
        with pytest.raises(RuntimeError, match="g_topk"):
            prog.g_topk("t", *bad)
    for i, v in ((2, P_(g)), (2, P_(x)), (3, P_(o)), (4, P_(o)), (2, P_(step))):  # aliasing
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError, match="of their own"):
            prog.g_topk("t", *bad)
    for Bb, kmin, steps, obj in ((0, 1, 10, 0), (4097, 8, 10, 0), (B, 0, 10, 0), (B, B + 1, 10, 0), (B, 8, 0, 0),
                                 (B, 8, (1 << 24) + 1, 0), (B, 8, 10, 3), (B, 8, 10, -1)):
        bad = list(good)
        bad[5], bad[6], bad[7], bad[9] = Bb, kmin, steps, obj
        with pytest.raises(RuntimeError, match="g_topk"):
            prog.g_topk("t", *bad)
        if obj == 0:
            with pytest.raises(RuntimeError, match="topk_k"):
                h.topk_k(torch.zeros(4, dtype=torch.int64, device=dev), Bb, kmin, steps)
    assert prog.size() == 0
    with pytest.raises(TypeError):
        h.g_topk(x, g.double(), 4)
    with pytest.raises(TypeError):
        h.g_topk(x, g, (8, 10))  # a schedule without the counter
    with pytest.raises(TypeError):
        h.g_topk(x, g, (8, 10), "bce", torch.zeros(1, device=dev))
    with pytest.raises(ValueError):
        h.g_topk(x, g, 4, "wgan")
    with pytest.raises(TypeError):
        h.topk_k(torch.zeros(4, device=dev), B, 8, 10)


# ------------------------------------------------------------------ 2. the engine's recorded selection
def _check_recorded(eng, t, tag):
    """sel / info / dl_g_k against the oracle on the engine's own logits and seed at global step t."""
    B = eng.B
    x, dl_g = eng.logits[B:].cpu(), eng.dl_g.cpu()
    k = R.topk_k(t, B, R.topk_kmin(B, eng.topk.nu), eng.topk.steps)
    sel = R.topk_select(x, k)
    assert torch.equal(eng.topk_sel.cpu(), sel.to(torch.int32)) and torch.equal(eng.topk_selection().cpu(), sel), tag
    info = eng.topk_info.cpu()
    assert float(info[3]) == k and float(info[2]) == float(np.float32(B) / np.float32(k)), tag
    assert float(info[1]) == float(R.topk_threshold(x, k)), tag
    assert torch.equal(eng.dl_g_k.cpu().view(torch.int32), R.topk_seed(dl_g, sel, B, k).view(torch.int32)), tag
    w64 = float(R.topk_g_loss(x.double(), sel, eng.gan_loss))
    assert abs(float(info[0]) - w64) <= 1e-5 * max(1.0, abs(w64)), tag
    kk, g, thr = eng.last_topk()
    assert (kk, g, thr) == (k, float(info[0]), float(info[1])), tag
    return k


@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 28, 1), ("fp16", 28, 1), ("fp32", 28, 1), ("bf16", 64, 3),
                                              ("fp32", 64, 3)])
def test_engine_selection_is_the_oracles_and_d_is_untouched(dtype, size, c_dim):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = TD._engine(cfg, 8, 1, dtype=dtype, seed=3, **TOPK)
    off = TD._engine(cfg, 8, 1, dtype=dtype, seed=3)
    assert off.dl_g_k is None and off.topk_sel is None and off.topk_info is None and off.last_topk() is None
    assert off.topk_selection() is None
    names = eng.op_names()
    assert [n for n in names if n != "g_topk"] == off.op_names() and names.count("g_topk") == 1
    assert names[eng._a_fwd] == "g_topk"  # the first op behind the forward
    ks = []
    for t in range(6):
        assert eng.global_step == t
        eng.train_step()
        torch.cuda.synchronize()
        ks.append(_check_recorded(eng, t, "step %d" % t))
        if t == 0:  # the same weights: D's side and the reported losses are bitwise those without top-k
            off.train_step()
            torch.cuda.synchronize()
            assert torch.equal(eng.losses, off.losses) and torch.equal(eng.grad_d.flat, off.grad_d.flat)
            assert torch.equal(eng.logits, off.logits) and torch.equal(eng.dl_g, off.dl_g)
            assert torch.equal(eng.dl_d, off.dl_d) and torch.equal(eng.grad_g.flat, off.grad_g.flat)  # k(0) = B
    assert ks == [8, 7, 6, 5, 4, 4]


# ------------------------------------------------------------------ 3. against ReferenceStep
class _WithMask:
    """ReferenceStep behind the two calls ``_check_piece`` makes, the engine's recorded mask passed as topk=."""

    def __init__(self, ref, eng, rdev):
        self.ref, self.eng, self.rdev = ref, eng, rdev

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, topk=self.eng.topk_selection().to(self.rdev))

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z)


def _topk_piece(eng, ref, ref_model, cfg, real, dtype, sn, tag, rdev):
    """One full step through ``_check_piece`` with the engine's mask, then the reference's own selection on
    the same (pre-step) weights and z: where the two differ, the reference logit is at its threshold."""
    t = eng.global_step
    sn0 = eng.model.d_sn.flat.to(rdev, copy=True) if sn else None  # (_check_piece ends with the power step)
    TD._check_piece(eng, _WithMask(ref, eng, rdev), ref_model, cfg, real, dtype, sn, True, eng.train_full_step, tag)
    _check_recorded(eng, t, tag)
    ref.global_step = t
    if sn:
        sn1 = ref_model.d_sn.flat.clone()
        ref_model.d_sn.flat.copy_(sn0)
    with torch.no_grad():
        out = ref.forward_losses(real, eng.z.to(rdev), update_ema=False)
    if sn:
        ref_model.d_sn.flat.copy_(sn1)
    own, x = out["topk_sel"].cpu(), out["logits_fake"].float().cpu()
    mask = eng.topk_selection().cpu()
    k = int(mask.sum())
    assert int(own.sum()) == k == ref.topk_k(eng.B), tag
    thr = float(R.topk_threshold(x, k))
    ltol = {"fp32": 1e-5, "bf16": 3e-2, "fp16": 2e-2}[dtype]  # (_check_piece's loss tolerances)
    diff = (own != mask).nonzero().flatten().tolist()
    print("%s %s: k %d, %d sample(s) selected differently by the reference, threshold %.4f" % (tag, dtype, k, len(diff), thr))
    for i in diff:
        assert abs(float(x[i]) - thr) <= ltol * max(1.0, abs(thr)), (tag, i, float(x[i]), thr)
    return k


@pytest.mark.parametrize("dtype,kind,size,c_dim", [(d, o, 28, 1) for d in ("fp32", "bf16", "fp16") for o in KINDS
                                                   if (d, o) not in (("fp32", "hinge"), ("fp16", "lsgan"))]
                         + [("bf16", "bce", 64, 3), ("fp16", "hinge", 64, 3), ("fp32", "lsgan", 64, 3)])
def test_four_topk_steps_track_the_reference(dtype, kind, size, c_dim, seed=3):
    """(No fp32 + hinge case: the fp32 comparison's kink bookkeeping counts the reference's relu calls, and the
    hinge loss itself calls relu twice; hinge runs in bf16 and fp16 here. No fp16 + lsgan case either: the
    least-squares seeds overflow fp16 at the initial loss scale within these four steps, with or without top-k
    (measured: step 1 is skipped and the scale halved in both), as
    tests/test_hip_gan_objectives.py describes, and a skipped step has no finite gradients to compare; lsgan
    runs in fp32 and bf16 here.)"""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, gan_loss=kind, **TOPK)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, gan_loss=kind, **TOPK)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    ks = [_topk_piece(eng, ref, ref_model, cfg, real, dtype, False, "step %d" % s, rdev) for s in range(4)]
    assert ks == [8, 7, 6, 5] and eng.global_step == 4


def test_cycle_with_sub_steps_spectral_norm_and_hinge(seed=4):
    """d_steps = 2, spectral norm, BN-free D, hinge: the sub-step records no g_topk and leaves the top-k
    buffers untouched; the full step behind it tracks the reference."""
    cfg, B, dtype = DCGANConfig(output_size=28, c_dim=1, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, gan_loss="hinge", **TOPK)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2, gan_loss="hinge", **TOPK)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    assert "g_topk" not in eng.sub_op_names(0) and eng.op_names().count("g_topk") == 1
    for t in range(2):
        before = [b.clone() for b in (eng.dl_g_k, eng.topk_sel, eng.topk_info)]
        TD._check_piece(eng, _WithMask(ref, eng, rdev), ref_model, cfg, reals[0], dtype, True, False,
                        lambda: eng.train_d_step(0), "step %d sub-step" % t)
        for a, b in zip(before, (eng.dl_g_k, eng.topk_sel, eng.topk_info)):
            assert torch.equal(a, b)
        assert _topk_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, "step %d full" % t, rdev) == 8 - t
    assert eng.global_step == 2


def test_composed_with_augmentations_and_noise():
    """translation, cutout + the color policy + instance noise + top-k: the selection is the oracle's on the
    engine's own logits, D's side at step 0 is bitwise that of the same engine without top-k."""
    kw = dict(seed=5, d_augment="translation,cutout", d_color_augment="brightness,saturation,contrast",
              instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=4)
    cfg = DCGANConfig(output_size=64, c_dim=3)
    eng = TD._engine(cfg, 8, 1, **kw, **TOPK)
    off = TD._engine(cfg, 8, 1, **kw)
    assert [n for n in eng.op_names() if n != "g_topk"] == off.op_names()
    for t in range(3):
        eng.train_step()
        torch.cuda.synchronize()
        _check_recorded(eng, t, "step %d" % t)
        if t == 0:
            off.train_step()
            torch.cuda.synchronize()
            assert torch.equal(eng.losses, off.losses) and torch.equal(eng.grad_d.flat, off.grad_d.flat)
    assert all(v == v and abs(v) < 1e4 for v in eng.last_losses().values())


# ------------------------------------------------------------------ 4. graph == eager, nu = 1, eval
@pytest.mark.parametrize("dtype,d_steps", [("bf16", 2), ("fp16", 1)])
def test_graph_replay_follows_the_live_counter(dtype, d_steps):
    """A k baked in at capture time would stay at the first replay's."""
    kw = dict(dtype=dtype, seed=1, **TOPK)
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    ks = []
    for t in range(6):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
        for a, b in ((e1.dl_g_k, e2.dl_g_k), (e1.topk_sel, e2.topk_sel), (e1.topk_info, e2.topk_info)):
            assert torch.equal(a, b)
        ks.append(_check_recorded(e2, t, "replay %d" % t))
    assert ks == [8, 7, 6, 5, 4, 4] and e2.graph_enabled and not e1.graph_enabled


def test_nu_one_is_the_engine_without_the_arguments():
    cfg = small()
    a = TD._engine(cfg, 8, 2, seed=2, g_topk=1.0, g_topk_steps=1000)
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    b = HipEngine(cfg, 8, dev, seed=2, graph=False, d_steps=2)  # built without the arguments
    for k, x in enumerate(TD._reals(8, cfg, "bf16", 2)):
        b.set_batch(x.to(dev), k)
    assert not a.topk.active and a.dl_g_k is None and b.dl_g_k is None
    assert a.op_names() == b.op_names() and "g_topk" not in a.op_names() and a.kernel_count() == b.kernel_count()
    assert a.sub_op_names(0) == b.sub_op_names(0)
    for _ in range(3):
        a.train_step()
        b.train_step()
    for x, y in zip(TD._snap(a), TD._snap(b)):
        assert torch.equal(x, y)


def test_eval_losses_stay_clean():
    cfg, B = small(), 8
    on = TD._engine(cfg, B, 1, seed=2, **TOPK)
    off = TD._engine(cfg, B, 1, seed=7)
    on.train_step()
    on.train_step()
    torch.cuda.synchronize()
    for name in ("g", "d"):
        getattr(off.model, name).flat.copy_(getattr(on.model, name).flat)
    off.after_state_load()
    real = TD._reals(B, cfg, "bf16", 3)[2]
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    before = [b.clone() for b in (on.dl_g_k, on.topk_sel, on.topk_info)]
    a, b = on.eval_losses(real, z), off.eval_losses(real, z)
    assert a == b and a["d_loss"] > 0
    for x, y in zip(before, (on.dl_g_k, on.topk_sel, on.topk_info)):
        assert torch.equal(x, y)  # no top-k op ran
    names = [on.progEval.name(i) for i in range(on.progEval.size())]
    assert "g_topk" not in names and names == [off.progEval.name(i) for i in range(off.progEval.size())]


def test_engine_rejects_a_batch_beyond_the_kernels_limit():
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    with pytest.raises(ValueError, match="g_topk"):
        HipEngine(small(), 4097, dev, g_topk=0.5, g_topk_steps=4, dry_run=True)
    with pytest.raises(ValueError, match="g_topk"):
        HipEngine(small(), 8, dev, g_topk=0.0, g_topk_steps=4, dry_run=True)


# ------------------------------------------------------------------ 5. one-rank RCCL DDP
STEPS = 3


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, **TOPK)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "pd": eng.opt_d.powers.cpu(), "pg": eng.opt_g.powers.cpu(),
            "losses": eng.losses.cpu(), "topk_info": eng.topk_info.cpu(), "topk_sel": eng.topk_sel.cpu(),
            "dl_g_k": eng.dl_g_k.cpu()}


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
    assert eng.ddp and eng._schedule() == schedule and eng.topk.active
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
def test_rccl_single_rank_ddp_matches_fused_with_topk(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert r["ops"].count("g_topk") == 1
    assert float(fused_run["topk_info"][3]) == 6.0  # k(2) of 8 -> 4 over 4 steps
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k


# ------------------------------------------------------------------ 6. resume through the trainer
def test_trainer_resume_is_exact_mid_anneal(tmp_path, monkeypatch):
    """bf16: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more, with the anneal of k
    under way at the restart -- every saved tensor bitwise, and no key beyond the run without top-k."""
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
    TF = ["--g_topk=0.5", "--g_topk_steps=6"]

    def run(ck, steps, tf=TF):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + tf)
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
    assert "top-k generator updates: k from B to ceil(0.5 B) over 6 steps" in text
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    run(tmp_path / "c", 4, tf=[])  # without top-k: another model, under the same keys
    ic, sc = load(tmp_path / "c")
    assert list(sc) == list(sa) and any(not (sa[k] == sc[k]).all() for k in sa)
