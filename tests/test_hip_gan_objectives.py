"""GPU tests of the selectable GAN objectives (bce | lsgan | hinge, one-sided label smoothing):
the stand-alone loss kernel against the fp32 oracle, the head GEMV's fused loss block against head
+ stand-alone loss, the default instance against today's calls, and whole steps of the fp32 /
bf16 / fp16 engines (eager, hipGraph, eval_losses, one-rank RCCL DDP)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
LOSS_SCALE = 32768.0  # HipEngine.INIT_LOSS_SCALE, the scale of the fp16 engine tests
KINDS = [("bce", 0.0), ("bce", 0.1), ("lsgan", 0.0), ("lsgan", 0.1), ("hinge", 0.0)]
NON_DEFAULT = [("hinge", 0.0), ("lsgan", 0.1)]


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def _prog(dt=0):
    return H().ext().Program(dt)


def _p(t):
    return 0 if t is None else t.data_ptr()


def bf(t):
    return t.to(torch.bfloat16).contiguous()


def close(out, ref, rel=1.5e-2, name=""):  # (tests/test_hip_kernels.py)
    out = out.float()
    ref = ref.float()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    print("%s: max err %.3e vs scale %.3e" % (name, err, scale))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).mul(scale).to(dev)


def oracle(logits, kind, s):
    """fp32 oracle on logits [2B]: (losses[4], dl_d[2B], dl_g[B]); the seeds are autograd's.
    bce at EXACTLY x = 0: the TF form max(x,0) - x t + log1p(exp(-|x|)) is smooth but written with
    two kinks that cancel there; autograd differentiates the pieces and returns 1 - t, not the
    derivative sigmoid(0) - t of the function. Those rows take the analytic seed (tests/
    test_gan_objectives.py pins autograd's value at that point)."""
    B = logits.numel() // 2
    lr = logits[:B].detach().clone().requires_grad_(True)
    lf = logits[B:].detach().clone().requires_grad_(True)
    dr, df, gl, dl = R.gan_losses(lr, lf, kind, s)
    gdr, gdf = torch.autograd.grad(dl, [lr, lf], retain_graph=True)
    (ggf,) = torch.autograd.grad(gl, [lf])
    if kind == "bce":
        gdr = torch.where(lr.detach() == 0, torch.full_like(gdr, (0.5 - (1.0 - s)) / B), gdr)
        gdf = torch.where(lf.detach() == 0, torch.full_like(gdf, 0.5 / B), gdf)
        ggf = torch.where(lf.detach() == 0, torch.full_like(ggf, -0.5 / B), ggf)
    return torch.stack([dr, df, gl, dl]).detach(), torch.cat([gdr, gdf]), ggf


# ------------------------------------------------------------------ 1. the stand-alone loss kernel
@pytest.mark.parametrize("B", [1, 37, 300])
@pytest.mark.parametrize("kind,s", KINDS)
def test_gan_loss_kernel_matches_oracle(kind, s, B):
    """B = 1: one row per half; 37: 2B < 256, a single pass; 300: 2B > 512, every thread strides
    twice and some a third time. The thresholds of every objective are planted in both halves."""
    h = H()
    logits = 4 * torch.randn(2 * B, generator=torch.Generator().manual_seed(32 + B))
    if B > 1:
        logits[:3] = torch.tensor([1.0, -1.0, 0.0])
        logits[B:B + 3] = torch.tensor([-1.0, 1.0, 0.0])
    logits = logits.to(dev)
    losses, seed_d, seed_g = oracle(logits, kind, s)
    for ls in (None, torch.tensor([LOSS_SCALE, 0.0, 0.0], device=dev)):
        out, dld, dlg, prob = h.gan_loss(logits, kind, s, ls)
        torch.cuda.synchronize()
        k = 1.0 if ls is None else LOSS_SCALE
        tag = "%s s=%g B=%d scale=%g " % (kind, s, B, k)
        close(out, losses, 1e-5, tag + "losses")  # the losses are not scaled
        close(dld, seed_d * k, 1e-5, tag + "dl_d")
        close(dlg, seed_g * k, 1e-5, tag + "dl_g")
        close(prob, torch.sigmoid(logits), 1e-5, tag + "prob")
        if ls is not None:
            assert ls.tolist() == [LOSS_SCALE, 0.0, 0.0]
    if kind == "hinge" and B > 1:  # the masks at the kinks, exactly: torch's subgradient is 0 there
        assert dld[0] == 0 and dld[1] != 0 and dld[2] != 0
        assert dld[B] == 0 and dld[B + 1] != 0 and dld[B + 2] != 0


# ------------------------------------------------------------------ 2. fused head == head + loss
def _bufs(B):
    return [torch.full((n,), float("nan"), device=dev) for n in (2 * B, 4, 2 * B, B, 2 * B)]


@pytest.mark.parametrize("B,K", [(3, 32), (64, 8192)])
@pytest.mark.parametrize("kind,s", NON_DEFAULT)
def test_head_gemv_fused_objective_matches_separate(kind, s, B, K):
    """gemv_head with the objective's losses in its last-arriving block == gemv_head + gan_loss,
    bitwise, over two replays (the arrival counter re-arms)."""
    h = H()
    obj = h.gan_loss_id(kind, s)
    x = bf(rnd(2 * B, K, seed=110))
    w = rnd(K, scale=3.0 / K ** 0.5, seed=111)  # logits of O(1): both hinge mask states occur
    hb = rnd(1, scale=0.25, seed=112)
    a, b = _bufs(B), _bufs(B)
    pr = _prog()
    pr.gemv_head("h", _p(x), _p(w), _p(hb), _p(a[0]), 2 * B, K, 0)
    pr.gan_loss("l", _p(a[0]), B, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), 0, 0, obj, s)
    pr.gemv_head("hl", _p(x), _p(w), _p(hb), _p(b[0]), 2 * B, K, 0, _p(b[1]), _p(b[2]), _p(b[3]), _p(b[4]), 0, obj, s)
    for _ in range(2):
        h.run(pr)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        for u in b:
            u.fill_(float("nan"))
    h.run(pr)
    torch.cuda.synchronize()
    losses, seed_d, seed_g = oracle(b[0], kind, s)  # ... and it is this objective that ran
    close(b[1], losses, 1e-5, "losses")
    close(b[2], seed_d, 1e-5, "dl_d")
    close(b[3], seed_g, 1e-5, "dl_g")
    if kind == "hinge" and B > 3:
        assert 0 < int((b[2][:B] == 0).sum()) < B and 0 < int((b[2][B:] == 0).sum()) < B


@pytest.mark.parametrize("B,K,C", [(2, 2048, 8), (64, 8192, 512)])
@pytest.mark.parametrize("kind,s", NON_DEFAULT)
def test_head_gemv_bn_fused_objective_matches_separate(kind, s, B, K, C):
    """gemv_head_bn == bn_apply_act + gemv_head + gan_loss with the objective: the written
    activation bitwise, the rest as tests/test_hip_kernels.py::test_head_gemv_bn_apply_fused."""
    h = H()
    obj = h.gan_loss_id(kind, s)
    x = bf(rnd(2 * B, K, scale=2.0, seed=113))
    w = rnd(K, scale=3.0 / K ** 0.5, seed=114)
    hb = rnd(1, seed=115)
    scale = (1 + 0.2 * rnd(2, C, seed=116)).contiguous()
    shift = (0.2 * rnd(2, C, seed=117)).contiguous()
    ya, yb = torch.empty_like(x), torch.empty_like(x)
    a, b = _bufs(B), _bufs(B)
    pr = _prog()
    pr.bn_apply_act("apply", _p(x), _p(ya), _p(scale), _p(shift), 2 * B * (K // C), C, B * (K // C), 2, 0.2, 0)
    pr.gemv_head("h", _p(ya), _p(w), _p(hb), _p(a[0]), 2 * B, K, 0)
    pr.gan_loss("l", _p(a[0]), B, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), 0, 0, obj, s)
    pr.gemv_head_bn("hbn", _p(x), _p(w), _p(hb), _p(b[0]), 2 * B, K, 0, _p(b[1]), _p(b[2]), _p(b[3]), _p(b[4]), 0,
                    _p(scale), _p(shift), C, B, 2, 0.2, _p(yb), obj, s)
    for _ in range(2):
        h.run(pr)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb)
        if kind == "hinge":  # a last-bit logit difference may not flip a mask: none sits that close
            assert float(torch.minimum((a[0][:B] - 1).abs().min(), (a[0][B:] + 1).abs().min())) > 1e-4
        for u, v in zip(a, b):  # same operands; FMA contraction may differ in the last bit
            torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6)
        yb.zero_()
        for u in b:
            u.fill_(float("nan"))


# ------------------------------------------------------------------ 3. the default is unchanged
def test_explicit_default_equals_todays_calls():
    h = H()
    B, K, C = 64, 8192, 512
    x = bf(rnd(2 * B, K, scale=2.0, seed=113))
    w = rnd(K, scale=0.02, seed=114)
    hb = rnd(1, seed=115)
    scale = (1 + 0.2 * rnd(2, C, seed=116)).contiguous()
    shift = (0.2 * rnd(2, C, seed=117)).contiguous()
    lg = rnd(2 * B, scale=4.0, seed=32)
    ls = torch.tensor([LOSS_SCALE, 0.0, 0.0], device=dev)
    sets = [[_bufs(B) for _ in range(3)] for _ in range(2)]
    ys = [torch.empty_like(x), torch.empty_like(x)]
    pr = _prog()
    for (l, g, gb), y, extra in zip(sets, ys, ((), (0, 0.0))):
        pr.gan_loss("l", _p(lg), B, _p(l[1]), _p(l[2]), _p(l[3]), _p(l[4]), 0, _p(ls), *extra)
        pr.gemv_head("h", _p(x), _p(w), _p(hb), _p(g[0]), 2 * B, K, 0, _p(g[1]), _p(g[2]), _p(g[3]), _p(g[4]), 0, *extra)
        pr.gemv_head_bn("hbn", _p(x), _p(w), _p(hb), _p(gb[0]), 2 * B, K, 0, _p(gb[1]), _p(gb[2]), _p(gb[3]),
                        _p(gb[4]), _p(ls), _p(scale), _p(shift), C, B, 2, 0.2, _p(y), *extra)
    h.run(pr)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    for today, explicit in zip(sets[0], sets[1]):
        for u, v in zip(today[1:], explicit[1:]):
            assert torch.equal(u, v) and bool(torch.isfinite(u).all())
    for u, v in zip(sets[0][1:], sets[1][1:]):
        assert torch.equal(u[0], v[0])  # the logits
    # today's values: the reference's three sigmoid cross-entropies
    losses, seed_d, _ = oracle(lg, "bce", 0.0)
    close(sets[0][0][1], losses, 1e-5, "losses")
    close(sets[0][0][2], seed_d * LOSS_SCALE, 1e-5, "dl_d")


# ------------------------------------------------------------------ 4. whole steps
def _real(B, cfg, edt=None):
    real = torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(5)) * 2 - 1
    real = real.to(dev)
    return real if edt is None else real.to(edt).float()


def _engine(cfg, B, **kw):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    kw.setdefault("graph", False)
    return HipEngine(cfg, B, dev, **kw)


def _scale_head(cfg, c, *models):
    """Multiply D's head Matrix by c (the head kernels read the fp32 master: no mirror to refresh)."""
    for m in models:
        m.d[cfg.d_lin_name + "/Matrix"].mul_(c)


def _masks_cut(xr, xf, what):
    """At least 2 rows on each side of x_r = 1 and of x_f = -1, none within 1e-3 of a threshold."""
    xr, xf = xr.flatten().float().cpu(), xf.flatten().float().cpu()
    counts = [int((xr > 1).sum()), int((xr < 1).sum()), int((xf > -1).sum()), int((xf < -1).sum())]
    margin = min(float((xr - 1).abs().min()), float((xf + 1).abs().min()))
    print("%s: rows x_r>1 %d, x_r<1 %d, x_f>-1 %d, x_f<-1 %d; nearest threshold %.4f" % (what, *counts, margin))
    assert min(counts) >= 2 and margin > 1e-3, (what, counts, margin)


# (size, c_dim, B, model seed, head constant): chosen on a CPU reference forward so that the
# reference logits alone put >= 2 rows on each side of both hinge thresholds
#   64x64x3 B=16 seed 3 x8:  8 / 8 real rows around 1, 7 / 9 fake rows around -1, nearest 0.47
#   28x28x1 B=8  seed 1 x16: 6 / 2 real, 2 / 6 fake, nearest 0.84
FP32_CASES = [(64, 3, 16, 3, 8.0), (28, 1, 8, 1, 16.0)]


@pytest.mark.parametrize("kind,s", NON_DEFAULT)
@pytest.mark.parametrize("size,c_dim,B,seed,c", FP32_CASES)
def test_engine_fp32_step_matches_reference_tightly(size, c_dim, B, seed, c, kind, s):
    """tests/test_hip_engine.py::test_engine_fp32_step_matches_reference_tightly with the
    objective: every live gradient within 1e-3 relative, losses within 1e-5, against the CPU fp32
    autograd reference. hinge: the head is scaled so that the masks cut (asserted on the reference)."""
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = _engine(cfg, B, seed=seed, dtype="fp32", gan_loss=kind, label_smooth=s)
    assert (eng.gan_loss, eng.label_smooth) == (kind, s)
    real = _real(B, cfg)
    eng.set_batch(real)
    ref_model = DCGAN(cfg, device=torch.device("cpu"), seed=seed)
    if kind == "hinge":
        _scale_head(cfg, c, eng.model, ref_model)
    eng.train_step()
    torch.cuda.synchronize()
    out, gd, gg = ReferenceStep(ref_model, gan_loss=kind, label_smooth=s).compute_grads(real.cpu(), eng.z.cpu())
    if kind == "hinge":
        _masks_cut(out["logits_real"].detach(), out["logits_fake"].detach(), "reference %dx%d" % (size, size))
    L = eng.last_losses()
    for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss"):
        r = float(out[k].detach())
        print(k, L[k], r)
        assert abs(L[k] - r) <= 1e-5 * max(1.0, abs(r)), (k, L[k], r)
    gdref, ggref = ref_model.d.like(), ref_model.g.like()
    gdref.flat.copy_(gd)
    ggref.flat.copy_(gg)
    gl_last = cfg.g_layers()[-1].name
    errs = {}
    for name in ref_model.d.names():
        if name.endswith("/biases") and not name.startswith("d_h0_conv"):
            continue  # dead bias (followed by BN)
        errs[name] = rel(eng.grad_d[name], gdref[name])
    for name in ref_model.g.names():
        if (name.endswith("/biases") and name.split("/")[0] != gl_last) or name == "g_h0_lin/bias":
            continue
        errs[name] = rel(eng.grad_g[name], ggref[name])
    print("fp32 %s s=%g relative grad errors (%dx%dx%d, B=%d): max %.2e" % (kind, s, size, size, c_dim, B,
                                                                           max(errs.values())))
    bad = {k: v for k, v in errs.items() if v > 1e-3}
    assert not bad, bad


def test_engine_bf16_lsgan_step_matches_reference():
    """tests/test_hip_engine.py::test_engine_step_matches_reference at 64x64x3 B=16, lsgan + s=0.1."""
    cfg, B = DCGANConfig(), 16
    eng = _engine(cfg, B, seed=3, gan_loss="lsgan", label_smooth=0.1)
    real = _real(B, cfg, torch.bfloat16)
    eng.set_batch(real)
    ref_model = DCGAN(cfg, device=dev, seed=3)
    assert torch.equal(ref_model.g.flat, eng.model.g.flat)
    eng.train_step()
    torch.cuda.synchronize()
    out, gd, gg = ReferenceStep(ref_model, gan_loss="lsgan", label_smooth=0.1).compute_grads(real, eng.z.clone())
    L = eng.last_losses()
    for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss"):
        r = float(out[k].detach())
        print(k, L[k], r)
        assert abs(L[k] - r) <= 3e-2 * max(1.0, abs(r)), (k, L[k], r)
    gdref, ggref = ref_model.d.like(), ref_model.g.like()
    gdref.flat.copy_(gd)
    ggref.flat.copy_(gg)
    gl_last = cfg.g_layers()[-1].name
    errs = {}
    for name in ref_model.d.names():
        if name.endswith("/biases") and not name.startswith("d_h0_conv"):
            continue
        errs[name] = rel(eng.grad_d[name], gdref[name])
    for name in ref_model.g.names():
        if name.endswith("/biases") and name.split("/")[0] != gl_last:
            continue
        errs[name] = rel(eng.grad_g[name], ggref[name])
    print("bf16 lsgan relative grad errors: " + ", ".join("%s %.4f" % kv for kv in errs.items()))
    small_sums = {gl_last + "/biases"}
    tol = {k: (0.35 if k.endswith("/biases") else 0.25) for k in errs}
    bad = {k: v for k, v in errs.items() if v > tol[k] and k not in small_sums}
    assert not bad, bad
    assert sum(errs.values()) / len(errs) < 0.15
    assert eng.global_step == 1


def test_engine_fp16_lsgan_step_matches_reference():
    """tests/test_hip_engine.py::test_engine_fp16_step_matches_reference, lsgan + s=0.1."""
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    cfg, B = DCGANConfig(), 16
    eng = _engine(cfg, B, seed=3, dtype="fp16", gan_loss="lsgan", label_smooth=0.1)
    real = _real(B, cfg, torch.float16)
    eng.set_batch(real)
    ref_model = DCGAN(cfg, device=dev, seed=3)
    eng.train_step()
    torch.cuda.synchronize()
    out, gd, gg = ReferenceStep(ref_model, gan_loss="lsgan", label_smooth=0.1).compute_grads(real, eng.z.clone())
    L = eng.last_losses()
    for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss"):
        r = float(out[k].detach())
        print(k, L[k], r)
        assert abs(L[k] - r) <= 2e-2 * max(1.0, abs(r)), (k, L[k], r)
    scale = HipEngine.INIT_LOSS_SCALE  # raw engine grads carry the loss scale
    e_d = rel(eng.grad_d.flat / scale, gd)
    e_g = rel(eng.grad_g.flat / scale, gg)
    print("fp16 lsgan whole-step relative grad error: D %.4f G %.4f" % (e_d, e_g))
    assert e_d < 0.1 and e_g < 0.15


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_engine_16bit_hinge_seeds_follow_own_logits(dtype):
    """A 16-bit logit error can flip a hinge mask against the fp32 reference, so the seeds and
    losses are checked against the oracle on the engine's OWN logits (the backward below the
    seeds is the code every other engine test covers). Head scaled as in the fp32 test."""
    cfg, B = DCGANConfig(), 16
    eng = _engine(cfg, B, seed=3, dtype=dtype, gan_loss="hinge")
    eng.set_batch(_real(B, cfg, torch.bfloat16 if dtype == "bf16" else torch.float16))
    _scale_head(cfg, 8.0, eng.model)
    k = float(eng.loss_scale[0]) if dtype == "fp16" else 1.0
    assert k == (LOSS_SCALE if dtype == "fp16" else 1.0)
    eng.train_step()
    torch.cuda.synchronize()
    _masks_cut(eng.logits[:B], eng.logits[B:], "%s engine" % dtype)
    losses, seed_d, seed_g = oracle(eng.logits, "hinge", 0.0)
    assert float((eng.dl_d / k - seed_d).abs().max()) <= 1e-6
    assert float((eng.dl_g / k - seed_g).abs().max()) <= 1e-6
    for half in (eng.dl_d[:B], eng.dl_d[B:]):  # both mask states occur in each half
        assert 0 < int((half == 0).sum()) < B
    if dtype == "fp16":  # the seeds carry the current loss scale
        assert float(eng.dl_d.abs().max()) == LOSS_SCALE / B and bool((eng.dl_g == -LOSS_SCALE / B).all())
    L = eng.last_losses()
    close(torch.tensor([L[n] for n in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss")]), losses.cpu(), 1e-5, "losses")
    close(eng.prob, torch.sigmoid(eng.logits), 1e-5, "prob")
    finite = bool(torch.isfinite(eng.grad_d.flat).all()) and bool(torch.isfinite(eng.grad_g.flat).all())
    if dtype == "fp16":
        # seeds of 2048 through a head scaled by 8 overflow fp16 further down (16x the gradients of
        # the default objective at this scale): the dynamic loss scaling answers as for any overflow
        assert float(eng.loss_scale[0]) == (LOSS_SCALE if finite else LOSS_SCALE / 2)
    else:
        assert finite and float(eng.grad_d.flat.abs().max()) > 0 and float(eng.grad_g.flat.abs().max()) > 0


# ------------------------------------------------------------------ 5. replay, eval_losses, DDP
def test_engine_graph_replay_matches_eager_with_hinge():
    cfg, B = DCGANConfig(), 8
    real = _real(B, cfg)
    e1 = _engine(cfg, B, seed=1, graph=False, gan_loss="hinge")
    e2 = _engine(cfg, B, seed=1, graph=True, gan_loss="hinge")
    for e in (e1, e2):
        e.set_batch(real)
    for _ in range(5):
        e1.train_step()
        e2.train_step()
        torch.cuda.synchronize()
        assert e1.last_losses() == e2.last_losses()
    assert e2.graph_enabled and not e1.graph_enabled and e2.global_step == 5
    assert torch.equal(e1.model.g.flat, e2.model.g.flat) and torch.equal(e1.model.d.flat, e2.model.d.flat)
    assert torch.equal(e1.dl_d, e2.dl_d) and torch.equal(e1.dl_g, e2.dl_g)


def test_eval_losses_with_hinge():
    cfg, B = DCGANConfig(), 8
    eng = _engine(cfg, B, seed=2, gan_loss="hinge")
    real = _real(B, cfg)
    eng.set_batch(real)
    eng.train_step()
    torch.cuda.synchronize()
    kept = eng.losses.clone()
    z = (torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    ev = eng.eval_losses(real, z)
    torch.cuda.synchronize()
    losses, _, _ = oracle(eng.logits, "hinge", 0.0)  # (the eval forward wrote eng.logits)
    close(torch.tensor([ev["g_loss"], ev["d_loss"]]), losses[2:].cpu(), 1e-5, "eval losses")
    assert abs(ev["g_loss"] + float(eng.logits[B:].mean())) <= 1e-5 * max(1.0, abs(ev["g_loss"]))
    assert torch.equal(eng.losses, kept)


STEPS = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_engine():
    cfg, B = DCGANConfig(), 16
    eng = _engine(cfg, B, seed=3, graph=False, rank_seeded_z=False, gan_loss="lsgan", label_smooth=0.1)
    eng.set_batch(_real(B, cfg))
    return eng


def _rccl_worker(out_dir, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["DCGAN_FORCE_DDP"] = "1"
    os.environ["DCGAN_DDP_SCHEDULE"] = "concurrent"
    os.environ["DCGAN_DDP_SHARD"] = "0"
    os.environ.pop("DCGAN_DIST_BACKEND", None)
    torch.cuda.set_device(0)
    from distributed_tensorflow_for_dcgan_amd.parallel import dist as D
    import torch.distributed as tdist
    D.init_distributed(1, 0, torch.device("cuda", 0))
    eng = _ddp_engine()
    assert eng.ddp and eng._schedule() == "concurrent"
    for _ in range(STEPS):
        eng.train_step()
    torch.cuda.synchronize()
    torch.save({"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "losses": eng.losses.cpu(),
                "step": eng.global_step, "backend": tdist.get_backend(), "kind": eng.gan_loss,
                "s": eng.label_smooth}, os.path.join(out_dir, "rccl.pt"))
    D.barrier()
    D.shutdown()


def test_rccl_single_rank_ddp_lsgan_matches_fused(tmp_path):
    eng = _ddp_engine()
    assert not eng.ddp and eng._schedule() == "fused"
    for _ in range(STEPS):
        eng.train_step()
    torch.cuda.synchronize()
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), _free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and (r["kind"], r["s"]) == ("lsgan", 0.1)
    assert torch.equal(r["g"], eng.model.g.flat.cpu())
    assert torch.equal(r["d"], eng.model.d.flat.cpu())
    assert torch.equal(r["losses"], eng.losses.cpu())
    # ... and it is the least-squares objective that trained: the losses are the oracle's on the last logits
    losses, _, _ = oracle(eng.logits, "lsgan", 0.1)
    close(eng.losses, losses, 1e-5, "fused losses")
