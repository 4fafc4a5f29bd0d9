"""GPU tests of the D-only sub-steps (``d_steps`` > 1), ``beta2`` and the per-network learning rates
of the HIP engine: the sub-step's update kernels (adam1 = Adam + mirror + D's powers in one launch;
step_end as the sub-step records it, without G's powers and the step), a sub-step and whole cycles
against ``ReferenceStep`` (bf16 / fp16 / fp32), the z of the sub-steps, hipGraph replay, the fp16 overflow sub-step, one-rank RCCL DDP, checkpoint resume through
the trainer, and that the defaults change nothing.

Comparisons with the reference are those of ``test_step_matches_reference`` in
test_hip_d_spectral_norm.py (its helpers are imported, its tolerances repeated in ``_check_piece``):
fp32 against the CPU reference, losses 1e-5, every live gradient 1e-3, activations at a kink
compared on the engine's side after showing that they are kinks; bf16 losses 3e-2, gradients 0.25
(biases 0.35), mean 0.15; fp16 losses 2e-2, D 0.1, G 0.15. Parameters: the engine's new D weights
are TF-Adam (fp32 oracle, the tolerance of test_hip_kernels.py::test_adam_matches_tf_formula) of the
engine's own gradient, which the gradient comparison ties to the reference's.

Measured on an MI355X (B = 8; 24 single sub-steps and 4 cycles of 9 pieces): fp32 largest per-tensor
gradient error 9.9e-5 (d_h3_lin/bias; otherwise 1e-6..1e-5; bound 1e-3), 3 of 17 fp32 pieces with an
activation on the other side of a kink, largest |input| 4.1e-7 (bound 1e-6); bf16 largest per-tensor
error 0.16 (g_bn2/beta in a full step; sub-steps <= 0.14; bounds 0.25 / 0.35); fp16 D <= 0.031,
G <= 0.012 (bounds 0.1 / 0.15)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

import test_hip_d_spectral_norm as SNT  # the full step's comparison helpers
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BUILDS = SNT.BUILDS
PAD = SNT.PAD
rel, _padded, _canaries_intact = SNT.rel, SNT._padded, SNT._canaries_intact
ENV = ("DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_D_UPDATE", "DCGAN_D_SPECTRAL_NORM",
       "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


# ------------------------------------------------------------------ kernels
def _adam_sizes():
    cap = H().adam1_max_blocks()
    # one vector; less than one block's worth; one vector past two whole grid passes (cap blocks
    # x 256 threads x one float4 each), so the grid-stride loop's tail iteration runs
    return [4, 1020, (2 * cap * 256 + 1) * 4]


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_adam1_equals_adam_plus_powers_and_the_tf_oracle(which, build):
    h = H()
    n = _adam_sizes()[which]
    edt, dt = BUILDS[build], int(build == "fp16")
    g0 = torch.Generator().manual_seed(40 + which)
    w0 = torch.randn(n, generator=g0) * 0.02
    grads = [torch.randn(n, generator=g0) * 1e-2 for _ in range(3)]
    lr, b1, b2, eps, gscale = 3e-4, 0.5, 0.9, 1e-8, 0.5
    bufs, views = {}, {}
    for side in ("one", "two"):
        for name, x, dtp in (("w", w0, None), ("wbf", torch.zeros(n), edt), ("m", torch.zeros(n), None),
                             ("v", torch.zeros(n), None), ("p", torch.tensor([b1, b2]), None),
                             ("g", torch.zeros(n), None)):
            bufs[side, name], views[side, name] = _padded(x, dtype=dtp)
    wr, mr, vr, b1p, b2p = w0.clone(), torch.zeros(n), torch.zeros(n), b1, b2
    for g in grads:
        for side in ("one", "two"):
            views[side, "g"].copy_(g)
        a = {k: views["one", k] for k in ("w", "wbf", "g", "m", "v", "p")}
        h.adam1_(a["w"], a["wbf"], a["g"], a["m"], a["v"], a["p"], lr, b1, b2, eps, gscale)
        b = {k: views["two", k] for k in ("w", "wbf", "g", "m", "v", "p")}
        prog = h.ext().Program(dt)
        prog.adam_bf("adam", b["w"].data_ptr(), b["wbf"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(),
                     b["v"].data_ptr(), b["p"].data_ptr(), n, lr, b1, b2, eps, gscale, 0, 0, 0)
        prog.step_end("powers", b["p"].data_ptr(), 0, b1, b2, 0.0, 0.0, 0, 0)
        h.run(prog)
        torch.cuda.synchronize()
        R.tf_adam_update(wr, g * gscale, mr, vr, b1p, b2p, lr, b1, b2, eps)
        b1p *= b1
        b2p *= b2
        for k in ("w", "wbf", "m", "v", "p", "g"):
            assert torch.equal(views["one", k], views["two", k]), (k, n)
    for key, buf in bufs.items():
        assert _canaries_intact(buf), key
    w = views["one", "w"].cpu()
    assert torch.allclose(w, wr, atol=1e-6, rtol=1e-5)  # (test_adam_matches_tf_formula's tolerance)
    assert torch.allclose(views["one", "p"].cpu(), torch.tensor([b1p, b2p]), rtol=1e-6)
    assert torch.equal(views["one", "wbf"].cpu(), w.to(edt)) and not torch.equal(w, w0)


def test_adam1_rejects_bad_arguments():
    h = H()
    t = lambda n, d=torch.float32: torch.zeros(n, dtype=d, device=dev)  # noqa: E731
    p = torch.tensor([0.5, 0.9], device=dev)
    with pytest.raises(ValueError):
        h.adam1_(t(6), t(6, torch.bfloat16), t(6), t(6), t(6), p, 1e-4, 0.5, 0.9, 1e-8)   # n % 4
    with pytest.raises(TypeError):
        h.adam1_(t(8), t(8), t(8), t(8), t(8), p, 1e-4, 0.5, 0.9, 1e-8)                     # fp32 mirror
    with pytest.raises(ValueError):
        h.adam1_(t(8), t(4, torch.bfloat16), t(8), t(8), t(8), p, 1e-4, 0.5, 0.9, 1e-8)
    with pytest.raises(RuntimeError):
        h.ext().Program(2).adam1("x", 1, 1, 1, 1, 1, 1, 8, 1e-4, 0.5, 0.9, 1e-8, 1.0, 0)   # the fp32 build has none


@pytest.mark.parametrize("ls0,want_ls,advance", [([1024.0, 1.0, 5.0], [512.0, 0.0, 0.0], False),
                                                 ([1024.0, 0.0, 5.0], [1024.0, 0.0, 6.0], True),
                                                 ([1024.0, 0.0, 1999.0], [2048.0, 0.0, 0.0], True),
                                                 (None, None, True)])
def test_d_step_end_kernel(ls0, want_ls, advance):
    """The sub-step's op as the engine records it: step_end with null G powers and null step.
    Overflow: halve, clear, D's powers stay; a good step: count; growth at the interval: double.
    G's powers (the neighbouring floats) and the step counter are bitwise untouched."""
    _check_step_end(ls0, want_ls, advance, with_g_and_step=False)


@pytest.mark.parametrize("ls0,want_ls,advance", [([1024.0, 0.0, 5.0], [1024.0, 0.0, 6.0], True),
                                                 ([1024.0, 1.0, 5.0], [512.0, 0.0, 0.0], False)])
def test_step_end_kernel_with_g_powers_and_step(ls0, want_ls, advance):
    """The full step's op: a good step advances both power pairs and the counter; an overflowed one
    advances the counter only, halves the scale and clears the flag."""
    _check_step_end(ls0, want_ls, advance, with_g_and_step=True)


def _check_step_end(ls0, want_ls, advance, with_g_and_step):
    h = H()
    b1, b2, b1g, b2g = 0.5, 0.9, 0.75, 0.999
    buf, view = _padded(torch.tensor([0.25, 0.81, 0.125, 0.729]))  # [D's powers | G's powers]
    sbuf = torch.full((2 * PAD + 1,), -3, dtype=torch.int64, device=dev)
    step = sbuf[PAD:PAD + 1]
    step.fill_(7)
    lsb, ls = (None, None) if ls0 is None else _padded(torch.tensor(ls0))
    prog = h.ext().Program()
    if with_g_and_step:
        prog.step_end("step_end", view[:2].data_ptr(), view[2:].data_ptr(), b1, b2, b1g, b2g, step.data_ptr(), 0,
                      0 if ls is None else ls.data_ptr(), 2000)
    else:
        prog.step_end("d_step_end", view[:2].data_ptr(), 0, b1, b2, 0.0, 0.0, 0, 0,
                      0 if ls is None else ls.data_ptr(), 2000)
    h.run(prog)
    torch.cuda.synchronize()
    f32 = lambda *x: torch.tensor(x, dtype=torch.float32)  # noqa: E731  (the products rounded as the kernel's)
    want_d = f32(0.25, 0.81) * f32(b1, b2) if advance else f32(0.25, 0.81)
    want_g = f32(0.125, 0.729) * f32(b1g, b2g) if advance and with_g_and_step else f32(0.125, 0.729)
    assert torch.equal(view[:2].cpu(), want_d)
    assert torch.equal(view[2:].cpu(), want_g) and int(step) == (8 if with_g_and_step else 7)
    assert _canaries_intact(buf) and _canaries_intact(sbuf, fill=-3)
    if ls is not None:
        assert ls.tolist() == want_ls and _canaries_intact(lsb)


# ------------------------------------------------------------------ a sub-step / the cycle vs the reference
def _reals(B, cfg, dtype, n):
    out = []
    for k in range(n):
        x = torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(5 + k)) * 2 - 1
        out.append(x.to(BUILDS[dtype]).float())
    return out


def _engine(cfg, B=8, d_steps=2, **kw):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    kw.setdefault("graph", False)
    eng = HipEngine(cfg, B, dev, d_steps=d_steps, **kw)
    for k, x in enumerate(_reals(B, cfg, kw.get("dtype", "bf16"), d_steps)):
        eng.set_batch(x.to(dev), k)
    return eng


def _g_state(eng):
    t = [eng.model.g.flat, eng.wbf_g.flat, eng.opt_g.m.flat, eng.opt_g.v.flat, eng.opt_g.powers, eng.model.g_bn.flat,
         torch.as_tensor(eng.model.g_bn.steps), eng.step_counter]
    if eng.g_ema is not None:
        t += [eng.g_ema.flat, eng.wbf_g_ema.flat]
    return [x.detach().cpu().clone() for x in t]


def _d_state(eng):
    t = [eng.model.d.flat, eng.wbf_d.flat, eng.opt_d.m.flat, eng.opt_d.v.flat, eng.opt_d.powers]
    if eng.d_spectral_norm:
        t += [eng.model.d_sn.flat, eng.sn_head]
    return [x.detach().cpu().clone() for x in t]


def _sync_ref(ref_model, eng, sn):
    ref_model.g.flat.copy_(eng.model.g.flat)
    ref_model.d.flat.copy_(eng.model.d.flat)
    if sn:
        ref_model.d_sn.flat.copy_(eng.model.d_sn.flat)


def _check_piece(eng, ref, ref_model, cfg, real, dtype, sn, full, run, tag):
    """Run one piece of the cycle on the engine (`run`: a D sub-step, or the full step) from the
    engine's own state and compare its losses, gradients and -- for D -- the parameters it wrote
    with the reference on the engine's z. full: compare G's gradients too."""
    rdev = next(iter(ref_model.d.tensors.values())).device
    _sync_ref(ref_model, eng, sn)
    scale = float(eng.loss_scale[0]) if dtype == "fp16" else 1.0
    od = eng.opt_d
    w0, m0, v0 = od.params.flat.cpu().clone(), od.m.flat.cpu().clone(), od.v.flat.cpu().clone()
    p0 = od.powers.cpu().clone()
    run()
    torch.cuda.synchronize()
    z = eng.z.to(rdev)
    grads = (lambda: ref.compute_grads(real, z, update_ema=False)) if full else \
        (lambda: ref.compute_d_grads(real, z) + (None,))
    bn_keep = (ref_model.d_bn.flat.clone(), ref_model.g_bn.flat.clone())  # (compute_d_grads moves D's averages)
    if dtype == "fp32":
        ins = []
        with SNT._recording(ins):  # the unmodified reference
            out, gd, gg = grads()
        signs = SNT._engine_signs(eng, cfg)
        assert len(ins) == len(signs)
        at_kink = [x.flatten()[(m.flatten() != (x.flatten() > 0))].abs() for x, m in zip(ins, signs)]
        flips = sum(k.numel() for k in at_kink)
        far = max([float(k.max()) for k in at_kink if k.numel()], default=0.0)
        near = sum(int((x.abs() < SNT.KINK_MAX_INPUT).sum()) for x in ins)
        print("%s fp32: %d activation(s) with another sign than the reference's, largest |input| %.2e; %d reference "
              "inputs below %.0e" % (tag, flips, far, near, SNT.KINK_MAX_INPUT))
        assert flips <= near and far < SNT.KINK_MAX_INPUT, (tag, flips, near, far)
        if flips:  # the same piece on the engine's side of those kinks
            with SNT._engine_masks(eng, cfg):
                out, gd, gg = grads()
    else:
        out, gd, gg = grads()
    ref_model.d_bn.flat.copy_(bn_keep[0])
    ref_model.g_bn.flat.copy_(bn_keep[1])
    L = eng.last_losses()
    ltol = {"fp32": 1e-5, "bf16": 3e-2, "fp16": 2e-2}[dtype]
    for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss"):
        r = float(out[k].detach())
        assert abs(L[k] - r) <= ltol * max(1.0, abs(r)), (tag, k, L[k], r)
    gl_last = cfg.g_layers()[-1].name
    dead = {L_.name + "/biases" for L_ in cfg.d_layers() if L_.bn} | {L_.name + "/biases" for L_ in cfg.g_layers() if L_.bn}
    if dtype == "fp16":
        e_d = rel(eng.grad_d.flat / scale, gd)
        e_g = rel(eng.grad_g.flat / scale, gg) if full else 0.0
        print("%s fp16 relative grad error: D %.4f G %.4f" % (tag, e_d, e_g))
        assert e_d < 0.1 and e_g < 0.15
    else:
        gdref = ref_model.d.like()
        gdref.flat.copy_(gd)
        errs = {n: rel(eng.grad_d[n], gdref[n]) for n in ref_model.d.names() if n not in dead}
        if full:
            ggref = ref_model.g.like()
            ggref.flat.copy_(gg)
            for n in ref_model.g.names():
                if n not in dead and not (dtype == "fp32" and n == "g_h0_lin/bias"):
                    errs[n] = rel(eng.grad_g[n], ggref[n])
        print("%s %s max rel grad error %.3e (%s)" % (tag, dtype, max(errs.values()), max(errs, key=errs.get)))
        if dtype == "fp32":
            bad = {k: v for k, v in errs.items() if v > 1e-3}
        else:
            bad = {k: v for k, v in errs.items()
                   if v > (0.35 if k.endswith("/biases") else 0.25) and k != gl_last + "/biases"}
            assert sum(errs.values()) / len(errs) < 0.15
        assert not bad, (tag, bad)
    # D's parameters: TF-Adam(lr_d, beta1, beta2) of the engine's gradient from the pre-step state
    b1p, b2p = float(p0[0]), float(p0[1])
    R.tf_adam_update(w0, eng.grad_d.flat.cpu() / scale, m0, v0, b1p, b2p, od.lr, od.beta1, od.beta2, od.eps)
    assert torch.allclose(od.params.flat.cpu(), w0, atol=1e-6, rtol=1e-5), tag
    assert torch.allclose(od.powers.cpu(), torch.tensor([b1p * od.beta1, b2p * od.beta2]), rtol=1e-6), tag
    if not eng.f32:  # the 16-bit mirror (with spectral norm its kernel slices hold W / sigma: checked below)
        name = "d_h0_conv/biases"
        got, want = (eng.wbf_d[name], eng.model.d[name]) if sn else (eng.wbf_d.flat, eng.model.d.flat)
        assert torch.equal(got, want.to(eng.edt)), tag
    if sn:  # one power step on the new weights from the stored u, copies rewritten
        snr = ref_model.d_sn
        snr.power_step_({k: v.to(rdev) for k, v in eng.model.d.tensors.items()})
        for name, _, _ in snr.shapes:
            for a, b in ((eng.model.d_sn.u[name], snr.u[name]), (eng.model.d_sn.v[name], snr.v[name]),
                         (eng.model.d_sn.sigma[name], snr.sigma[name])):
                assert rel(a, b) < 1e-5, (tag, name)
        SNT._copies_match_state(eng)


def _ref_for(cfg, dtype, seed, sn, **kw):
    rdev = torch.device("cpu") if dtype == "fp32" else dev
    ref_model = DCGAN(cfg, device=rdev, seed=seed)
    return ref_model, ReferenceStep(ref_model, d_spectral_norm=sn, seed=seed, **kw), rdev


@pytest.mark.parametrize("size,c_dim", [(28, 1), (64, 3)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("sn,bn", [(True, True), (True, False), (False, False), (False, True)])
def test_sub_step_matches_reference(sn, bn, dtype, size, c_dim, seed=3):
    """``train_d_step(0)`` from the common initial state: D's gradients, parameters and losses
    against ``ReferenceStep`` on the engine's z; everything of G and the step counter bitwise
    unchanged; D's BN moving averages moved. (With live Adam slots and powers: the cycle test.)"""
    B = 8
    cfg = DCGANConfig(output_size=size, c_dim=c_dim, d_bn=bn)
    kw = dict(beta2=0.9, lr_d=3e-4, lr_g=1e-4)
    eng = _engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=sn, g_ema_decay=0.999, **kw)
    ref_model, ref, rdev = _ref_for(cfg, dtype, seed, sn, **kw)
    assert (eng.opt_d.lr, eng.opt_g.lr, eng.opt_d.beta2) == (3e-4, 1e-4, 0.9)
    torch.cuda.synchronize()
    g0, d0 = _g_state(eng), _d_state(eng)
    dbn0, dbn_steps0 = eng.model.d_bn.flat.clone(), torch.as_tensor(eng.model.d_bn.steps).clone()
    real0 = _reals(B, cfg, dtype, 1)[0].to(rdev)
    _check_piece(eng, ref, ref_model, cfg, real0, dtype, sn, False, lambda: eng.train_d_step(0), "sub-step")
    for k, (x, y) in enumerate(zip(g0, _g_state(eng))):
        assert torch.equal(x, y), "G state %d changed" % k
    assert eng.global_step == 0
    assert not any(torch.equal(x, y) for x, y in zip(d0, _d_state(eng)))
    assert torch.equal(torch.as_tensor(eng.model.d_bn.steps), dbn_steps0 + 1)
    if bn:
        assert not torch.equal(eng.model.d_bn.flat, dbn0)
    names = eng.sub_op_names(0)
    assert len([n for n in names if n in ("adam_d", "adam_d1")]) == 1
    assert ("adam_d1" in names) == (dtype == "bf16")


@pytest.mark.parametrize("dtype,size,c_dim,sn,bn", [("bf16", 64, 3, False, True), ("bf16", 28, 1, True, False),
                                                    ("fp16", 28, 1, True, False), ("fp32", 28, 1, True, True)])
def test_three_training_steps_track_the_reference_cycle(dtype, size, c_dim, sn, bn, seed=4):
    """d_steps = 3. Engine `a` runs ``train_step`` three times. Engine `b` runs the same cycle piece
    by piece -- sub-step 0, sub-step 1, the full step, each on its own staged batch -- and every
    piece is compared with the reference from b's state (``_check_piece``). Then a == b bitwise:
    ``train_step`` is that cycle, in that order, on those batches and z."""
    B = 8
    cfg = DCGANConfig(output_size=size, c_dim=c_dim, d_bn=bn)
    a = _engine(cfg, B, 3, dtype=dtype, seed=seed, d_spectral_norm=sn, beta2=0.9, g_ema_decay=0.999)
    b = _engine(cfg, B, 3, dtype=dtype, seed=seed, d_spectral_norm=sn, beta2=0.9, g_ema_decay=0.999)
    ref_model, ref, rdev = _ref_for(cfg, dtype, seed, sn, beta2=0.9)
    reals = [x.to(rdev) for x in _reals(B, cfg, dtype, 3)]
    for step in range(3):
        a.train_step()
        for k in range(2):
            g0 = _g_state(b)
            _check_piece(b, ref, ref_model, cfg, reals[k], dtype, sn, False, lambda: b.train_d_step(k),
                         "step %d sub-step %d" % (step, k))
            for x, y in zip(g0, _g_state(b)):  # G (live slots, powers, counts) and the step counter
                assert torch.equal(x, y)
            assert b.global_step == step
        _check_piece(b, ref, ref_model, cfg, reals[2], dtype, sn, True, b.train_full_step, "step %d full" % step)
        torch.cuda.synchronize()
        assert a.global_step == b.global_step == step + 1
        assert a.last_losses() == b.last_losses()
        for x, y in zip(_g_state(a) + _d_state(a), _g_state(b) + _d_state(b)):
            assert torch.equal(x, y)
        assert torch.equal(a.model.d_bn.flat, b.model.d_bn.flat) and torch.equal(a.model.g_bn.flat, b.model.g_bn.flat)
    # D's powers advanced 9 times, G's 3 times
    assert float(a.opt_d.powers[1]) == pytest.approx(0.9 ** 10, rel=1e-5)
    assert float(a.opt_g.powers[1]) == pytest.approx(0.9 ** 4, rel=1e-5)
    assert list(torch.as_tensor(a.model.d_bn.steps)) == [9, 9] and list(torch.as_tensor(a.model.g_bn.steps)) == [3]


def test_z_of_the_sub_steps():
    cfg = DCGANConfig(output_size=28, c_dim=1)

    def draw():
        eng = _engine(cfg, 8, 3, seed=6)
        zs = []
        for _ in range(2):
            for run in (lambda: eng.train_d_step(0), lambda: eng.train_d_step(1), eng.train_full_step):
                run()
                torch.cuda.synchronize()
                zs.append(eng.z.cpu().clone())
        return zs
    zs, again = draw(), draw()
    for i in range(len(zs)):
        assert float(zs[i].min()) >= -1.0 and float(zs[i].max()) <= 1.0 and float(zs[i].std()) > 0.4
        for j in range(i):
            assert not torch.equal(zs[i], zs[j]), (i, j)
    for x, y in zip(zs, again):  # a second engine built from the same seeds draws the same ones
        assert torch.equal(x, y)
    # the full step's z is the one an engine without sub-steps draws
    one = _engine(cfg, 8, 1, seed=6)
    one.train_step()
    torch.cuda.synchronize()
    assert torch.equal(one.z.cpu(), zs[2])


# ------------------------------------------------------------------ graph == eager, defaults, fp16 skip
def _snap(eng):
    torch.cuda.synchronize()
    return _g_state(eng) + _d_state(eng) + [eng.model.d_bn.flat.cpu().clone(), eng.model.g_bn.flat.cpu().clone(),
                                             eng.losses.cpu().clone()]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_graph_replay_matches_eager(dtype):
    cfg = DCGANConfig(d_bn=False)
    e1 = _engine(cfg, 16, 3, dtype=dtype, seed=1, d_spectral_norm=True, g_ema_decay=0.999)
    e2 = _engine(cfg, 16, 3, dtype=dtype, seed=1, d_spectral_norm=True, g_ema_decay=0.999, graph=True)
    for _ in range(4):
        e1.train_step()
        e2.train_step()
        for x, y in zip(_snap(e1), _snap(e2)):
            assert torch.equal(x, y)
    assert e2.graph_enabled and not e1.graph_enabled and e1.global_step == e2.global_step == 4
    assert [len(g) for g in e2._sub_graphs] == [1, 1]  # one captured graph per sub-step


def test_defaults_change_nothing():
    cfg = DCGANConfig()
    plain = _engine(cfg, 16, 1, seed=1)
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    bare = HipEngine(cfg, 16, dev, seed=1, graph=False)  # built without the arguments
    bare.set_batch(_reals(16, cfg, "bf16", 1)[0].to(dev))
    dflt = _engine(cfg, 16, 1, seed=1, beta2=R.ADAM_BETA2, lr_d=None, lr_g=None)
    assert bare.op_names() == dflt.op_names() == plain.op_names()
    assert bare.kernel_count() == dflt.kernel_count()
    for p in ("progA", "progB", "progW", "progC", "progX", "progCast"):
        assert getattr(bare, p).size() == getattr(dflt, p).size(), p
    assert dflt._sub == [] and dflt.progDU is None and len(dflt.d_ins) == 1 and dflt.d_ins[0] is dflt.d_in
    for _ in range(3):
        bare.train_step()
        dflt.train_step()
        for x, y in zip(_snap(bare), _snap(dflt)):
            assert torch.equal(x, y)
    other = _engine(cfg, 16, 1, seed=1, beta2=0.9)
    other.train_step()
    other.train_step()
    assert not torch.equal(_snap(other)[0], _snap(dflt)[0])  # (and beta2 does train another model)


def test_fp16_overflow_sub_step_leaves_the_state():
    eng = _engine(DCGANConfig(d_bn=False), 16, 2, seed=1, dtype="fp16", d_spectral_norm=True)
    eng.train_step()
    torch.cuda.synchronize()
    assert eng.loss_scale.tolist()[1] == 0.0
    d0, g0 = _d_state(eng), _g_state(eng)
    good = eng.loss_scale.tolist()[2]
    eng.loss_scale[0] = 1e38
    eng.train_d_step(0)
    torch.cuda.synchronize()
    ls = eng.loss_scale.tolist()
    assert ls[1:] == [0.0, 0.0] and good >= 2.0 and ls[0] == pytest.approx(0.5e38, rel=1e-6)
    for x, y in zip(d0 + g0, _d_state(eng) + _g_state(eng)):  # Adam(D), D's powers and sn_power skipped
        assert torch.equal(x, y)
    eng.loss_scale[0] = 1024.0
    eng.train_d_step(0)  # the next sub-step proceeds
    torch.cuda.synchronize()
    assert eng.loss_scale.tolist() == [1024.0, 0.0, 1.0]
    assert not any(torch.equal(x, y) for x, y in zip(d0, _d_state(eng)))
    for x, y in zip(g0, _g_state(eng)):
        assert torch.equal(x, y)
    SNT._copies_match_state(eng)


# ------------------------------------------------------------------ one-rank RCCL DDP
STEPS = 3


def _ddp_engine(graph):
    return _engine(DCGANConfig(d_bn=False), 16, 2, seed=3, graph=graph, rank_seeded_z=False, d_spectral_norm=True,
                   beta2=0.9)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "sn": eng.model.d_sn.flat.cpu(),
            "mirror": eng.wbf_d.flat.cpu(), "head": eng.sn_head.cpu(), "pd": eng.opt_d.powers.cpu(),
            "pg": eng.opt_g.powers.cpu(), "losses": eng.losses.cpu()}


def _rccl_worker(out_dir, graph, port):
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
    eng = _ddp_engine(graph)
    assert eng.ddp and eng._schedule() == "concurrent"
    for _ in range(STEPS):
        eng.train_step()
    out = _result(eng)
    out.update({"step": eng.global_step, "backend": tdist.get_backend(), "graph": eng.graph_enabled,
                "ops": eng.sub_op_names(0), "sub_graphs": [len(g) for g in eng._sub_graphs]})
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


@pytest.mark.parametrize("graph", [False, True])
def test_rccl_single_rank_ddp_matches_fused(tmp_path, graph, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), graph, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"] == graph
    assert "adam_d" in r["ops"] and "d_step_end" in r["ops"] and "adam_d1" not in r["ops"]
    assert r["sub_graphs"] == ([4] if graph else [])
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k


# ------------------------------------------------------------------ checkpoint resume through the trainer
def test_trainer_resume_is_exact_with_d_steps(tmp_path, monkeypatch):
    """bf16, d_steps = 2: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more --
    every saved tensor bitwise (D's powers after 8 updates included), and no key beyond the
    default run's."""
    import io
    from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
    from distributed_tensorflow_for_dcgan_amd.data import pipeline as P
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    from distributed_tensorflow_for_dcgan_amd.utils import flags as F
    made = []

    def source(flags, batch, shape, device, **kw):  # two alternating batches, restarted with every run
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
        made.append(Two())
        return made[-1]
    monkeypatch.setattr(T, "make_source", source)

    def run(ck, steps, d_steps=2):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--d_steps=%d" % d_steps, "--beta2=0.9",
                            "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries", "--save_model_secs=1e9",
                            "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"])
        out = io.StringIO()
        assert T.run(fl, out=out) == 0, out.getvalue()
        return out.getvalue()

    def load(ck, d_steps=2):
        from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
        eng = HipEngine(DCGANConfig(output_size=28, c_dim=1), 8, dev, seed=99, graph=False, d_steps=d_steps, beta2=0.9)
        info = CK.CheckpointManager(str(ck)).restore_latest(eng)
        torch.cuda.synchronize()
        return info, CK.collect_state(eng)
    run(tmp_path / "a", 4)
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    assert [m.i for m in made] == [8, 4, 4]  # two real batches per training step
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    assert float(sa["beta2_power"].reshape(-1)[0]) == pytest.approx(0.9 ** 9, rel=1e-5)
    assert float(sa["beta2_power_1"].reshape(-1)[0]) == pytest.approx(0.9 ** 5, rel=1e-5)
    run(tmp_path / "c", 1, d_steps=1)
    assert list(load(tmp_path / "c", 1)[1]) == list(sa)
