"""CPU tests of the selectable GAN objectives (``gan_loss`` = bce | lsgan | hinge, one-sided
``label_smooth``): the fp32 oracle against hand-written closed forms, the validator everywhere the
options can be set, the flags and environment defaults, the reference engine, the hazard check of
every schedule on dry-run HIP engines, and the command line."""
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F
from test_g_ema import CASES

CPU = torch.device("cpu")
SMALL = DCGANConfig(output_size=28, c_dim=1)
KINDS = [("bce", 0.0), ("bce", 0.1), ("lsgan", 0.0), ("lsgan", 0.1), ("hinge", 0.0)]
# the thresholds of every objective (hinge: 1 and -1; the clamp of bce: 0) sit in both halves
XR = [1.0, -1.0, 0.0, 2.5, -3.0, 0.75, 1.25]
XF = [-1.0, 1.0, 0.0, -2.5, 3.0, -0.75, -1.25]


def _closed_form(kind, s):
    """(d_real, d_fake, g, seeds of d_loss on [real | fake], seed of g_loss on fake), python floats."""
    B, t = len(XR), 1.0 - s
    sp = lambda x: max(x, 0.0) + math.log1p(math.exp(-abs(x)))  # softplus(x)
    sg = lambda x: 1.0 / (1.0 + math.exp(-x))
    if kind == "bce":
        dr = sum(sp(x) - x * t for x in XR) / B
        df = sum(sp(x) for x in XF) / B
        g = sum(sp(x) - x for x in XF) / B
        sr, sf, gg = [(sg(x) - t) / B for x in XR], [sg(x) / B for x in XF], [(sg(x) - 1.0) / B for x in XF]
    elif kind == "lsgan":
        dr = 0.5 * sum((x - t) ** 2 for x in XR) / B
        df = 0.5 * sum(x * x for x in XF) / B
        g = 0.5 * sum((x - 1.0) ** 2 for x in XF) / B
        sr, sf, gg = [(x - t) / B for x in XR], [x / B for x in XF], [(x - 1.0) / B for x in XF]
    else:
        dr = sum(max(1.0 - x, 0.0) for x in XR) / B
        df = sum(max(1.0 + x, 0.0) for x in XF) / B
        g = -sum(XF) / B
        sr = [-1.0 / B if x < 1.0 else 0.0 for x in XR]   # torch's subgradient: 0 at the kink
        sf = [1.0 / B if x > -1.0 else 0.0 for x in XF]
        gg = [-1.0 / B] * B
    return dr, df, g, sr + sf, gg


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("kind,s", KINDS)
def test_oracle_matches_closed_forms(kind, s):
    xr = torch.tensor(XR, requires_grad=True)
    xf = torch.tensor(XF, requires_grad=True)
    dr, df, g, dl = R.gan_losses(xr, xf, kind, s) if (kind, s) != ("bce", 0.0) else R.gan_losses(xr, xf)
    assert torch.equal(dl, dr + df)
    e_dr, e_df, e_g, e_seed_d, e_seed_g = _closed_form(kind, s)
    # fp32 evaluation of sums of 7 terms of magnitude <= 8: a few ulp of the largest term
    for got, exp in ((dr, e_dr), (df, e_df), (g, e_g)):
        assert abs(float(got.detach()) - exp) <= 4e-6, (float(got.detach()), exp)
    gdr, gdf = torch.autograd.grad(dl, [xr, xf], retain_graph=True)
    (ggf,) = torch.autograd.grad(g, [xf])
    got_d, got_g = torch.cat([gdr, gdf]).double(), ggf.double()
    exp_d, exp_g = torch.tensor(e_seed_d, dtype=torch.float64), torch.tensor(e_seed_g, dtype=torch.float64)
    keep_d, keep_g = torch.ones(2 * len(XR), dtype=torch.bool), torch.ones(len(XF), dtype=torch.bool)
    if kind == "bce":
        # The TF form max(x,0) - x t + log1p(exp(-|x|)) is smooth, but written with two kinks at
        # x = 0 that cancel; autograd differentiates the pieces (clamp' = 1, |x|' = 0 there) and
        # returns 1 - t instead of sigmoid(0) - t at EXACTLY 0. The seed is the derivative of the
        # function, sigmoid(x) - t, which is what the kernels compute; autograd is the witness
        # everywhere else, and at 0 the oracle's value is checked to be that documented artefact.
        at0 = torch.tensor([x == 0.0 for x in XR + XF])
        keep_d, keep_g = ~at0, ~at0[len(XR):]
        B = len(XR)
        assert torch.allclose(got_d[at0], torch.tensor([(1.0 - (1.0 - s)) / B, 1.0 / B], dtype=torch.float64), atol=1e-7)
        assert torch.allclose(got_g[at0[B:]], torch.tensor([0.0], dtype=torch.float64), atol=1e-7)
    assert int(keep_d.sum()) >= 2 * len(XR) - 2
    assert torch.allclose(got_d[keep_d], exp_d[keep_d], rtol=0, atol=1e-6)
    assert torch.allclose(got_g[keep_g], exp_g[keep_g], rtol=0, atol=1e-6)
    if kind == "hinge":  # the masks are exact, at the kinks too
        B = len(XR)
        assert gdr.tolist() == [float(torch.tensor(-1.0 / B)) if x < 1.0 else 0.0 for x in XR]
        assert gdf.tolist() == [float(torch.tensor(1.0 / B)) if x > -1.0 else 0.0 for x in XF]


def test_two_argument_form_is_bce_without_smoothing():
    g = torch.Generator().manual_seed(5)
    xr, xf = 4 * torch.randn(33, generator=g), 4 * torch.randn(33, generator=g)
    for a, b in zip(R.gan_losses(xr, xf), R.gan_losses(xr, xf, kind="bce", label_smooth=0)):
        assert torch.equal(a, b)
    for a, b in zip(R.gan_losses(xr, xf), R.gan_losses(xr, xf, "bce", 0.1)):
        assert a.dtype == b.dtype == torch.float32
    assert not torch.equal(R.gan_losses(xr, xf)[0], R.gan_losses(xr, xf, "bce", 0.1)[0])
    assert torch.equal(R.gan_losses(xr, xf)[2], R.gan_losses(xr, xf, "bce", 0.1)[2])  # G's target is never smoothed


BAD = [("wgan", 0.0), ("BCE", 0.0), (None, 0.0), ("bce", -0.1), ("lsgan", 0.5), ("bce", 0.75), ("lsgan", float("nan")),
       ("hinge", 0.1)]


@pytest.mark.parametrize("kind,s", BAD)
def test_bad_objective_is_rejected_everywhere(kind, s, monkeypatch):
    monkeypatch.delenv("DCGAN_GAN_LOSS", raising=False)
    monkeypatch.delenv("DCGAN_LABEL_SMOOTH", raising=False)
    x = torch.zeros(2)
    with pytest.raises(ValueError):
        R.check_gan_loss(kind, s)
    with pytest.raises(ValueError):
        R.gan_losses(x, x, kind, s)
    if kind is not None:  # (None = "take the default" for the engines and has no spelling as a flag)
        with pytest.raises(SystemExit):
            F.parse_flags(["--gan_loss=%s" % kind, "--label_smooth=%r" % s])
        with pytest.raises(ValueError):
            ReferenceEngine(SMALL, 2, CPU, gan_loss=kind, label_smooth=s)
        with pytest.raises(ValueError):
            build_engine(SMALL, 2, CPU, engine="reference", gan_loss=kind, label_smooth=s)
        from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
        with pytest.raises(ValueError):
            HipEngine(SMALL, 2, CPU, dry_run=True, graph=False, gan_loss=kind, label_smooth=s)
        from distributed_tensorflow_for_dcgan_amd.ops import hip as H
        with pytest.raises(ValueError):
            H.gan_loss_id(kind, s)


def test_good_objectives_validate():
    assert R.check_gan_loss("bce") == ("bce", 0.0)
    assert R.check_gan_loss("lsgan", 0.25) == ("lsgan", 0.25)
    assert R.check_gan_loss("hinge", 0) == ("hinge", 0.0)
    assert R.check_gan_loss("bce", "0.1") == ("bce", 0.1)
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    assert [H.gan_loss_id(k) for k in R.GAN_LOSSES] == [0, 1, 2]


def test_bindings_reject_bad_objectives():
    """Program.gan_loss / gemv_head / gemv_head_bn on a dry (recording) program: std::runtime_error."""
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    pr = H.ext().Program(0, True)
    for obj, s in ((3, 0.0), (-1, 0.0), (0, 0.5), (1, -0.1), (0, float("nan")), (2, 0.1)):
        with pytest.raises(RuntimeError):
            pr.gan_loss("l", 4096, 4, 8192, 12288, 16384, 20480, 0, 0, obj, s)
        with pytest.raises(RuntimeError):
            pr.gemv_head("h", 4096, 8192, 12288, 16384, 8, 32, 0, 20480, 24576, 28672, 32768, 0, obj, s)
        with pytest.raises(RuntimeError):
            pr.gemv_head_bn("hb", 4096, 8192, 12288, 16384, 4, 2048, 0, 20480, 24576, 28672, 32768, 0, 36864, 40960,
                            8, 2, 2, 0.2, 65536, obj, s)
    assert pr.size() == 0
    pr.gan_loss("l", 4096, 4, 8192, 12288, 16384, 20480, 0, 0, 2, 0.0)
    pr.gan_loss("l", 4096, 4, 8192, 12288, 16384, 20480, 0)  # today's call
    assert pr.size() == 2
    assert pr.op_info(0)[4] == pr.op_info(1)[4]  # the same byte ranges


# ------------------------------------------------------------------ 2. flags and environment
def test_flags_parse_and_defaults():
    fl = F.parse_flags([])
    assert fl.gan_loss == "bce" and fl.label_smooth == 0.0
    assert F.default_flags().gan_loss == "bce" and F.default_flags().label_smooth == 0.0
    fl = F.parse_flags(["--gan_loss=lsgan", "--label_smooth", "0.1"])
    assert fl.gan_loss == "lsgan" and fl.label_smooth == 0.1
    assert fl.explicitly_set("gan_loss") and fl.explicitly_set("label_smooth")
    assert F.parse_flags(["--gan_loss", "hinge"]).gan_loss == "hinge"
    with pytest.raises(SystemExit):
        F.parse_flags(["--gan_loss=hinge", "--label_smooth=0.1"])


def test_env_switches_set_the_engine_default(monkeypatch):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    monkeypatch.delenv("DCGAN_GAN_LOSS", raising=False)
    monkeypatch.delenv("DCGAN_LABEL_SMOOTH", raising=False)
    for e in (ReferenceEngine(SMALL, 2, CPU), HipEngine(SMALL, 2, CPU, dry_run=True, graph=False)):
        assert (e.gan_loss, e.label_smooth) == ("bce", 0.0)
    monkeypatch.setenv("DCGAN_GAN_LOSS", "lsgan")
    monkeypatch.setenv("DCGAN_LABEL_SMOOTH", "0.2")
    for e in (ReferenceEngine(SMALL, 2, CPU), build_engine(SMALL, 2, CPU, engine="reference"),
              HipEngine(SMALL, 2, CPU, dry_run=True, graph=False)):
        assert (e.gan_loss, e.label_smooth) == ("lsgan", 0.2)
    # an explicit argument wins, each on its own
    for e in (ReferenceEngine(SMALL, 2, CPU, gan_loss="bce", label_smooth=0.0),
              HipEngine(SMALL, 2, CPU, dry_run=True, graph=False, gan_loss="bce", label_smooth=0.0)):
        assert (e.gan_loss, e.label_smooth) == ("bce", 0.0)
    assert ReferenceEngine(SMALL, 2, CPU, label_smooth=0.1).label_smooth == 0.1
    monkeypatch.setenv("DCGAN_GAN_LOSS", "hinge")  # hinge from the environment + the smoothing from it: an error
    with pytest.raises(ValueError):
        ReferenceEngine(SMALL, 2, CPU)
    with pytest.raises(ValueError):
        HipEngine(SMALL, 2, CPU, dry_run=True, graph=False)
    assert HipEngine(SMALL, 2, CPU, dry_run=True, graph=False, label_smooth=0.0).gan_loss == "hinge"


# ------------------------------------------------------------------ 3. reference engine
def _real(B, cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=g) * 2 - 1


@pytest.mark.parametrize("kind,s", KINDS)
def test_reference_engine_gradients_are_autograd_of_the_oracle(kind, s):
    eng = ReferenceEngine(SMALL, 4, CPU, seed=3, gan_loss=kind, label_smooth=s)
    assert (eng.gan_loss, eng.label_smooth) == (kind, s)
    real = _real(4, SMALL)
    z = torch.rand(4, SMALL.z_dim, generator=torch.Generator().manual_seed(1)) * 2 - 1
    m = eng.model
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in m.g.tensors.items()}
    Pd = {k: v.detach().clone().requires_grad_(True) for k, v in m.d.tensors.items()}
    fake = m.generator(z, train=True, P=Pg, update_ema=False)
    _, logits = m.discriminator(torch.cat([real, fake], 0), groups=2, slots=(0, 1), train=True, P=Pd, update_ema=False)
    dr, df, gl, dl = R.gan_losses(logits[:4], logits[4:], kind, s)
    out, gd, gg = eng.step_impl.compute_grads(real, z, update_ema=False)
    assert torch.equal(out["d_loss"], dl) and torch.equal(out["g_loss"], gl)
    assert torch.equal(out["d_loss_real"], dr) and torch.equal(out["d_loss_fake"], df)
    exp_d = torch.autograd.grad(dl, [Pd[n] for n in m.d.names()], retain_graph=True)
    exp_g = torch.autograd.grad(gl, [Pg[n] for n in m.g.names()])
    got_d, got_g = m.d.like(), m.g.like()
    got_d.flat.copy_(gd)
    got_g.flat.copy_(gg)
    for n, e in zip(m.d.names(), exp_d):
        assert torch.equal(got_d[n], e), n
    for n, e in zip(m.g.names(), exp_g):
        assert torch.equal(got_g[n], e), n
    assert float(gd.abs().max()) > 0 and float(gg.abs().max()) > 0
    eng.set_batch(real)
    eng.train_step()  # the step itself runs and reports the four losses
    assert set(eng.last_losses()) == {"d_loss_real", "d_loss_fake", "g_loss", "d_loss"}
    assert all(math.isfinite(v) for v in eng.last_losses().values())


def test_reference_engine_default_is_todays_engine(monkeypatch):
    monkeypatch.delenv("DCGAN_GAN_LOSS", raising=False)
    monkeypatch.delenv("DCGAN_LABEL_SMOOTH", raising=False)
    a = ReferenceEngine(SMALL, 4, CPU, seed=3)
    b = ReferenceEngine(SMALL, 4, CPU, seed=3, gan_loss="bce", label_smooth=0.0)
    c = ReferenceEngine(SMALL, 4, CPU, seed=3, gan_loss="lsgan")
    for e in (a, b, c):
        e.set_batch(_real(4, SMALL))
        e.train_step()
    assert a.last_losses() == b.last_losses()
    assert torch.equal(a.model.g.flat, b.model.g.flat) and torch.equal(a.model.d.flat, b.model.d.flat)
    # today's losses, spelled out: the reference's three sigmoid cross-entropies
    lr_, lf = a.step_impl.last["logits_real"], a.step_impl.last["logits_fake"]
    sce = R.sigmoid_cross_entropy_with_logits
    assert torch.equal(a.step_impl.last["d_loss_real"], sce(lr_, torch.ones_like(lr_)).mean())
    assert torch.equal(a.step_impl.last["g_loss"], sce(lf, torch.ones_like(lf)).mean())
    assert not torch.equal(a.model.d.flat, c.model.d.flat)


# ------------------------------------------------------------------ 4. schedules (dry-run HIP engines)
@pytest.mark.parametrize("kind,s", [("hinge", 0.0), ("lsgan", 0.1)])
@pytest.mark.parametrize("case", list(enumerate(CASES)))
def test_schedules_with_objectives_have_no_stream_hazards(case, kind, s, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    k, (world, schedule, timing) = case
    dtype = ("bf16", "fp16", "fp32")[k % 3]  # one dtype per case: the ops and byte ranges do not depend on the objective
    sched, hz, n = SC.check(DCGANConfig(), 4, dtype, world, schedule, timing, gan_loss=kind, label_smooth=s)
    assert sched == (schedule or ("fused" if world == 1 and not timing else "concurrent"))
    assert n > 100
    assert hz == [], "\n".join(map(str, hz[:10]))


def test_objective_changes_no_op_and_no_byte_range():
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine

    def ops(**kw):
        eng = HipEngine(SMALL, 4, CPU, dry_run=True, graph=False, **kw)
        return eng, [(eng.progA.op_info(i)[0], eng.progA.op_info(i)[1], [tuple(a[1:]) for a in eng.progA.op_info(i)[4]])
                     for i in range(eng.progA.size())]
    base, o0 = ops()
    for kw in (dict(gan_loss="hinge"), dict(gan_loss="lsgan", label_smooth=0.1), dict(gan_loss="bce", label_smooth=0.2)):
        eng, o = ops(**kw)
        assert o == o0 and eng.kernel_count() == base.kernel_count()
        assert eng.gan_loss == kw["gan_loss"] and eng.label_smooth == kw.get("label_smooth", 0.0)


# ------------------------------------------------------------------ 5. command line
def test_cli_trains_with_lsgan_and_label_smoothing(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--synthetic", "--output_size=28", "--c_dim=1", "--batch_size=4", "--device=cpu", "--engine=reference",
              "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
              "--save_summaries_secs=1000", "--sample_every=0"]

    def run(args):
        env = dict(os.environ, OMP_NUM_THREADS="4")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DCGAN_GAN_LOSS", "DCGAN_LABEL_SMOOTH"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(root, "image_train.py")] + common + args, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout

    rc, out = run(["--max_steps=3", "--gan_loss=lsgan", "--label_smooth=0.1"])
    assert rc == 0, out
    assert "'gan_loss': 'lsgan'" in out and "'label_smooth': 0.1" in out
    assert out.count("GAN objective: lsgan, label_smooth 0.1") == 1
    rc, out = run(["--gan_loss=hinge", "--label_smooth=0.1"])
    assert rc != 0 and "label_smooth" in out
