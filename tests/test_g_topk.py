"""Top-k generator updates (--g_topk / --g_topk_steps), CPU side: the oracle of ops/reference.py (keys,
ranks, k(t), kmin, the seed and the loss), validation and precedence, ``ReferenceStep`` with top-k against
a hand-written autograd step, the dry-run HIP schedules (hazards, where ``g_topk`` sits and what it reads
and writes, a planted race), the trainer and the CLI."""
import glob
import io
import math
import os
import subprocess
import sys

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
TOPK_ENV = ("DCGAN_G_TOPK", "DCGAN_G_TOPK_STEPS")
ENV = TOPK_ENV + ("DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS", "DCGAN_D_AUGMENT",
                  "DCGAN_D_COLOR_AUGMENT", "DCGAN_LR_DECAY", "DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G",
                  "DCGAN_DDP_SHARD", "DCGAN_DDP_SCHEDULE", "DCGAN_SERIAL_DBWD", "DCGAN_D_SPECTRAL_NORM",
                  "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS", "DCGAN_D_UPDATE")
KINDS = ("bce", "lsgan", "hinge")
ON = dict(g_topk=0.5, g_topk_steps=10)


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


# ------------------------------------------------------------------ 1. the oracle
def test_known_answers():
    kmin = R.topk_kmin(128, 0.5)
    assert kmin == 64
    assert [R.topk_k(t, 128, kmin, 1000) for t in (0, 500, 999, 1000, 1001, 10 ** 9)] == [128, 96, 65, 64, 64, 64]
    x = torch.tensor([0.5, -1, 0.5, 2, -0.0, +0.0])
    sel = lambda k: set(R.topk_select(x, k).nonzero().flatten().tolist())  # noqa: E731
    assert sel(2) == {3, 0} and sel(3) == {3, 0, 2} and sel(4) == {3, 0, 2, 5}  # (+0 ranks above -0)
    assert sel(5) == {3, 0, 2, 5, 4} and sel(1) == {3}
    assert R.topk_rank(x).tolist() == [1, 5, 2, 0, 4, 3]
    assert float(R.topk_threshold(x, 2)) == 0.5 and float(R.topk_threshold(x, 6)) == -1.0
    assert math.copysign(1.0, float(R.topk_threshold(x, 5))) == -1.0  # the -0 itself
    for bad in (0, 7):
        with pytest.raises(ValueError):
            R.topk_select(x, bad)


def test_keys_are_monotone_and_order_the_specials():
    nan = float("nan")
    neg_nan = torch.tensor([-1], dtype=torch.int32).view(torch.float32)  # 0xFFFFFFFF: a NaN with the sign bit
    x = torch.cat([neg_nan, torch.tensor([-math.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.5, math.inf, nan])])
    key = R.topk_keys(x)
    assert key.tolist() == sorted(key.tolist()) and len(set(key.tolist())) == x.numel()
    assert int(key.min()) == 0 and int(key.max()) < 2 ** 32
    g = torch.Generator().manual_seed(0)
    v = torch.randn(4096, generator=g) * 10
    assert torch.equal(torch.argsort(R.topk_keys(v)), torch.argsort(v.double()))  # (no ties: the same order)


@pytest.mark.parametrize("B", [1, 2, 5, 64, 257])
def test_select_against_topk_and_a_stable_sort(B):
    g = torch.Generator().manual_seed(B)
    for x in (torch.randn(B, generator=g), torch.randint(0, 3, (B,), generator=g).float(), torch.full((B,), 1.5)):
        order = torch.sort(x, descending=True, stable=True).indices
        for k in sorted({1, max(1, B // 2), max(1, B - 1), B}):
            sel = R.topk_select(x, k)
            want = torch.zeros(B, dtype=torch.bool)
            want[order[:k]] = True
            assert torch.equal(sel, want) and int(sel.sum()) == k
            if x.unique().numel() == B:  # no ties: torch.topk names the same set
                assert set(torch.topk(x, k).indices.tolist()) == set(sel.nonzero().flatten().tolist())
            assert float(R.topk_threshold(x, k)) == float(x[order[k - 1]])


def test_exactly_k_whatever_the_input():
    nan, inf = float("nan"), float("inf")
    inputs = [torch.full((9,), -2.0), torch.tensor([0.0, -0.0] * 5), torch.tensor([inf, -inf, inf, 1.0, -inf]),
              torch.tensor([nan] * 6), torch.tensor([nan, 1.0, inf, -inf, nan, -0.0, 0.0])]
    for x in inputs:
        for k in range(1, x.numel() + 1):
            sel = R.topk_select(x, k)
            assert int(sel.sum()) == k
            assert bool((sel | ~R.topk_select(x, max(1, k - 1))).all())  # nested: k - 1's selection stays
    assert R.topk_select(inputs[0], 3).nonzero().flatten().tolist() == [0, 1, 2]  # ties: the lower index wins
    assert R.topk_select(inputs[1], 5).nonzero().flatten().tolist() == [0, 2, 4, 6, 8]  # every +0 above every -0
    assert R.topk_select(inputs[4], 3).nonzero().flatten().tolist() == [0, 2, 4]  # NaN (positive bits) above +inf


@pytest.mark.parametrize("B,nu,steps", [(128, 0.5, 1000), (8, 0.5, 4), (4096, 1e-6, 1 << 24), (1000, 0.1, 7), (5, 1.0, 3),
                                        (1, 0.5, 9), (7, 0.75, 1)])
def test_k_of_t_against_big_integers(B, nu, steps):
    kmin = R.topk_kmin(B, nu)
    ts = sorted({0, 1, 2, steps // 3, steps // 2, steps - 1, steps, steps + 1, 1 << 32, 1 << 40} | set(range(0, min(steps, 50))))
    ks = []
    for t in ts:
        tt = t if t < steps else steps
        want = B - ((B - kmin) * tt) // steps  # Python integers: no overflow
        assert R.topk_k(t, B, kmin, steps) == want
        ks.append(want)
    assert ks[0] == B and ks == sorted(ks, reverse=True)
    assert all(k == kmin for t, k in zip(ts, ks) if t >= steps) and R.topk_k(1 << 40, B, kmin, steps) == kmin
    with pytest.raises(ValueError):
        R.topk_k(0, B, B + 1, steps)
    with pytest.raises(ValueError):
        R.topk_k(0, B, kmin, 0)


def test_kmin():
    want = {(1, 1.0): 1, (1, 0.75): 1, (1, 0.5): 1, (1, 0.1): 1, (1, 1e-6): 1,
            (8, 1.0): 8, (8, 0.75): 6, (8, 0.5): 4, (8, 0.1): 1, (8, 0.125): 1, (8, 1e-6): 1,
            (128, 1.0): 128, (128, 0.75): 96, (128, 0.5): 64, (128, 0.1): 13, (128, 1 / 128): 1, (128, 1e-6): 1}
    for (B, nu), k in want.items():
        assert R.topk_kmin(B, nu) == k, (B, nu)
    assert R.topk_kmin(1, 1 / 1) == 1 and R.topk_kmin(8, 1 / 8) == 1
    assert R.topk_kmin(10, 0.3) == 3  # 10 * 0.3 = 3.0000000000000004: the 1e-9 keeps it at 3
    with pytest.raises(ValueError):
        R.topk_kmin(0, 0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_the_seed_is_the_gradient_of_the_mean_over_the_selected(kind):
    B, ls = 16, 512.0
    x = 3 * torch.randn(B, generator=torch.Generator().manual_seed(7))
    xr = torch.randn(B, generator=torch.Generator().manual_seed(8))
    xa = x.double().requires_grad_(True)
    R.gan_losses(xr.double(), xa, kind)[2].backward()
    dl_g = (xa.grad * ls).float()  # the all-sample seed, with a loss scale: g'(x_i) * ls / B
    for k in (1, 5, 8, 16):
        sel = R.topk_select(x, k)
        seed = R.topk_seed(dl_g, sel, B, k)
        xf = x.double().requires_grad_(True)
        loss = R.topk_g_loss(xf, sel, kind)
        loss.backward()
        assert torch.allclose(seed.double(), xf.grad * ls, rtol=1e-6, atol=1e-9)
        assert float(seed.sum()) == pytest.approx(float(xf.grad.sum()) * ls, rel=1e-5, abs=1e-6)
        assert not bool(seed[~sel].view(torch.int32).ne(0).any())  # +0, sign bit clear
        assert torch.equal(seed[sel], dl_g[sel] * (torch.tensor(float(B)) / torch.tensor(float(k))))
        l32 = R.topk_g_loss(x, sel, kind)
        assert l32.dtype == torch.float32 and float(l32) == pytest.approx(float(loss.detach()), rel=1e-5, abs=1e-6)
    assert float(R.topk_g_loss(x.double(), torch.ones(B, dtype=torch.bool), kind)) == \
        pytest.approx(float(R.gan_losses(xr.double(), x.double(), kind)[2]), rel=1e-12)
    # label smoothing never touches G's target: the bce term is target 1
    if kind == "bce":
        assert float(R.gan_losses(xr, x, "bce", 0.2)[2]) == float(R.gan_losses(xr, x, "bce", 0.0)[2])


# ------------------------------------------------------------------ 2. validation, precedence
BAD = [("g_topk", 0.0), ("g_topk", -0.5), ("g_topk", 1.5), ("g_topk", float("nan")), ("g_topk", float("inf")),
       ("g_topk_steps", 0), ("g_topk_steps", -3), ("g_topk_steps", 2 ** 24 + 1)]


@pytest.mark.parametrize("name,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_invalid_values_are_rejected_everywhere(name, value, monkeypatch, capsys):
    kw = dict(g_topk=0.5, g_topk_steps=10)
    kw[name] = value
    with pytest.raises(ValueError, match=name):
        R.check_g_topk(kw["g_topk"], kw["g_topk_steps"])
    with pytest.raises(ValueError, match=name):
        ReferenceStep(DCGAN(small(), seed=0), **kw)
    with pytest.raises(ValueError, match=name):
        ReferenceEngine(small(), 4, CPU, **kw)
    with pytest.raises(ValueError, match=name):
        _hip(**kw)
    with pytest.raises(ValueError, match=name):
        build_engine(small(), 4, CPU, engine="reference", **kw)
    if (name, value) != ("g_topk_steps", 0):  # (0 on the command line: until the end of training)
        with pytest.raises(SystemExit):
            F.parse_flags(["--%s=%s" % (k, v) for k, v in kw.items()])
        assert name in capsys.readouterr().err
    for k, v in zip(TOPK_ENV, (kw["g_topk"], kw["g_topk_steps"])):
        monkeypatch.setenv(k, str(v))
    with pytest.raises(ValueError, match=name):
        ReferenceEngine(small(), 4, CPU)
    with pytest.raises(ValueError, match=name):
        _hip()


def test_the_bindings_validate_on_their_own():
    """(A dry Program: records only.) Null or aliasing buffers and bad schedules throw at record time."""
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    ok = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 16, 8, 10, 0x6000, 0]
    assert prog.g_topk("t", *ok) == 0
    name, slot, kind, ev, acc = prog.op_info(0)
    assert (name, slot) == ("t", 0)
    assert sorted(acc) == [(0x1000, 64, False), (0x2000, 64, False), (0x3000, 64, True), (0x4000, 64, True),
                           (0x5000, 16, True), (0x6000, 8, False)]
    assert H.ext().Program(2, True).g_topk("t", *ok, 1) == 0  # (every element build; a stream slot)
    for i in (0, 1, 2, 3, 4, 8):
        bad = list(ok)
        bad[i] = 0
        with pytest.raises(RuntimeError, match="non-null"):
            prog.g_topk("t", *bad)
    for i, v in ((2, 0x2000), (2, 0x1000), (3, 0x3000), (4, 0x3000 + 60), (2, 0x6000 - 60), (3, 0x5000)):
        bad = list(ok)
        bad[i] = v
        with pytest.raises(RuntimeError, match="of their own"):
            prog.g_topk("t", *bad)
    for B, kmin, steps, obj in ((0, 1, 10, 0), (4097, 8, 10, 0), (16, 0, 10, 0), (16, 17, 10, 0), (16, 8, 0, 0),
                                (16, 8, 2 ** 24 + 1, 0), (16, 8, 10, 3), (16, 8, 10, -1)):
        bad = list(ok)
        bad[5], bad[6], bad[7], bad[9] = B, kmin, steps, obj
        with pytest.raises(RuntimeError, match="g_topk"):
            prog.g_topk("t", *bad)
        if obj == 0:
            with pytest.raises(RuntimeError, match="topk_k"):
                prog.topk_k("k", 0x1000, 0x2000, 4, B, kmin, steps)
    assert prog.size() == 1
    assert prog.g_topk("t", 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 4096, 1, 2 ** 24, 0x60000, 2) == 1  # the limits
    with pytest.raises(RuntimeError, match="non-null"):
        prog.topk_k("k", 0, 0x2000, 4, 16, 8, 10)
    assert prog.topk_k("k", 0x1000, 0x2000, 4, 16, 8, 10) == 2
    assert sorted(prog.op_info(2)[4]) == [(0x1000, 32, False), (0x2000, 16, True)]


def test_an_explicit_argument_wins_over_the_environment(monkeypatch):
    for k, v in zip(TOPK_ENV, ("0.25", "50")):
        monkeypatch.setenv(k, v)
    assert R.resolve_g_topk() == R.GTopK(0.25, 50)
    for mk in (lambda **kw: ReferenceEngine(small(), 4, CPU, **kw), lambda **kw: _hip(**kw)):
        assert mk().topk == R.GTopK(0.25, 50)
        assert mk(g_topk=0.5, g_topk_steps=9).topk == R.GTopK(0.5, 9)
        assert mk(g_topk_steps=7).topk == R.GTopK(0.25, 7)
        assert not mk(g_topk=1.0).topk.active
    monkeypatch.setenv("DCGAN_G_TOPK", "half")
    with pytest.raises(ValueError, match="DCGAN_G_TOPK"):
        R.resolve_g_topk()
    for k in TOPK_ENV:
        monkeypatch.delenv(k)
    assert R.resolve_g_topk() == R.GTopK() and not _hip().topk.active and _hip().dl_g_k is None
    assert R.GTopK().describe() == "off" and R.GTopK(0.5, 9).describe() == "k from B to ceil(0.5 B) over 9 steps"
    assert R.resolve_g_topk(R.GTopK(0.5, 9)) == R.GTopK(0.5, 9)
    assert R.check_g_topk(1.0, 12345) == R.GTopK(1.0, 1)  # off: steps is not read
    with pytest.raises(ValueError, match="g_topk"):
        _hip(DCGANConfig(output_size=28, c_dim=1), g_topk="many")


def test_open_ended_length_resolves_to_the_end_of_training():
    assert R.check_g_topk(0.5, 0, total_steps=50).steps == 50
    assert R.check_g_topk(0.5, 7, total_steps=50).steps == 7  # an explicit length stays
    for total in (0, -2, 2 ** 24 + 1):
        with pytest.raises(ValueError, match="g_topk_steps"):
            R.check_g_topk(0.5, 0, total_steps=total)
    with pytest.raises(ValueError, match="g_topk_steps"):
        R.check_g_topk(0.5, 0)
    assert R.check_g_topk(0.5, 0, open_ended=True).steps == 0
    fl = F.parse_flags([])
    assert (fl.g_topk, fl.g_topk_steps) == (1.0, 0)
    fl = F.parse_flags(["--g_topk=0.5"])
    assert (fl.g_topk, fl.g_topk_steps) == (0.5, 0)


# ------------------------------------------------------------------ 3. ReferenceStep
def _hand_step(model, real, z, kind, sel):
    """d_loss, g_loss over all B, and their gradients by plain autograd -- G's of the mean over `sel`."""
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in model.g.tensors.items()}
    Pd = {k: v.detach().clone().requires_grad_(True) for k, v in model.d.tensors.items()}
    fake = model.generator(z, train=True, P=Pg, update_ema=False)
    _, logits = model.discriminator(torch.cat([real, fake], 0), groups=2, slots=(0, 1), train=True, P=Pd,
                                    update_ema=False)
    B = real.shape[0]
    _, _, g_loss, d_loss = R.gan_losses(logits[:B], logits[B:], kind, 0.0)
    xf = logits[B:]
    if sel is None:
        g_obj = g_loss
    else:
        idx = sel.nonzero().flatten()
        term = {"bce": lambda v: R.sigmoid_cross_entropy_with_logits(v, torch.ones_like(v)),
                "lsgan": lambda v: 0.5 * (v - 1.0) ** 2, "hinge": lambda v: -v}[kind]
        g_obj = term(xf[idx]).sum() / idx.numel()
    dn, gn = model.d.names(), model.g.names()
    gd = torch.autograd.grad(d_loss, [Pd[n] for n in dn], retain_graph=True, allow_unused=True)
    gg = torch.autograd.grad(g_obj, [Pg[n] for n in gn], allow_unused=True)
    return d_loss, g_loss, g_obj, xf.detach(), dict(zip(dn, gd)), dict(zip(gn, gg))


def _flat_grads(ps, grads):
    out = ps.like()
    for n, g in grads.items():
        if g is not None:
            out[n].copy_(g)
    return out.flat


@pytest.mark.parametrize("kind", KINDS)
def test_reference_step_with_topk_is_autograd_on_the_selected(kind):
    cfg, B = small(), 8
    st = ReferenceStep(DCGAN(cfg, seed=3), gan_loss=kind, g_topk=0.5, g_topk_steps=4)
    plain = ReferenceStep(DCGAN(cfg, seed=3), gan_loss=kind)
    assert st.topk == R.GTopK(0.5, 4) and st.topk_k(B) == 8 and plain.topk_k(B) == 8
    st.global_step = plain.global_step = 2
    assert st.topk_k(B) == 6
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    _, _, _, xf, _, _ = _hand_step(st.model, real, z, kind, None)
    sel = R.topk_select(xf, 6)
    d_loss, g_loss, g_obj, _, gd, gg = _hand_step(st.model, real, z, kind, sel)
    out, fd, fg = st.compute_grads(real, z, update_ema=False)
    assert torch.equal(out["topk_sel"], sel) and int(out["topk_sel"].sum()) == 6
    assert float(out["d_loss"].detach()) == float(d_loss.detach()) and float(out["g_loss"].detach()) == float(g_loss.detach())
    assert float(out["g_loss_topk"].detach()) == float(g_obj.detach()) != float(g_loss.detach())
    assert torch.equal(fd, _flat_grads(st.model.d, gd)) and torch.equal(fg, _flat_grads(st.model.g, gg))
    # D's side and the reported g_loss are those of the step without top-k; G's gradient is not
    out0, fd0, fg0 = plain.compute_grads(real, z, update_ema=False)
    assert torch.equal(fd, fd0) and float(out0["g_loss"].detach()) == float(g_loss.detach())
    assert out0["topk_sel"] is None and out0["g_loss_topk"] is out0["g_loss"] and not torch.equal(fg, fg0)
    # a passed-in mask is honoured; False = none
    other = torch.zeros(B, dtype=torch.bool)
    other[[1, 4, 6]] = True
    _, _, g_other, _, _, gg_o = _hand_step(st.model, real, z, kind, other)
    out2, fd2, fg2 = st.compute_grads(real, z, update_ema=False, topk=other)
    assert torch.equal(out2["topk_sel"], other) and float(out2["g_loss_topk"].detach()) == float(g_other.detach())
    assert torch.equal(fd2, fd) and torch.equal(fg2, _flat_grads(st.model.g, gg_o))
    out3, _, fg3 = st.compute_grads(real, z, update_ema=False, topk=False)
    assert out3["topk_sel"] is None and torch.equal(fg3, fg0)
    # the step reports the all-sample g_loss, the sub-step selects nothing
    got = st.step(real, z)
    assert got["g_loss"] == float(g_loss.detach()) and st.global_step == 3 and sorted(got) == sorted(plain.step(real, z))
    st.d_step(real, z)
    assert st.last["topk_sel"] is None


def _run_steps(n=3, d_steps=2, **kw):
    cfg, B = small(), 4
    st = ReferenceStep(DCGAN(cfg, seed=3), d_steps=d_steps, **kw)
    losses = []
    for step in range(n):
        for k in range(d_steps - 1):
            losses.append(st.d_step(_real(B, cfg, 10 * step + k), _z(B, cfg, 100 * step + k)))
        losses.append(st.step(_real(B, cfg, 10 * step + 9), _z(B, cfg, 100 * step + 9)))
    return losses, st.model.d.flat.clone(), st.model.g.flat.clone()


def test_nu_one_is_bitwise_the_step_without_it():
    plain = _run_steps()
    off = _run_steps(g_topk=1.0, g_topk_steps=5)
    assert off[0] == plain[0] and torch.equal(off[1], plain[1]) and torch.equal(off[2], plain[2])
    on = _run_steps(g_topk=0.5, g_topk_steps=2)
    assert on[0][:2] == plain[0][:2]  # k(0) = B: the first cycle's losses are the same
    assert not torch.equal(on[2], plain[2]) and not torch.equal(on[1], plain[1])


def test_reference_engine_reports_the_selection_and_clean_eval_losses():
    cfg, B = small(), 8
    e = ReferenceEngine(cfg, B, CPU, seed=3, g_topk=0.5, g_topk_steps=2)
    plain = ReferenceEngine(cfg, B, CPU, seed=3)
    assert plain.last_topk() is None and plain.topk_selection() is None
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    assert e.eval_losses(real, z) == plain.eval_losses(real, z)
    e.set_synthetic_batch(real)
    ks = []
    for _ in range(3):
        e.train_step()
        k, g, thr = e.last_topk()
        sel = e.topk_selection()
        x = e.step_impl.last["logits_fake"].detach()
        assert int(sel.sum()) == k and torch.equal(sel, R.topk_select(x, k)) and thr == float(x[sel].min())
        assert g == pytest.approx(float(R.topk_g_loss(x, sel, "bce")))
        ks.append(k)
    assert ks == [8, 6, 4]


# ------------------------------------------------------------------ 4. schedules (dry-run HIP engines)
CASES = [(1, None, "fp32", 1), (1, None, "fp32", 2), (1, "serial", "fp32", 1)]
for _w in (2, 4, 8):
    for _wire in ("fp32", "bf16"):
        CASES += [(_w, None, _wire, 1), (_w, None, _wire, 2), (_w, "ddp", _wire, 1), (_w, "serial", _wire, 1)]
OTHERS = dict(instance_noise=0.2, instance_noise_end=0.05, instance_noise_steps=10, d_augment="translation,cutout",
              d_color_augment="brightness,saturation,contrast")


def _record(eng, steps=1):
    ex = SC.RecordingExec(eng.ext)
    eng._ensure_comm()
    for s in range(steps):
        ex.step = s
        eng._run_step(ex)
    return ex


def _name(op):
    return op.label.split(":", 1)[1]


def _check_topk_op(eng):
    """One g_topk per step, none in a D sub-step: the first op behind the forward, on the stream of the g_loss
    chain it seeds; it reads the fake logits, dl_g and the 8-byte counter and writes buffers of its own."""
    B = eng.B
    names = eng.op_names()
    assert names.count("g_topk") == 1 and names[eng._a_fwd] == "g_topk"
    assert all("g_topk" not in eng.sub_op_names(k) for k in range(eng.d_steps - 1))
    ex = _record(eng)
    idx = [i for i, op in enumerate(ex.ops) if _name(op) == "g_topk"]
    assert len(idx) == 1
    op = ex.ops[idx[0]]
    assert sorted(op.acc) == sorted([(eng.logits.data_ptr() + 4 * B, 4 * B, False), (eng.dl_g.data_ptr(), 4 * B, False),
                                     (eng.step_counter.data_ptr(), 8, False), (eng.dl_g_k.data_ptr(), 4 * B, True),
                                     (eng.topk_sel.data_ptr(), 4 * B, True), (eng.topk_info.data_ptr(), 16, True)])
    # the head op (the writer of the logits and of dl_g) is ordered before it; the g_loss chain reads its seed,
    # on its stream, and nothing reads the all-sample dl_g but g_topk
    writers = [o for o in ex.ops[:idx[0]] if any(w and a == eng.dl_g.data_ptr() for a, _, w in o.acc)]
    head = writers[-1]  # (the D sub-steps' heads write dl_g too, ahead of the full step's)
    assert len(writers) == eng.d_steps and head.vc[head.stream] <= op.vc.get(head.stream, 0)
    seed_readers = [o for o in ex.ops if any(not w and a == eng.dl_g_k.data_ptr() for a, _, w in o.acc)]
    assert seed_readers and all(_name(o).startswith("g.") and o.stream == op.stream for o in seed_readers)
    nxt = [o for o in ex.ops[idx[0] + 1:] if o.stream == op.stream][0]
    assert nxt in seed_readers, _name(nxt)
    assert [_name(o) for o in ex.ops if any(not w and a == eng.dl_g.data_ptr() for a, _, w in o.acc)] == ["g_topk"]
    # the D chain does not wait for it: its ops are not ordered behind g_topk
    if eng._schedule() == "fused":
        d_chain = [o for o in ex.ops if o.stream.startswith("alt") and _name(o).startswith(("d", "head"))]
        assert d_chain and not any(op.vc[op.stream] <= o.vc.get(op.stream, 0) for o in d_chain[:3])
    # `losses` has no new writer
    lo = eng.losses.data_ptr()
    assert "g_topk" not in {_name(o) for o in ex.ops if any(w and lo <= a < lo + 16 for a, _, w in o.acc)}


@pytest.mark.parametrize("world,schedule,wire,d_steps", CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in CASES])
@pytest.mark.parametrize("others", [False, True], ids=["alone", "noise+aug+color"])
def test_schedules_are_hazard_free_with_the_topk_op(world, schedule, wire, d_steps, others):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **ON, **(OTHERS if others else {}))
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_topk_op(eng)


@pytest.mark.parametrize("dtype,size,c_dim,kw", [("fp16", 28, 1, dict(gan_loss="hinge")), ("fp32", 28, 1, dict(gan_loss="lsgan")),
                                                 ("fp32", 64, 3, dict(d_spectral_norm=True)),
                                                 ("bf16", 64, 3, dict(g_ema_decay=0.999, gan_loss="bce", label_smooth=0.1)),
                                                 ("bf16", 128, 3, dict())])
@pytest.mark.parametrize("d_steps", [1, 3])
def test_other_dtypes_sizes_and_switches_are_hazard_free(dtype, size, c_dim, kw, d_steps):
    for world in (1, 2):
        eng = _hip(DCGANConfig(output_size=size, c_dim=c_dim), dtype=dtype, world=world, d_steps=d_steps, **ON, **kw)
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))
        _check_topk_op(eng)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free_with_the_topk_op(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    for others in ({}, OTHERS):
        eng = _hip(world=world, **ON, **others)
        assert eng._sharded()
        hz, n = SC.check_engine(eng)
        assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
        _check_topk_op(eng)


def test_checker_finds_g_topk_moved_ahead_of_the_head_op():
    """The fused step with g_topk issued on a stream of its own BEFORE the head op (the writer of the logits
    and of dl_g), with nothing ordering the two. Only the accesses to the logits, dl_g and the top-k buffers
    are kept, so those alone decide."""
    def planted(eng):
        head = max(i for i in range(eng._a_fwd)
                   if any(w and a == eng.dl_g.data_ptr() for a, _, w in eng.progA.op_info(i)[4]))
        topk = eng.topk.active

        def bad_fused(ex, cs):
            ex.run(eng.progA, [cs, ex.side], 0, head)
            if topk:
                ex.wait(ex.alt[1], cs)
                ex.run(eng.progA, [ex.alt[1], ex.side], eng._a_fwd, eng._a_fwd + 1)
            ex.run(eng.progA, [cs, ex.side], head, eng._a_fwd)
            ex.wait(ex.alt[0], cs)
            ex.run(eng.progB, ex.alt)
            if topk:
                ex.wait(cs, ex.alt[1])
            ex.run(eng.progA, [cs, ex.side], eng._a_fwd + (1 if topk else 0), -1)
            ex.run(eng.progW, [cs, ex.side])
            ex.wait(cs, ex.alt[0])
            ex.run(eng.progC, [cs, ex.side])
        eng._run_fused = bad_fused
        ex = _record(eng, steps=2)
        keep = [(t.data_ptr(), t.data_ptr() + t.numel() * 4) for t in
                (eng.logits, eng.dl_g, eng.dl_g_k, eng.topk_sel, eng.topk_info) if t is not None]
        for op in ex.ops:
            op.acc = [a for a in op.acc if any(lo <= a[0] < hi for lo, hi in keep)]
        return SC.find_hazards(ex.ops)
    eng = _hip(**ON)
    assert SC.check_engine(eng)[0] == []
    hz = planted(eng)
    assert hz and all("g_topk" in h.a + h.b for h in hz), "\n".join(map(str, hz))
    # (one report per pair of ops, at the lowest range they share: the fake logits or dl_g)
    assert all(h.addr in (eng.dl_g.data_ptr(), eng.logits.data_ptr() + 16) and "head" in h.a + h.b for h in hz)
    assert planted(_hip()) == []


def test_with_the_switch_off_the_recorded_ops_are_todays():
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16"),
               dict(dtype="fp32"), OTHERS):
        off = _hip(g_topk=1.0, g_topk_steps=77, **kw)
        bare = _hip(**kw)
        assert off.dl_g_k is None and bare.dl_g_k is None and off.topk_sel is None and off.topk_info is None
        assert off.op_names() == bare.op_names() and "g_topk" not in bare.op_names()
        assert off.kernel_count() == bare.kernel_count()
        a, b = _record(off), _record(bare)
        assert [(_name(x), x.stream, len(x.acc)) for x in a.ops] == [(_name(x), x.stream, len(x.acc)) for x in b.ops]
        on = _hip(**ON, **kw)
        assert on.kernel_count() == bare.kernel_count() + 1
        assert [n for n in on.op_names() if n != "g_topk"] == bare.op_names()
        assert [on.sub_op_names(k) for k in range(on.d_steps - 1)] == [bare.sub_op_names(k) for k in range(bare.d_steps - 1)]


def test_engine_refuses_a_batch_beyond_the_kernels_limit():
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    with pytest.raises(ValueError, match="g_topk needs batch_size"):
        HipEngine(small(), R.TOPK_MAX_B + 1, CPU, dry_run=True, graph=False, **ON)


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
    fl = _train_flags(tmp_path, "--g_topk=0.5", "--max_steps=100", "--epoch=1")
    assert T.run(fl, out=out) == 0
    assert (built[-1]["g_topk"], built[-1]["g_topk_steps"]) == (0.5, 8)
    assert "top-k generator updates: k from B to ceil(0.5 B) over 8 steps" in out.getvalue()
    out = io.StringIO()
    fl = _train_flags(tmp_path / "b", "--g_topk=0.5", "--g_topk_steps=3", "--max_steps=1", "--epoch=0")
    assert T.run(fl, out=out) == 0
    assert built[-1]["g_topk_steps"] == 3 and "over 3 steps" in out.getvalue()
    fl = _train_flags(tmp_path / "c", "--g_topk=0.5", "--max_steps=0", "--epoch=0")
    with pytest.raises(SystemExit, match="g_topk_steps"):
        T.run(fl, out=io.StringIO())
    out = io.StringIO()
    assert T.run(_train_flags(tmp_path / "d", "--max_steps=1", "--epoch=0"), out=out) == 0
    assert "top-k" not in out.getvalue() and built[-1]["g_topk"] == 1.0


def test_cli_runs_with_topk_and_logs_a_falling_k(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=4", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=8", "--sample_every=0", "--save_summaries_secs=0", "--epoch=0", "--g_topk=0.5",
            "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "top-k generator updates: k from B to ceil(0.5 B) over 4 steps" in p.stdout
    files = glob.glob(str(tmp_path / "ck" / "events.out.tfevents.*"))
    assert len(files) == 1
    seen = {"g_topk/k": {}, "g_topk/threshold": {}, "g_loss_topk": {}, "g_loss": {}}
    for ev in read_events(files[0]):
        for v in ev["values"]:
            if v.get("tag") in seen:
                seen[v["tag"]][ev["step"]] = v["simple_value"]
    # the event at step s reports the selection that step s - 1 -> s was taken with
    assert seen["g_topk/k"] == {1: 8.0, 2: 7.0, 3: 6.0, 4: 5.0}
    assert sorted(seen["g_topk/threshold"]) == sorted(seen["g_loss_topk"]) == [1, 2, 3, 4]
    assert all(math.isfinite(v) for tag in seen for v in seen[tag].values())
    if seen["g_loss"]:  # the all-sample loss stays in the log; at k = B the two agree
        assert seen["g_loss_topk"][1] == pytest.approx(seen["g_loss"][1], rel=1e-5)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--g_topk=0"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "g_topk" in bad.stdout
