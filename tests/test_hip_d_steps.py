"""GPU tests of the D-only sub-steps (``d_steps`` > 1), ``beta2`` and the per-network learning rates
of the HIP engine: the sub-step's update kernels (adam1 = Adam + mirror + D's powers in one launch;
step_end as the sub-step records it, without G's powers and the step), a sub-step and whole cycles
against ``ReferenceStep`` (bf16 / fp16 / fp32), the z of the sub-steps, hipGraph replay, the fp16 overflow sub-step, one-rank RCCL DDP, checkpoint resume through
the trainer, and that the defaults change nothing.

Comparisons with the reference are those of ``test_step_matches_reference`` in
test_hip_d_spectral_norm.py (``check_piece`` of hip_harness.py repeats its tolerances):
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
import pytest
import torch

import hip_harness as HH
from hip_harness import BUILDS, H, PAD, dev
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

_padded, _canaries_intact = HH.padded, HH.intact
_engine, _reals, _ref_for, _check_piece, _copies_match_state = HH.engine, HH.reals, HH.ref_for, HH.check_piece, HH.copies_match_state
_g_state, _d_state, _snap = HH.g_state, HH.d_state, HH.snap
ENV = HH.ENV
_clean_env = HH.clean_env(ENV)


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
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_graph_replay_matches_eager(dtype):
    cfg = DCGANConfig(d_bn=False)
    e1 = _engine(cfg, 16, 3, dtype=dtype, seed=1, d_spectral_norm=True, g_ema_decay=0.999)
    e2 = _engine(cfg, 16, 3, dtype=dtype, seed=1, d_spectral_norm=True, g_ema_decay=0.999, graph=True)
    for _ in range(4):
        e1.train_step()
        e2.train_step()
        HH.snap_equal(e1, e2)
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
        HH.snap_equal(bare, dflt)
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
    _copies_match_state(eng)


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


def _sub_ops(eng):
    return {"ops": eng.sub_op_names(0), "sub_graphs": [len(g) for g in eng._sub_graphs]}


DDP = HH.Ddp(_ddp_engine, _result, STEPS, extras=_sub_ops)


@pytest.fixture(scope="module")
def fused_run():
    return HH.fused_result(DDP, ENV)


@pytest.mark.parametrize("graph", [False, True])
def test_rccl_single_rank_ddp_matches_fused(tmp_path, graph, fused_run):
    r = HH.rccl_run(tmp_path, DDP, "concurrent", graph, fused_run)
    assert "adam_d" in r["ops"] and "d_step_end" in r["ops"] and "adam_d1" not in r["ops"]
    assert r["sub_graphs"] == ([4] if graph else [])


# ------------------------------------------------------------------ checkpoint resume through the trainer
def test_trainer_resume_is_exact_with_d_steps(tmp_path, monkeypatch):
    """bf16, d_steps = 2: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more --
    every saved tensor bitwise (D's powers after 8 updates included), and no key beyond the
    default run's."""
    kw = dict(d_steps=2, beta2=0.9)
    r = HH.trainer_resume(tmp_path, monkeypatch, ["--d_steps=2", "--beta2=0.9"], load_kw=kw)
    assert [m.i for m in r.made] == [8, 4, 4]  # two real batches per training step
    sa = r.a[1]
    assert float(sa["beta2_power"].reshape(-1)[0]) == pytest.approx(0.9 ** 9, rel=1e-5)
    assert float(sa["beta2_power_1"].reshape(-1)[0]) == pytest.approx(0.9 ** 5, rel=1e-5)
    r.run(tmp_path / "c", 1, ["--d_steps=1", "--beta2=0.9"])
    assert list(r.load(tmp_path / "c", d_steps=1, beta2=0.9)[1]) == list(sa)
