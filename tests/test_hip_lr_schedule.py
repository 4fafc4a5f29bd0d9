"""GPU tests of the learning-rate schedule the Adam kernels evaluate from the device step counter:
the factor probe against the fp64 closed form, scheduled Adam == plain Adam at lr * f (bitwise, every
Adam kernel), the zero step, a decay that has not started, the engine against ``ReferenceStep``
(the comparison and tolerances of test_hip_d_steps.py), hipGraph replay, one-rank RCCL DDP, resume
through the trainer and the bindings' argument checks.

Shapes: adam_ n = 4100 (float4 body + scalar tail, 5 blocks), adam1 / adam2 n = 2052 and 1028
(% 4 == 0, more than one block), canaries around every buffer; engines at 28x28x1, batch 8."""
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
_padded, _canaries_intact = SNT._padded, SNT._canaries_intact
ENV = TD.ENV + ("DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP")
KINDS = ("linear", "cosine", "exponential")
F32 = torch.float32


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def small():
    return DCGANConfig(output_size=28, c_dim=1)


# ------------------------------------------------------------------ 1. the factor probe
M = 1 << 24
# (start, steps, end, warmup); every `end` is an fp32 number, so fp32 and fp64 see the same schedule
PROBE = [(1000, 5000, 0.125, 300), (5, M, 2.0 ** -6, M), (M - 3, 7, 0.5, 0)]


def _grid(start, steps, warmup):
    t = {0, 1, 2, start - 1, start, start + 1, start + 2, start + steps // 3, start + steps // 2, start + steps - 1,
         start + steps, start + steps + 1, warmup - 2, warmup - 1, warmup, warmup + 1, warmup // 2,
         M - 2, M - 1, M, M + 1, M + 7, 2 * M + 5, (1 << 32) + 3, 1 << 40}
    t |= {start + (steps * i) // 97 for i in range(98)}
    return torch.tensor(sorted(x for x in t if x >= 0), dtype=torch.int64)


@pytest.mark.parametrize("kind", ("none",) + KINDS)
def test_factor_probe_matches_fp64(kind):
    """Bound: the device's largest absolute error over the grid <= 4 x the largest error of the fp32
    CPU oracle over the same grid, with a floor of 2^-22; the end points bitwise.

    Measured on an MI355X, largest absolute error over the three parameter sets, device / fp32
    oracle: none (warm-up only) 3.18e-9 / 3.18e-9, linear 3.71e-8 / 5.70e-8, cosine 6.77e-8 / 8.41e-8,
    exponential 3.84e-8 / 3.60e-8 (floor 2^-22 = 2.38e-7); per set: profiles/r11/lr_schedule_r11.txt."""
    h = H()
    worst_dev = worst_cpu = 0.0
    for start, steps, end, warmup in PROBE:
        s = R.check_lr_schedule(kind, start, steps, end, warmup)
        t = _grid(start, steps, warmup)
        buf, view = _padded(torch.zeros(t.numel()))
        tb, tv = _padded(t, fill=0)
        view.copy_(h.lr_factor(tv, s))
        got = h.lr_factor(t.to(dev), s).cpu()
        torch.cuda.synchronize()
        assert _canaries_intact(buf) and torch.equal(view.cpu(), got) and torch.equal(tv.cpu(), t)
        want = R.lr_factor(s, t, dtype=torch.float64)
        cpu = R.lr_factor(s, t)
        e_dev = float((got.double() - want).abs().max())
        e_cpu = float((cpu.double() - want).abs().max())
        print("lr_factor %-11s start %d steps %d end %g warmup %d: max abs error device %.3e, fp32 oracle %.3e"
              % (kind, start, steps, end, warmup, e_dev, e_cpu))
        worst_dev, worst_cpu = max(worst_dev, e_dev), max(worst_cpu, e_cpu)
        assert e_dev <= max(4 * e_cpu, 2.0 ** -22), (kind, start, steps, e_dev, e_cpu)
        # exact by selection: 1.0f up to `start`, `end` from start + steps on (outside the warm-up)
        out = t >= warmup
        if kind == "none":
            assert bool((got[out] == 1.0).all())
        else:
            assert bool((got[out & (t <= start)] == 1.0).all())
            assert bool((got[out & (t >= start + steps)] == torch.tensor(end, dtype=F32)).all())
            mid = out & (t > start) & (t < start + steps)
            assert bool((got[mid] <= 1.0).all())
        if warmup:  # the last warm-up step is the full factor: float(warmup) / float(warmup) == 1
            i = int((t == warmup - 1).nonzero()[0])
            plain = h.lr_factor(t[i:i + 1].to(dev), R.check_lr_schedule(kind, start, steps, end, 0)).cpu()
            assert torch.equal(got[i:i + 1], plain)
    print("lr_factor %s: worst device %.3e, worst fp32 oracle %.3e" % (kind, worst_dev, worst_cpu))


# ------------------------------------------------------------------ 2. scheduled Adam == Adam at lr * f
LR, B1, B2, EPS, GS = 3e-4, 0.5, 0.9, 1e-8, 0.5
# (kind, start, steps, end, warmup, t): in the decay; inside the warm-up; past 2^24; at the end (f = 0)
AT = [("linear", 2, 10, 0.1, 0, 7), ("cosine", 0, 9, 0.25, 5, 3), ("exponential", M, 100, 0.01, 0, M + 33),
      ("linear", 0, 2, 0.0, 0, 2), ("none", 0, 1, 1.0, 8, 2)]


def _sched(case):
    return R.check_lr_schedule(*case[:5]), case[5]


def _lr_times(lr, f):
    """fp32(lr) * f in fp32: the kernels' one multiply."""
    return float(torch.tensor(lr, dtype=F32) * f.cpu().reshape(()))


def _sides(n, edt, seed, gdt=None):
    g0 = torch.Generator().manual_seed(seed)
    init = (("w", torch.randn(n, generator=g0) * 0.02, None), ("wbf", torch.zeros(n), edt),
            ("m", torch.randn(n, generator=g0) * 1e-3, None), ("v", torch.rand(n, generator=g0) * 1e-5, None),
            ("p", torch.tensor([B1 ** 3, B2 ** 3]), None), ("g", torch.randn(n, generator=g0) * 1e-2, gdt))
    bufs, views = {}, {}
    for side in ("sched", "plain"):
        for name, x, dtp in init:
            bufs[side, name], views[side, name] = _padded(x, dtype=dtp)
    return bufs, views


def _same(bufs, views, keys, tag):
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(views["sched", k], views["plain", k]), (tag, k)
    for key, buf in bufs.items():
        assert _canaries_intact(buf), (tag, key)


@pytest.mark.parametrize("case", AT, ids=[c[0] + "-t%d" % c[5] for c in AT])
@pytest.mark.parametrize("gsrc", ["fp32", "bf16"])
def test_scheduled_adam_is_adam_at_lr_times_f(case, gsrc):
    h = H()
    s, t = _sched(case)
    n = 4100
    bufs, views = _sides(n, None, 11, torch.bfloat16 if gsrc == "bf16" else None)
    stb, step = _padded(torch.tensor([t], dtype=torch.int64), fill=0)
    f = h.lr_factor(step, s)
    w0 = views["plain", "w"].clone()
    a, b = ({k: views[side, k] for k in ("w", "g", "m", "v", "p")} for side in ("sched", "plain"))
    h.adam_(a["w"], a["g"], a["m"], a["v"], a["p"], LR, B1, B2, EPS, GS, lr_sched=s, step=step)
    h.adam_(b["w"], b["g"], b["m"], b["v"], b["p"], _lr_times(LR, f), B1, B2, EPS, GS)
    _same(bufs, views, ("w", "m", "v", "p", "g"), case)
    assert int(step) == t and not torch.equal(views["plain", "m"], torch.zeros(n, device=dev))
    assert torch.equal(views["plain", "w"], w0) == (float(f) == 0.0)  # (f = 0 moves no weight)
    assert float(views["plain", "p"][0]) == pytest.approx(B1 ** 4, rel=1e-6)


@pytest.mark.parametrize("case", AT[:4], ids=[c[0] + "-t%d" % c[5] for c in AT[:4]])
@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_scheduled_adam1_is_adam1_at_lr_times_f(case, build):
    h = H()
    s, t = _sched(case)
    n = 2052
    bufs, views = _sides(n, BUILDS[build], 12)
    stb, step = _padded(torch.tensor([t], dtype=torch.int64), fill=0)
    f = h.lr_factor(step, s)
    a, b = ({k: views[side, k] for k in ("w", "wbf", "g", "m", "v", "p")} for side in ("sched", "plain"))
    h.adam1_(a["w"], a["wbf"], a["g"], a["m"], a["v"], a["p"], LR, B1, B2, EPS, GS, lr_sched=s, step=step)
    h.adam1_(b["w"], b["wbf"], b["g"], b["m"], b["v"], b["p"], _lr_times(LR, f), B1, B2, EPS, GS)
    _same(bufs, views, ("w", "wbf", "m", "v", "p"), case)
    assert int(step) == t  # a sub-step's update never advances the global step
    assert float(views["sched", "p"][1]) == pytest.approx(B2 ** 4, rel=1e-6)
    assert torch.equal(views["sched", "wbf"], views["sched", "w"].to(BUILDS[build]))


@pytest.mark.parametrize("case", AT[:4], ids=[c[0] + "-t%d" % c[5] for c in AT[:4]])
def test_scheduled_adam2_is_adam2_at_lr_times_f(case):
    """A one-op adam2 Program: both sets, both power pairs and the step advance."""
    h = H()
    s, t = _sched(case)
    nA, nD, lrA, lrD = 2052, 1028, 1e-4, 4e-4
    bA, vA = _sides(nA, torch.bfloat16, 13)
    bD, vD = _sides(nD, torch.bfloat16, 14)
    steps = {side: _padded(torch.tensor([t], dtype=torch.int64), fill=0) for side in ("sched", "plain")}
    f = h.lr_factor(steps["sched"][1], s)
    for side, lrs, kw in (("sched", (lrA, lrD), dict(zip(("lr_kind", "lr_start", "lr_steps", "lr_end", "lr_warmup"),
                                                         s.hip_args()))),
                          ("plain", (_lr_times(lrA, f), _lr_times(lrD, f)), {})):
        p = lambda v, k: v[side, k].data_ptr()  # noqa: E731
        prog = h.ext().Program()
        prog.adam2("adam_gd", p(vA, "w"), p(vA, "wbf"), p(vA, "g"), p(vA, "m"), p(vA, "v"), p(vA, "p"), nA, lrs[0], B1,
                   B2, EPS, p(vD, "w"), p(vD, "wbf"), p(vD, "g"), p(vD, "m"), p(vD, "v"), p(vD, "p"), nD, lrs[1], 0.0,
                   0.99, EPS, GS, steps[side][1].data_ptr(), 0, **kw)
        h.run(prog)
    _same(bA, vA, ("w", "wbf", "m", "v", "p"), case)
    _same(bD, vD, ("w", "wbf", "m", "v", "p"), case)
    for side in ("sched", "plain"):
        assert int(steps[side][1]) == t + 1 and bool((steps[side][0][:SNT.PAD] == 0).all())
    assert float(vA["sched", "p"][0]) == pytest.approx(B1 ** 4, rel=1e-6)
    assert float(vD["sched", "p"][1]) == pytest.approx(B2 ** 3 * 0.99, rel=1e-6)


def test_tfadam_eager_path_takes_the_factor():
    """TFAdam.step(grads, f) on the GPU: the plain kernel at fp32(lr) * fp32(f), the kernels' multiply."""
    from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
    from distributed_tensorflow_for_dcgan_amd.optim.adam import TFAdam
    h = H()
    s, t = _sched(AT[0])
    f = h.lr_factor(torch.tensor([t], device=dev), s)
    opts = [TFAdam(DCGAN(small(), device=dev, seed=1).d, lr=LR, beta1=B1, beta2=B2) for _ in range(3)]
    for o in opts:
        o.use_hip = True
    g = torch.randn(opts[0].params.flat.numel(), generator=torch.Generator().manual_seed(3)).to(dev) * 1e-2
    opts[0].step(g, float(f))
    o = opts[1]
    h.adam_(o.params.flat, g, o.m.flat, o.v.flat, o.powers, LR, B1, B2, o.eps,
            lr_sched=s, step=torch.tensor([t], device=dev))
    opts[2].step(g)
    torch.cuda.synchronize()
    for a, b in ((opts[0].params.flat, o.params.flat), (opts[0].m.flat, o.m.flat), (opts[0].v.flat, o.v.flat),
                 (opts[0].powers, o.powers)):
        assert torch.equal(a, b)
    assert not torch.equal(opts[0].params.flat, opts[2].params.flat) and torch.equal(opts[0].m.flat, opts[2].m.flat)


# ------------------------------------------------------------------ 3. / 4. the zero step, before `start`
def _params(eng):
    t = [eng.model.g.flat, eng.model.d.flat]
    if not eng.f32:
        t += [eng.wbf_g.flat, eng.wbf_d.flat]
    return [x.detach().cpu().clone() for x in t]


def _slots(eng):
    return [x.detach().cpu().clone() for x in (eng.opt_g.m.flat, eng.opt_g.v.flat, eng.opt_d.m.flat, eng.opt_d.v.flat,
                                               eng.opt_g.powers, eng.opt_d.powers, eng.step_counter)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_the_zero_step_moves_no_weight(dtype):
    """linear, start 0, steps 2, end 0: factors 1, 0.5, 0 -- the third step leaves every parameter
    and 16-bit mirror of G and D bitwise alone while m, v, the beta powers and the step advance."""
    eng = TD._engine(small(), 8, 1, dtype=dtype, seed=2, lr_decay="linear", lr_decay_start=0, lr_decay_steps=2,
                     lr_end=0.0)
    assert eng.lr_sched == R.LrSchedule("linear", 0, 2, 0.0, 0)
    for _ in range(2):
        before = _params(eng)
        eng.train_step()
        torch.cuda.synchronize()
        assert not any(torch.equal(x, y) for x, y in zip(before, _params(eng)))
    before, slots = _params(eng), _slots(eng)
    eng.train_step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(before, _params(eng))):
        assert torch.equal(x, y), "parameter buffer %d moved at factor 0" % k
    assert not any(torch.equal(x, y) for x, y in zip(slots, _slots(eng)))
    assert eng.global_step == 3 and float(eng.opt_g.powers[0]) == pytest.approx(0.5 ** 4, rel=1e-6)


def test_before_the_decay_starts_nothing_changes():
    a = TD._engine(small(), 8, 1, seed=2, lr_decay="cosine", lr_decay_start=1000, lr_decay_steps=50)
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    b = HipEngine(small(), 8, dev, seed=2, graph=False)  # built without the arguments
    b.set_batch(TD._reals(8, small(), "bf16", 1)[0].to(dev))
    assert a.lr_sched.active and not b.lr_sched.active and a.op_names() == b.op_names()
    for _ in range(3):
        a.train_step()
        b.train_step()
    for x, y in zip(TD._snap(a), TD._snap(b)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 5. the engine against ReferenceStep
LRKW = dict(lr_decay_start=0, lr_decay_steps=4, lr_end=0.1, lr_warmup=2)


def _scheduled_piece(eng, ref, ref_model, cfg, real, dtype, sn, full, run, tag):
    """test_hip_d_steps._check_piece with its Adam oracle at lr * f, f = ReferenceStep's factor at
    the engine's global step; for a full step G's parameters get the same check as D's."""
    ref.global_step = eng.global_step
    f = ref.lr_factor()
    assert f == float(R.lr_factor(eng.lr_sched, eng.global_step))
    og, od = eng.opt_g, eng.opt_d
    g0 = [x.cpu().clone() for x in (og.params.flat, og.m.flat, og.v.flat, og.powers)]
    keep = (od.lr, og.lr)
    od.lr, og.lr = keep[0] * f, keep[1] * f  # (the recorded launches hold their own copy of lr)
    try:
        TD._check_piece(eng, ref, ref_model, cfg, real, dtype, sn, full, run, tag)
        if full:
            scale = float(eng.loss_scale[0]) if dtype == "fp16" else 1.0
            w0, m0, v0, p0 = g0
            R.tf_adam_update(w0, eng.grad_g.flat.cpu() / scale, m0, v0, float(p0[0]), float(p0[1]), og.lr, og.beta1,
                             og.beta2, og.eps)
            assert torch.allclose(og.params.flat.cpu(), w0, atol=1e-6, rtol=1e-5), tag
    finally:
        od.lr, og.lr = keep
    return f


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_four_scheduled_steps_track_the_reference(dtype, kind, seed=3):
    cfg, B = small(), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, lr_decay=kind, **LRKW)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, lr_decay=kind, **LRKW)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    fs = [_scheduled_piece(eng, ref, ref_model, cfg, real, dtype, False, True, eng.train_full_step,
                           "%s step %d" % (kind, s)) for s in range(4)]
    assert fs[0] == 0.5 and fs[1] < 1.0 and fs[3] < fs[2] < fs[1] and eng.global_step == 4


def test_scheduled_cycle_with_sub_steps_and_spectral_norm_tracks_the_reference(seed=4):
    cfg, B, dtype = DCGANConfig(output_size=28, c_dim=1, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, lr_decay="linear", **LRKW)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2, lr_decay="linear", **LRKW)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    for s in range(4):
        fa = _scheduled_piece(eng, ref, ref_model, cfg, reals[0], dtype, True, False, lambda: eng.train_d_step(0),
                              "step %d sub-step" % s)
        fb = _scheduled_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, True, eng.train_full_step,
                              "step %d full" % s)
        assert fa == fb and eng.global_step == s + 1  # the sub-step sees the step of the full step after it
    assert "adam_d1" in eng.sub_op_names(0)


# ------------------------------------------------------------------ 6. graph == eager
@pytest.mark.parametrize("dtype,d_steps", [("bf16", 2), ("fp16", 1), ("fp32", 1)])
def test_graph_replay_follows_the_live_counter(dtype, d_steps):
    """A factor baked in at capture time would repeat the first replayed step's rate."""
    kw = dict(dtype=dtype, seed=1, lr_decay="linear", **LRKW)
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    for _ in range(4):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
    assert e2.graph_enabled and not e1.graph_enabled and e1.global_step == e2.global_step == 4


# ------------------------------------------------------------------ 7. one-rank RCCL DDP
STEPS = 4


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, lr_decay="cosine", **LRKW)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "pd": eng.opt_d.powers.cpu(), "pg": eng.opt_g.powers.cpu(),
            "losses": eng.losses.cpu()}


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
    assert eng.ddp and eng._schedule() == schedule and eng.lr_sched.active
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
def test_rccl_single_rank_ddp_matches_fused_with_a_schedule(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert "adam_gd" not in r["ops"]  # (the DDP steps update with adam_bf + step_end)
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k


# ------------------------------------------------------------------ 8. resume through the trainer
def test_trainer_resume_is_exact_mid_decay(tmp_path, monkeypatch):
    """bf16: 4 steps in one run == 2 steps, a restart from the checkpoint, 2 more, with the decay
    (and the warm-up) under way at the restart -- every saved tensor bitwise, no new key."""
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
    LRF = ["--lr_decay=cosine", "--lr_decay_start=1", "--lr_decay_steps=6", "--lr_end=0.1", "--lr_warmup_steps=3"]

    def run(ck, steps, lrf=LRF):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + lrf)
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
    assert "learning-rate schedule: cosine to 0.1 x over steps 1..7, linear warm-up over 3 steps" in text
    run(tmp_path / "b", 2)
    text = run(tmp_path / "b", 4)
    assert "load success!" in text and "global_step 2" in text
    (ia, sa), (ib, sb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 4 and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    run(tmp_path / "c", 4, lrf=[])  # the constant rate trains another model, under the same keys
    ic, sc = load(tmp_path / "c")
    assert list(sc) == list(sa) and any(not (sa[k] == sc[k]).all() for k in sa)


# ------------------------------------------------------------------ 9. the bindings' argument checks
def test_bindings_reject_bad_schedules():
    h = H()
    x = torch.zeros(64, device=dev)
    xb = torch.zeros(64, device=dev, dtype=torch.bfloat16)
    p = torch.tensor([0.5, 0.9], device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ok = dict(lr_kind=1, lr_start=0, lr_steps=10, lr_end=0.1, lr_warmup=0, lr_step=step.data_ptr())
    BADKW = [dict(lr_kind=4), dict(lr_kind=-1), dict(lr_steps=0), dict(lr_steps=M + 1), dict(lr_start=-1),
             dict(lr_end=-0.5), dict(lr_end=1.5), dict(lr_kind=3, lr_end=0.0), dict(lr_warmup=-1),
             dict(lr_warmup=M + 1), dict(lr_step=0), dict(lr_kind=0, lr_warmup=3, lr_step=0)]
    P_ = lambda t: t.data_ptr()  # noqa: E731
    for bad in BADKW:
        kw = dict(ok, **bad)
        prog = h.ext().Program()
        with pytest.raises(RuntimeError, match="lr_"):
            prog.adam("a", P_(x), P_(x), P_(x), P_(x), P_(p), 64, 1e-4, 0.5, 0.9, 1e-8, 1.0, 0, **kw)
        with pytest.raises(RuntimeError, match="lr_"):
            prog.adam_bf("a", P_(x), P_(xb), P_(x), P_(x), P_(x), P_(p), 64, 1e-4, 0.5, 0.9, 1e-8, 1.0, 0, 0, 0, **kw)
        with pytest.raises(RuntimeError, match="lr_"):
            prog.adam1("a", P_(x), P_(xb), P_(x), P_(x), P_(x), P_(p), 64, 1e-4, 0.5, 0.9, 1e-8, 1.0, 0, **kw)
        kw2 = {k: v for k, v in kw.items() if k != "lr_step"}
        with pytest.raises(RuntimeError, match="lr_"):
            prog.adam2("a", P_(x), P_(xb), P_(x), P_(x), P_(x), P_(p), 64, 1e-4, 0.5, 0.9, 1e-8, P_(x), P_(xb), P_(x),
                       P_(x), P_(x), P_(p), 64, 1e-4, 0.5, 0.9, 1e-8, 1.0, kw["lr_step"], 0, **kw2)
        assert prog.size() == 0
    with pytest.raises(RuntimeError, match="lr_"):
        h.adam_(x, x.clone(), x.clone(), x.clone(), p, 1e-4, 0.5, 0.9, 1e-8, lr_sched=R.LrSchedule("linear", 0, 5, 0.0, 0))
    with pytest.raises(TypeError):
        h.adam_(x, x.clone(), x.clone(), x.clone(), p, 1e-4, 0.5, 0.9, 1e-8, lr_sched=R.LrSchedule("linear", 0, 5, 0.0, 0),
                step=torch.zeros(1, device=dev))
    with pytest.raises(TypeError):
        h.lr_factor(torch.zeros(4, device=dev), R.LrSchedule("linear", 0, 5, 0.0, 0))
