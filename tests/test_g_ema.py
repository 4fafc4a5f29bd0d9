"""CPU tests of the generator weight EMA (tf.train.ExponentialMovingAverage(decay, num_updates =
global step) over G's variables): the fp32 oracle, the flags, the reference engine, checkpoints
and -- on dry-run HIP engines -- where every update schedule records the ``ema_g`` op."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
from distributed_tensorflow_for_dcgan_amd.ckpt import tf_bundle
from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
SMALL = DCGANConfig(output_size=28, c_dim=1)


# ------------------------------------------------------------------ 1. the oracle
def test_ema_decay_warmup_and_cap():
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert R.ema_decay_t(0.999, 1) == f32(np.float32(2) / np.float32(11))
    assert R.ema_decay_t(0.999, 90) == f32(np.float32(91) / np.float32(100))
    assert abs(R.ema_decay_t(0.999, 90) - 0.91) < 1e-7
    assert R.ema_decay_t(0.999, 10000) == f32(0.999)  # (1 + t) / (10 + t) = 0.99910... > decay: capped
    assert R.ema_decay_t(0.5, 1) == f32(np.float32(2) / np.float32(11))  # min() picks the warm-up while it is smaller
    assert R.ema_decay_t(0.5, 100) == 0.5


def test_ema_update_matches_closed_form():
    """5 updates of a random 1000-vector == the unrolled sum s_T = prod(d) s_0 + sum_k (1 - d_k)
    prod_{j>k}(d_j) w_k, evaluated in float64."""
    g = torch.Generator().manual_seed(0)
    s0 = torch.randn(1000, generator=g)
    ws = [torch.randn(1000, generator=g) for _ in range(5)]
    decay = 0.9
    s = s0.clone()
    for t, w in enumerate(ws, 1):
        out = R.ema_update_(s, w, decay, t)
        assert out is s
    ds = [float(R.ema_decay_t(decay, t)) for t in range(1, 6)]
    exp = s0.double() * float(np.prod(ds))
    for k, w in enumerate(ws):
        exp += (1.0 - ds[k]) * float(np.prod(ds[k + 1:])) * w.double()
    # fp32 rounding of 5 updates of O(1) values: a few ulp of 1.0
    assert torch.allclose(s.double(), exp, rtol=0, atol=2e-6), (s.double() - exp).abs().max()
    assert s.dtype == torch.float32


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan")])
def test_bad_decay_is_rejected_everywhere(bad):
    with pytest.raises(ValueError):
        R.check_ema_decay(bad)
    with pytest.raises(ValueError):
        ReferenceEngine(SMALL, 2, CPU, g_ema_decay=bad)
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    with pytest.raises(ValueError):
        HipEngine(SMALL, 2, CPU, dry_run=True, graph=False, g_ema_decay=bad)


# ------------------------------------------------------------------ 2. flags
def test_flags_parse_and_defaults():
    fl = F.parse_flags([])
    assert fl.g_ema_decay == 0.0 and fl.sample_ema is True
    assert F.default_flags().g_ema_decay == 0.0 and F.default_flags().sample_ema is True
    fl = F.parse_flags(["--g_ema_decay=0.999", "--nosample_ema"])
    assert fl.g_ema_decay == 0.999 and fl.sample_ema is False
    fl = F.parse_flags(["--g_ema_decay", "0.5", "--sample_ema=false"])
    assert fl.g_ema_decay == 0.5 and fl.sample_ema is False
    assert fl.explicitly_set("g_ema_decay") and fl.explicitly_set("sample_ema")
    for bad in ("1.0", "-0.5", "2"):
        with pytest.raises(SystemExit):
            F.parse_flags(["--g_ema_decay=" + bad])


# ------------------------------------------------------------------ 3. reference engine
def _real(B, cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=g) * 2 - 1


@pytest.fixture(scope="module")
def ref_run():
    """ReferenceEngine(g_ema_decay=0.9), B=4, 3 steps: the weights after every step, the engine."""
    eng = ReferenceEngine(SMALL, 4, CPU, seed=3, g_ema_decay=0.9)
    eng.set_batch(_real(4, SMALL))
    w = [eng.model.g.flat.clone()]
    assert torch.equal(eng.g_ema.flat, w[0])  # starts at G's parameters
    for _ in range(3):
        eng.train_step()
        w.append(eng.model.g.flat.clone())
    return eng, w


def test_reference_engine_shadow_follows_the_oracle(ref_run):
    eng, w = ref_run
    assert eng.global_step == 3 and eng.g_ema_decay == 0.9
    s = w[0].clone()
    for t in (1, 2, 3):
        R.ema_update_(s, w[t], 0.9, t)
    assert torch.equal(eng.g_ema.flat, s)
    assert not torch.equal(eng.g_ema.flat, eng.model.g.flat)
    assert eng.g_ema.names() == eng.model.g.names()
    assert eng.g_ema.flat.numel() == eng.model.g.flat.numel()  # same flat layout, padding included
    z = torch.rand(4, SMALL.z_dim, generator=torch.Generator().manual_seed(1)) * 2 - 1
    a, b = eng.sampler(z, ema=True), eng.sampler(z, ema=False)
    assert a.shape == b.shape == (4, 28, 28, 1)
    assert not torch.equal(a, b)
    assert torch.equal(eng.sampler(z), a)  # None = the average when it is kept


def test_reference_engine_off_is_todays_engine(ref_run, monkeypatch):
    monkeypatch.delenv("DCGAN_G_EMA_DECAY", raising=False)
    on, _ = ref_run
    off = ReferenceEngine(SMALL, 4, CPU, seed=3, g_ema_decay=0.0)
    dflt = build_engine(SMALL, 4, CPU, engine="reference", seed=3)
    for e in (off, dflt):
        assert e.g_ema is None and e.g_ema_decay == 0.0
        e.set_batch(_real(4, SMALL))
        for _ in range(3):
            e.train_step()
    z = torch.rand(4, SMALL.z_dim, generator=torch.Generator().manual_seed(1)) * 2 - 1
    today = off.model.generator(z, train=False, update_ema=False)  # what sampler(z) was before
    assert torch.equal(off.sampler(z), today) and torch.equal(off.sampler(z, ema=False), today)
    assert torch.equal(off.model.g.flat, dflt.model.g.flat)
    assert torch.equal(off.model.g.flat, on.model.g.flat)  # keeping the average changes no weight
    assert torch.equal(on.sampler(z, ema=False), today)
    with pytest.raises(ValueError):
        off.sampler(z, ema=True)


def test_env_switch_sets_the_default(monkeypatch):
    monkeypatch.setenv("DCGAN_G_EMA_DECAY", "0.99")
    assert ReferenceEngine(SMALL, 2, CPU).g_ema_decay == 0.99
    assert ReferenceEngine(SMALL, 2, CPU, g_ema_decay=0.0).g_ema is None  # an explicit value wins
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    assert HipEngine(SMALL, 2, CPU, dry_run=True, graph=False).g_ema_decay == 0.99
    assert HipEngine(SMALL, 2, CPU, dry_run=True, graph=False, g_ema_decay=0.0).g_ema is None


# ------------------------------------------------------------------ 4. checkpoints
def _expected_keys_without_ema(eng):
    m = eng.model
    keys = list(m.g.tensors) + list(m.d.tensors) + ["Variable"]
    for bn, slots in ((m.g_bn, 1), (m.d_bn, 2)):
        for name, _ in bn.layers:
            for s in range(slots):
                scope = name if s == 0 else "%s_%d" % (name, s)
                keys += [scope + "/moments/Squeeze/ExponentialMovingAverage",
                         scope + "/moments/Squeeze_1/ExponentialMovingAverage"]
    keys += ["g_bn/ExponentialMovingAverage/local_step", "d_bn/ExponentialMovingAverage/local_step"]
    for ps, suf in ((m.d, ""), (m.g, "_1")):
        for name in ps.tensors:
            keys += [name + "/Adam", name + "/Adam_1"]
        keys += ["beta1_power" + suf, "beta2_power" + suf]
    return keys


def test_checkpoint_round_trip(ref_run, tmp_path, monkeypatch):
    monkeypatch.delenv("DCGAN_G_EMA_DECAY", raising=False)
    on, _ = ref_run
    g_names = list(on.model.g.tensors)
    ema_keys = [k + "/ExponentialMovingAverage" for k in g_names]
    st_on = CK.collect_state(on)
    assert list(st_on) == _expected_keys_without_ema(on) + ema_keys
    for k in g_names:
        assert np.array_equal(st_on[k + "/ExponentialMovingAverage"], on.g_ema[k].numpy())
    # off: exactly the parent's key set
    off = ReferenceEngine(SMALL, 4, CPU, seed=5)
    off.set_batch(_real(4, SMALL))
    off.train_step()
    st_off = CK.collect_state(off)
    assert list(st_off) == _expected_keys_without_ema(off)
    assert not any(k.endswith("/ExponentialMovingAverage") and "/moments/" not in k for k in st_off)
    # save (TF bundle on disk) -> load into a fresh engine: the shadow is bit-equal
    mgr = CK.CheckpointManager(str(tmp_path / "on"), save_secs=0)
    mgr.save(on)
    fresh = ReferenceEngine(SMALL, 4, CPU, seed=9, g_ema_decay=0.9)
    info = mgr.restore_latest(fresh)
    assert info["g_ema"] == "loaded" and info["global_step"] == 3
    assert torch.equal(fresh.g_ema.flat, on.g_ema.flat)
    assert torch.equal(fresh.model.g.flat, on.model.g.flat)
    # a shadow-less checkpoint: the shadow starts at the loaded weights, and info says so
    mgr_off = CK.CheckpointManager(str(tmp_path / "off"), save_secs=0)
    mgr_off.save(off)
    fresh2 = ReferenceEngine(SMALL, 4, CPU, seed=9, g_ema_decay=0.9)
    info = mgr_off.restore_latest(fresh2)
    assert "initialised from the loaded weights" in info["g_ema"]
    assert torch.equal(fresh2.g_ema.flat, off.model.g.flat) and torch.equal(fresh2.model.g.flat, off.model.g.flat)
    # a checkpoint with shadows into an engine without: the keys are ignored
    fresh3 = ReferenceEngine(SMALL, 4, CPU, seed=9)
    info = mgr.restore_latest(fresh3)
    assert "g_ema" not in info and fresh3.g_ema is None
    assert torch.equal(fresh3.model.g.flat, on.model.g.flat)
    # a partial set of shadow keys is not a shadow
    sd = tf_bundle.read_bundle(CK.latest_checkpoint(str(tmp_path / "on")))
    del sd[ema_keys[0]]
    fresh4 = ReferenceEngine(SMALL, 4, CPU, seed=9, g_ema_decay=0.9)
    assert "initialised" in CK.apply_state(fresh4, sd)["g_ema"]
    assert torch.equal(fresh4.g_ema.flat, on.model.g.flat)


# ------------------------------------------------------------------ 5. schedules (dry-run HIP engines)
CASES = [(1, None, False), (1, None, True), (1, "serial", False), (2, None, False), (2, "ddp", False),
         (2, "serial", False)]


def _dry(dtype="bf16", world=1, schedule=None, timing=False, decay=0.999, wire="fp32", cfg=None):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    eng = HipEngine(cfg or DCGANConfig(), 4, CPU, dtype=dtype, world=world, schedule=schedule, dry_run=True,
                    graph=False, allreduce_dtype=wire, g_ema_decay=decay)
    if timing:
        eng._timing = True
        eng._build_updates()
    return eng


def _ops(prog):
    return [prog.op_info(i) for i in range(prog.size())]


def _check_ema_op(eng):
    """ema_g: once, in progC, after every Adam launch that writes G, before the launch that
    advances the step counter / clears the overflow flag (unless adam2 already did: bias 0);
    recorded accesses = the issue's byte ranges; the segment tables cover progC exactly once."""
    ops = _ops(eng.progC)
    names = [o[0] for o in ops]
    assert names.count("ema_g") == 1
    k = names.index("ema_g")
    assert "ema_g" not in eng.op_names()[:-len(names)]  # (in no other program of the step)
    g_adams = [i for i, n in enumerate(names) if n.startswith("adam_g")]  # adam_g, adam_g_a/b/c, adam_gd
    assert g_adams and max(g_adams) < k
    if "step_end" in names:
        assert k < names.index("step_end")
    assert ops[k][1] == ops[max(g_adams)][1] == 0  # same stream slot as the Adam launch
    n = eng.model.g.flat.numel()
    es = 4 if eng.f32 else 2
    exp = [(eng.g_ema.flat.data_ptr(), 4 * n, True)]
    if not eng.f32:
        exp.append((eng.wbf_g_ema.flat.data_ptr(), es * n, True))
    exp += [(eng.model.g.flat.data_ptr(), 4 * n, False), (eng.step_counter.data_ptr(), 8, False)]
    if eng.f16:
        exp.append((eng.loss_scale.data_ptr(), 12, False))
    assert [tuple(a) for a in ops[k][4]] == exp
    # every op of progC is issued exactly once per step
    ex = SC.RecordingExec(eng.ext)
    eng._ensure_comm()
    eng._run_step(ex)
    labels = [o.label.split(":", 1)[1] for o in ex.ops]
    for nm in set(names):
        assert labels.count(nm) == names.count(nm), (nm, labels.count(nm))
    return ex


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("world,schedule,timing", CASES)
def test_schedules_with_ema_have_no_stream_hazards(dtype, world, schedule, timing, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    eng = _dry(dtype, world, schedule, timing)
    off = _dry(dtype, world, schedule, timing, decay=0.0)
    assert eng._schedule() == (schedule or ("fused" if world == 1 and not timing else "concurrent"))
    assert off.g_ema is None and off.wbf_g_ema is None and "ema_g" not in off.op_names()
    assert eng.kernel_count() == off.kernel_count() + 1
    assert [n for n in eng.op_names() if n != "ema_g"] == off.op_names()
    ex = _check_ema_op(eng)
    # the stream of the last Adam(G) launch
    by = {o.label.split(":", 1)[1]: o.stream for o in ex.ops}
    last_adam = [n for n in (o.label.split(":", 1)[1] for o in ex.ops) if n.startswith("adam_g")][-1]
    assert by["ema_g"] == by[last_adam]
    hz, n = SC.check_engine(eng)
    assert n > 100
    assert hz == [], "\n".join(map(str, hz[:10]))
    # the mirror refresh after a checkpoint load covers the shadow
    casts = _ops(eng.progCast)
    assert len(casts) == (0 if dtype == "fp32" else 3)
    if dtype != "fp32":
        assert any(a[0] == eng.wbf_g_ema.flat.data_ptr() and a[2] for a in casts[-1][4])
    assert any(t.data_ptr() == eng.g_ema.flat.data_ptr() for t in eng.sync_check_tensors())
    assert len(off.sync_check_tensors()) == 2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("schedule", [None, "serial", "ddp"])
def test_bf16_wire_schedules_with_ema_have_no_hazards(dtype, schedule, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    eng = _dry(dtype, 2, schedule, wire="bf16")
    _check_ema_op(eng)
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _, hz, _ = SC.check(DCGANConfig(), 4, dtype, 2, schedule, False, allreduce_dtype="bf16", g_ema_decay=0.999)
    assert hz == []


@pytest.mark.parametrize("split", ["0", "1"])
def test_adam_g_split_and_small_model_with_ema(split, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    monkeypatch.setenv("DCGAN_ADAM_G_SPLIT", split)
    for cfg in (DCGANConfig(), SMALL):
        eng = _dry(world=2, cfg=cfg)
        assert ("adam_G_a" in [n for n, _, _ in eng._segments()]) == (split == "1")
        _check_ema_op(eng)
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))


def test_step_bias_follows_the_step_counter(monkeypatch):
    """bias 0 after adam2 (it advances the counter itself), 1 before step_end: both see t =
    the global step after this step's increment. The bias is not part of op_info, so compare
    where the op sits relative to the launch that writes the counter."""
    monkeypatch.setenv("DCGAN_DDP_SHARD", "0")
    for kw in (dict(), dict(dtype="fp16"), dict(dtype="fp32"), dict(world=2), dict(schedule="serial")):
        eng = _dry(**kw)
        ops = _ops(eng.progC)
        names = [o[0] for o in ops]
        step_p = eng.step_counter.data_ptr()
        writers = [i for i, o in enumerate(ops) if any(a[0] == step_p and a[2] for a in o[4])]
        assert len(writers) == 1
        k = names.index("ema_g")
        assert (writers[0] < k) == (names[writers[0]] == "adam_gd")


def test_sharded_update_with_ema_raises(monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    with pytest.raises(ValueError, match="DCGAN_DDP_SHARD"):
        _dry(world=2)
    assert _dry(world=2, decay=0.0)._sharded()  # off: the sharded update itself is untouched


# ------------------------------------------------------------------ 6. planted hazards
def test_checker_finds_ema_in_front_of_adam_g_on_another_stream():
    """ema_g issued on the side stream without a join, while Adam(G) runs on the main stream."""
    eng = _dry(dtype="fp32")  # fused schedule, adam_g / ema_g / adam_d / step_end
    names = [o[0] for o in _ops(eng.progC)]
    k = names.index("ema_g")
    assert names[k - 1] == "adam_g"
    orig = eng._run_fused

    def racy(ex, cs):
        real_run = ex.run

        def run(prog, streams, begin=0, end=-1):
            if prog is eng.progC:
                real_run(prog, streams, 0, k)
                real_run(prog, [ex.alt[1], ex.side], k, k + 1)  # slot 0 -> the idle alt1 stream, no join
                real_run(prog, streams, k + 1, -1)
            else:
                real_run(prog, streams, begin, end)
        ex.run = run
        try:
            orig(ex, cs)
        finally:
            ex.run = real_run

    eng._run_fused = racy
    hz, _ = SC.check_engine(eng)
    txt = "\n".join(map(str, hz))
    assert hz and "ema_g@alt1" in txt and "adam_g@main" in txt, txt


def test_checker_finds_ema_before_the_g_collective():
    """Segmented DDP step: ema_g (and nothing else) moved in front of the join with G's
    collectives -- it then reads weights that the Adam launches after the join still write."""
    eng = _dry(world=2)
    names = [o[0] for o in _ops(eng.progC)]
    k = names.index("ema_g")
    orig_join = eng._ar_join

    def join(ex, dst):
        ex.run(eng.progC, [ex.alt[1], ex.side], k, k + 1)  # before Adam(G)'s last part, on another stream
        orig_join(ex, dst)

    eng._ar_join = join
    hz, _ = SC.check_engine(eng)
    assert any(("ema_g" in h.a and "adam_g" in h.b) or ("ema_g" in h.b and "adam_g" in h.a) for h in hz), \
        "\n".join(map(str, hz[:10]))


# ------------------------------------------------------------------ CLI: flags -> engine -> checkpoint -> sampler
def test_cli_trains_saves_and_samples_from_the_average(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--synthetic", "--output_size=28", "--c_dim=1", "--batch_size=4", "--device=cpu",
              "--checkpoint_dir=%s" % (tmp_path / "ck"), "--save_summaries_secs=1000", "--sample_every=0",
              "--num_samples=4"]

    def run(args):
        env = dict(os.environ, OMP_NUM_THREADS="4")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DCGAN_G_EMA_DECAY"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.join(root, "image_train.py")] + common + args, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout

    rc, out = run(["--max_steps=3", "--g_ema_decay=0.9", "--sample_dir=%s" % (tmp_path / "s0")])
    assert rc == 0, out
    assert "'g_ema_decay': 0.9" in out and "'sample_ema': True" in out
    sd = tf_bundle.read_bundle(CK.latest_checkpoint(str(tmp_path / "ck")))
    assert "g_h0_lin/Matrix/ExponentialMovingAverage" in sd
    assert not np.array_equal(sd["g_h0_lin/Matrix/ExponentialMovingAverage"], sd["g_h0_lin/Matrix"])
    pngs = {}
    for tag, extra in (("ema", ["--g_ema_decay=0.9"]), ("last", ["--g_ema_decay=0.9", "--nosample_ema"]), ("off", [])):
        rc, out = run(["--nois_train", "--sample_dir=%s" % (tmp_path / tag)] + extra)
        assert rc == 0, out
        assert ("generator weight EMA: loaded" in out) == (tag != "off")
        with open(tmp_path / tag / "test_000003.png", "rb") as f:
            pngs[tag] = f.read()
    assert pngs["ema"] != pngs["last"]      # the average is what gets sampled by default ...
    assert pngs["last"] == pngs["off"]      # ... and --nosample_ema is the sampler of a run without it
    rc, out = run(["--g_ema_decay=1.0"])
    assert rc != 0 and "g_ema_decay" in out
