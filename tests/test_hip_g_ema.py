"""GPU tests of the generator weight EMA: the streaming ``ema_kernel`` against the fp32 oracle
(ops.reference.ema_update_), the ``ema_g`` op inside the HIP engine's step (bf16 / fp16 / fp32,
eager and hipGraph, one-rank RCCL DDP), the EMA sampler, and that decay 0 changes nothing."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
DECAY = 0.999


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _engine(**kw):
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    cfg = kw.pop("cfg", DCGANConfig())
    B = kw.pop("B", 8)
    kw.setdefault("graph", False)
    eng = HipEngine(cfg, B, dev, **kw)
    real = torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(5)) * 2 - 1
    eng.set_batch(real.to(dev))
    return eng


# ------------------------------------------------------------------ 7. the kernel
def _sizes():
    cap = H().ema_max_blocks()
    # 7: less than one vector per block (tail only); 10003: the Adam test's size, n % 4 == 3;
    # the last: every thread of the capped grid strides at least twice, some a third time, + tail 3
    return [7, 10003, 2 * cap * 256 * 4 + 4 * 100 + 3]


@pytest.mark.parametrize("edt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_ema_kernel_matches_oracle(which, edt):
    h = H()
    n = _sizes()[which]
    PAD = 64  # canary elements behind every buffer: the kernel writes nothing past n
    g = torch.Generator().manual_seed(40 + which)
    s0 = torch.randn(n + PAD, generator=g)
    w = torch.randn(n + PAD, generator=g)
    wd = w.to(dev)

    def run(step, bias, mirror=True, ls=None):
        s = s0.to(dev)
        sbf = torch.full((n + PAD,), 7.0, dtype=edt, device=dev) if mirror else None
        st = torch.tensor([step], dtype=torch.int64, device=dev)
        lsd = None if ls is None else torch.tensor(ls, dtype=torch.float32, device=dev)
        h.ema_(s[:n], None if sbf is None else sbf[:n], wd[:n], DECAY, st, bias, lsd)
        torch.cuda.synchronize()
        assert int(st.item()) == step and torch.equal(wd.cpu(), w)
        assert torch.equal(s[n:].cpu(), s0[n:])
        if sbf is not None:
            assert torch.equal(sbf[n:].cpu(), torch.full((PAD,), 7.0, dtype=edt))
        if lsd is not None:
            assert lsd.tolist() == ls
        return s[:n].cpu(), None if sbf is None else sbf[:n].cpu()

    def oracle(t):
        return R.ema_update_(s0[:n].clone(), w[:n], DECAY, t)

    a, abf = run(4, 0)              # t = 4: the warm-up branch, 5 / 14
    b, bbf = run(4, 1)              # t = 5: 6 / 15
    c, cbf = run(10 ** 6, 0)        # far past the warm-up: d_t = decay
    assert R.ema_decay_t(DECAY, 10 ** 6) == float(torch.tensor(DECAY, dtype=torch.float32))
    for got, mir, t in ((a, abf, 4), (b, bbf, 5), (c, cbf, 10 ** 6)):
        # one fma in the kernel, two roundings in the oracle: at most an ulp apart
        assert torch.allclose(got, oracle(t), atol=1e-6, rtol=1e-5), (got - oracle(t)).abs().max()
        assert torch.equal(mir, got.to(edt))
    assert not torch.equal(a, b) and not torch.equal(b, c)
    assert torch.equal(run(5, 0)[0], b)              # the bias only shifts t
    d, none = run(4, 0, mirror=False)                # no mirror: the same shadow
    assert none is None and torch.equal(d, a)
    e, ebf = run(4, 0, ls=[1024.0, 1.0, 0.0])        # overflowed fp16 step: nothing moves
    assert torch.equal(e, s0[:n]) and torch.equal(ebf, torch.full((n,), 7.0, dtype=edt))
    f, fbf = run(4, 0, ls=[1024.0, 0.0, 3.0])        # a good fp16 step: as without the state
    assert torch.equal(f, a) and torch.equal(fbf, abf)


def test_ema_helper_rejects_bad_arguments():
    h = H()
    s, w = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    st = torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        h.ema_(s, None, w[:4], DECAY, st)
    with pytest.raises(TypeError):
        h.ema_(s, None, w, DECAY, st.int())
    with pytest.raises(RuntimeError):
        h.ema_(s, None, w, 1.0, st)
    assert torch.equal(s.cpu(), torch.zeros(8))


# ------------------------------------------------------------------ 8. inside the bf16 engine
@pytest.mark.parametrize("size,c_dim", [(64, 3), (28, 1)])
def test_engine_shadow_follows_the_oracle(size, c_dim):
    eng = _engine(cfg=DCGANConfig(output_size=size, c_dim=c_dim), B=8, seed=4, g_ema_decay=DECAY)
    assert "ema_g" in eng.op_names() and eng.g_ema_decay == DECAY
    assert torch.equal(eng.g_ema.flat, eng.model.g.flat)
    assert torch.equal(eng.wbf_g_ema.flat, eng.g_ema.flat.to(torch.bfloat16))
    s = eng.model.g.flat.clone().cpu()
    for t in (1, 2, 3):
        eng.train_step()
        torch.cuda.synchronize()
        assert eng.global_step == t
        R.ema_update_(s, eng.model.g.flat.cpu(), DECAY, t)
        got = eng.g_ema.flat.cpu()
        print("t=%d max |shadow - oracle| = %.3e" % (t, (got - s).abs().max()))
        assert torch.allclose(got, s, rtol=1e-5, atol=1e-7)
        assert torch.equal(eng.wbf_g_ema.flat, eng.g_ema.flat.to(torch.bfloat16))
        assert torch.equal(eng.wbf_g.flat, eng.model.g.flat.to(torch.bfloat16))
    assert not torch.equal(eng.g_ema.flat, eng.model.g.flat)


# ------------------------------------------------------------------ 9. graph == eager, 11. off is off
@pytest.fixture(scope="module")
def runs():
    """B=16, seed 1, 4 steps (3 for the off / default pair): eager + EMA, graph + EMA, decay 0,
    default constructor."""
    old = os.environ.pop("DCGAN_G_EMA_DECAY", None)
    try:
        out = {}
        for name, kw, steps in (("eager", dict(g_ema_decay=DECAY), 4), ("graph", dict(g_ema_decay=DECAY, graph=True), 4),
                                ("off", dict(g_ema_decay=0), 3), ("default", dict(), 3)):
            eng = _engine(B=16, seed=1, **kw)
            snaps = []
            for _ in range(steps):
                eng.train_step()
                torch.cuda.synchronize()
                snaps.append((eng.model.g.flat.clone(), eng.model.d.flat.clone(), eng.last_losses()))
            out[name] = (eng, snaps)
        return out
    finally:
        if old is not None:
            os.environ["DCGAN_G_EMA_DECAY"] = old


def test_engine_graph_replay_shadow_matches_eager(runs):
    (e1, s1), (e2, s2) = runs["eager"], runs["graph"]
    assert e2.graph_enabled and not e1.graph_enabled
    assert e1.global_step == e2.global_step == 4
    assert torch.equal(e1.g_ema.flat, e2.g_ema.flat)
    assert torch.equal(e1.wbf_g_ema.flat, e2.wbf_g_ema.flat)
    assert torch.equal(e1.model.g.flat, e2.model.g.flat) and torch.equal(e1.model.d.flat, e2.model.d.flat)
    assert not torch.equal(e1.g_ema.flat, e1.model.g.flat)


def test_off_is_off(runs):
    (off, so), (dflt, sd), (on, son) = runs["off"], runs["default"], runs["eager"]
    assert off.g_ema is None and off.wbf_g_ema is None and dflt.g_ema is None
    assert off.op_names() == dflt.op_names() and "ema_g" not in off.op_names()
    assert off.kernel_count() == dflt.kernel_count() == on.kernel_count() - 1
    assert [n for n in on.op_names() if n != "ema_g"] == off.op_names()
    for k in range(3):
        assert torch.equal(so[k][0], sd[k][0]) and torch.equal(so[k][1], sd[k][1]) and so[k][2] == sd[k][2]
        # ... and keeping the average changes neither the weights nor the losses
        assert torch.equal(so[k][0], son[k][0]) and torch.equal(so[k][1], son[k][1]) and so[k][2] == son[k][2]


# ------------------------------------------------------------------ 12. the sampler
def test_sampler_ema(runs):
    (off, so), (on, son) = runs["off"], runs["eager"]
    cfg, B = on.cfg, on.B
    z = (torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    # the average against the PyTorch sampler over the shadow
    ref = DCGAN(cfg, device=dev, seed=1)
    ref.g.flat.copy_(on.g_ema.flat)
    ref.g_bn.flat.copy_(on.model.g_bn.flat)
    s_ref = ref.sampler(z)
    s_ema = on.sampler(z, ema=True)
    assert s_ema.shape == (B, 64, 64, 3)
    print("sampler(ema=True) rel = %.3e" % rel(s_ema, s_ref))
    assert rel(s_ema, s_ref) < 5e-2
    assert torch.equal(on.sampler(z), s_ema)  # None: the average when it is kept
    assert rel(on.model.sampler(z, ema=True), s_ref) < 1e-6  # (the PyTorch sampler sees the same shadow)
    # the last iterate: bit-equal to the engine without the feature at the same weights
    fresh = _engine(B=16, seed=1, g_ema_decay=0)
    assert on.global_step == 4 and off.global_step == 3
    fresh.model.g.flat.copy_(on.model.g.flat)
    fresh.model.g_bn.flat.copy_(on.model.g_bn.flat)
    fresh.after_state_load()
    s_last = on.sampler(z, ema=False)
    assert torch.equal(s_last, fresh.sampler(z))
    assert torch.equal(fresh.sampler(z, ema=False), s_last)
    assert not torch.equal(s_last, s_ema)
    with pytest.raises(ValueError):
        fresh.sampler(z, ema=True)


def test_checkpoint_load_refreshes_the_shadow_mirror(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
    a = _engine(cfg=DCGANConfig(output_size=28, c_dim=1), seed=2, g_ema_decay=0.9)
    a.train_step()
    a.train_step()
    mgr = CK.CheckpointManager(str(tmp_path), save_secs=0)
    mgr.save(a)
    b = _engine(cfg=DCGANConfig(output_size=28, c_dim=1), seed=7, g_ema_decay=0.9)
    info = mgr.restore_latest(b)
    torch.cuda.synchronize()
    assert info["g_ema"] == "loaded"
    assert torch.equal(b.g_ema.flat, a.g_ema.flat) and torch.equal(b.wbf_g_ema.flat, a.wbf_g_ema.flat)
    z = (torch.rand(8, 100, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    assert torch.equal(a.sampler(z, ema=True), b.sampler(z, ema=True))


# ------------------------------------------------------------------ 10. fp16 skip, fp32
def test_fp16_skipped_step_leaves_the_shadow():
    eng = _engine(B=16, seed=1, dtype="fp16", graph=True, g_ema_decay=DECAY)
    eng.train_step()
    eng.train_step()  # second step replays the captured graphs
    torch.cuda.synchronize()
    assert eng.loss_scale.tolist()[1:] == [0.0, 2.0]
    s0, m0, w0 = eng.g_ema.flat.clone(), eng.wbf_g_ema.flat.clone(), eng.model.g.flat.clone()
    assert not torch.equal(s0, w0) and torch.equal(m0, s0.to(torch.float16))
    eng.loss_scale[0] = 1e38
    eng.train_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.model.g.flat, w0)
    assert torch.equal(eng.g_ema.flat, s0) and torch.equal(eng.wbf_g_ema.flat, m0)
    assert eng.loss_scale.tolist()[1] == 0.0 and eng.global_step == 3
    eng.loss_scale[0] = 1024.0
    eng.train_step()
    torch.cuda.synchronize()
    assert not torch.equal(eng.model.g.flat, w0) and not torch.equal(eng.g_ema.flat, s0)
    # t = the global step after the increment (the skipped step counted): 4
    exp = R.ema_update_(s0.clone().cpu(), eng.model.g.flat.cpu(), DECAY, 4)
    assert torch.allclose(eng.g_ema.flat.cpu(), exp, rtol=1e-5, atol=1e-7)
    assert torch.equal(eng.wbf_g_ema.flat, eng.g_ema.flat.to(torch.float16))


def test_fp32_engine_shadow_follows_the_oracle():
    eng = _engine(B=8, seed=4, dtype="fp32", g_ema_decay=DECAY)
    assert eng.wbf_g_ema is eng.g_ema  # no mirror: the sampler's GEMMs read the shadow itself
    s = eng.model.g.flat.clone().cpu()
    for t in (1, 2):
        eng.train_step()
        torch.cuda.synchronize()
        R.ema_update_(s, eng.model.g.flat.cpu(), DECAY, t)
        assert torch.allclose(eng.g_ema.flat.cpu(), s, rtol=1e-5, atol=1e-7)
    z = (torch.rand(8, 100, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    ref = DCGAN(eng.cfg, device=dev, seed=4)
    ref.g.flat.copy_(eng.g_ema.flat)
    ref.g_bn.flat.copy_(eng.model.g_bn.flat)
    assert rel(eng.sampler(z, ema=True), ref.sampler(z)) < 5e-2


# ------------------------------------------------------------------ 13. one-rank RCCL DDP
STEPS = 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_engine(graph):
    return _engine(B=16, seed=3, graph=graph, rank_seeded_z=False, g_ema_decay=DECAY)


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
    torch.cuda.synchronize()
    torch.save({"g": eng.model.g.flat.cpu(), "ema": eng.g_ema.flat.cpu(), "mirror": eng.wbf_g_ema.flat.cpu(),
                "step": eng.global_step, "backend": tdist.get_backend(), "graph": eng.graph_enabled,
                "ops": eng.op_names()}, os.path.join(out_dir, "rccl.pt"))
    D.barrier()
    D.shutdown()


@pytest.fixture(scope="module")
def fused_run():
    eng = _ddp_engine(True)
    assert not eng.ddp and eng._schedule() == "fused"
    for _ in range(STEPS):
        eng.train_step()
    torch.cuda.synchronize()
    return eng.model.g.flat.cpu(), eng.g_ema.flat.cpu(), eng.wbf_g_ema.flat.cpu()


@pytest.mark.parametrize("graph", [False, True])
def test_rccl_single_rank_ddp_shadow_matches_fused(tmp_path, graph, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), graph, _free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"] == graph
    assert r["ops"].count("ema_g") == 1 and {"adam_g_a", "adam_g_b", "adam_g_c"} <= set(r["ops"])
    g, ema, mirror = fused_run
    assert torch.equal(r["g"], g)
    assert torch.equal(r["ema"], ema), (r["ema"] - ema).abs().max()
    assert torch.equal(r["mirror"], mirror)
