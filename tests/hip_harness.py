"""What the GPU feature tests (tests/test_hip_*.py) share: the small helpers, the engine against
``ReferenceStep`` piece by piece (``check_piece``: the comparison every per-step reference test rests
on), the one-rank RCCL DDP run against the fused step, and the exact resume through the trainer.

A plain module, imported by name: no test, no fixture of its own, no pytest hook. Nothing here touches
the GPU at import, so the module also loads where the GPU tests are only collected."""
import contextlib
import io
import os
import socket
from typing import Any, Callable, NamedTuple, Optional

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import options as O
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

dev = torch.device("cuda", 0)
BUILDS = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PAD = 64  # canary elements around every slice the kernels write
FILL = 7.0
# The switches every feature module clears around its tests. Literal: DCGAN_D_UPDATE is no option of
# ops/options.py, and DCGAN_LABEL_SMOOTH, which is one, was never in this list.
ENV = ("DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G", "DCGAN_D_UPDATE", "DCGAN_D_SPECTRAL_NORM",
       "DCGAN_G_EMA_DECAY", "DCGAN_GAN_LOSS")


def env_of(*groups):
    """The environment variables of whole option groups, from ops/options.py's table."""
    return tuple(n for g in groups for n in O.TABLE[g].env)


def clean_env(names):
    """An autouse fixture that removes `names` from the environment around every test of a module."""
    @pytest.fixture(autouse=True)
    def _clean_env(monkeypatch):
        for k in names:
            monkeypatch.delenv(k, raising=False)
    return _clean_env


# ------------------------------------------------------------------ small helpers
def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def small():
    return DCGANConfig(output_size=28, c_dim=1)


def prog(dt=None):
    return H().ext().Program() if dt is None else H().ext().Program(dt)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def bf(t):
    return t.to(torch.bfloat16).contiguous()


def close(out, ref, rel=1.5e-2, name="", show=False):
    """max |out - ref| <= rel x max |ref|. show: print the two numbers first (test_hip_gan_objectives.py's
    copy did, test_hip_kernels.py's did not)."""
    out = out.float()
    ref = ref.float()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item()
    if show:
        print("%s: max err %.3e vs scale %.3e" % (name, err, scale))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).mul(scale).to(dev)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def slot(shape, dtype, off=0, fill=FILL, pad=PAD):
    """A view of `shape` (or of n elements) `off` elements past a 16-byte boundary, `pad` canaries of
    `fill` on both sides: (buffer, view)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * pad + off,), fill, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[pad + off:pad + off + n].view(shape)


def intact(buf, off=0, fill=FILL, pad=PAD):
    return bool((buf[:pad + off] == fill).all()) and bool((buf[-pad:] == fill).all())


def padded(x, dtype=None, fill=FILL):
    """x, flattened, inside a slot of its own: (buffer, view of x)."""
    dtype = dtype or x.dtype
    buf, view = slot(x.numel(), dtype, fill=fill)
    view.copy_(x.flatten().to(dtype))
    return buf, view


def ulps_apart(a, b):
    """Distance in units of the last place between two 16-bit tensors of one dtype."""
    ia, ib = a.view(torch.int16).int(), b.view(torch.int16).int()
    key = lambda x: torch.where(x < 0, -(x & 0x7FFF), x)  # noqa: E731  sign-magnitude -> ordered
    return (key(ia) - key(ib)).abs()


# ------------------------------------------------------------------ engines and their state
def real(B, cfg, edt=None):
    x = torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(5)) * 2 - 1
    if edt is not None and edt != torch.float32:
        x = x.to(edt).float()
    return x


def reals(B, cfg, dtype, n):
    out = []
    for k in range(n):
        x = torch.rand(B, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(5 + k)) * 2 - 1
        out.append(x.to(BUILDS[dtype]).float())
    return out


def engine(cfg, B=8, d_steps=None, **kw):
    """An eager HipEngine with its batches staged. d_steps None: built without the argument, one batch
    through ``set_batch(x)`` (test_hip_d_spectral_norm.py's engine); a number: built with it, batch k
    through ``set_batch(x, k)`` (test_hip_d_steps.py's). Batch 0 is the same tensor in both."""
    from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
    kw.setdefault("graph", False)
    if d_steps is None:
        eng = HipEngine(cfg, B, dev, **kw)
        eng.set_batch(real(B, cfg, BUILDS[kw.get("dtype", "bf16")]).to(dev))
        return eng
    eng = HipEngine(cfg, B, dev, d_steps=d_steps, **kw)
    for k, x in enumerate(reals(B, cfg, kw.get("dtype", "bf16"), d_steps)):
        eng.set_batch(x.to(dev), k)
    return eng


def g_state(eng):
    t = [eng.model.g.flat, eng.wbf_g.flat, eng.opt_g.m.flat, eng.opt_g.v.flat, eng.opt_g.powers, eng.model.g_bn.flat,
         torch.as_tensor(eng.model.g_bn.steps), eng.step_counter]
    if eng.g_ema is not None:
        t += [eng.g_ema.flat, eng.wbf_g_ema.flat]
    return [x.detach().cpu().clone() for x in t]


def d_state(eng):
    t = [eng.model.d.flat, eng.wbf_d.flat, eng.opt_d.m.flat, eng.opt_d.v.flat, eng.opt_d.powers]
    if eng.d_spectral_norm:
        t += [eng.model.d_sn.flat, eng.sn_head]
    return [x.detach().cpu().clone() for x in t]


def snap(eng):
    torch.cuda.synchronize()
    return g_state(eng) + d_state(eng) + [eng.model.d_bn.flat.cpu().clone(), eng.model.g_bn.flat.cpu().clone(),
                                           eng.losses.cpu().clone()]


def snap_equal(first, *others):
    """Every tensor of ``snap`` is bitwise the same in all the engines."""
    want = snap(first)
    for eng in others:
        for x, y in zip(want, snap(eng)):
            assert torch.equal(x, y)


def copies_match_state(eng):
    """Every normalised copy is W * (1 / sigma) of the stored sigma, rounded to its dtype."""
    sn = eng.model.d_sn
    for name, K, C in sn.shapes:
        exp = eng.model.d[name].flatten() * (1.0 / sn.sigma[name])
        if name.endswith("/Matrix"):
            got = eng.sn_head
        else:
            got = eng.wbf_d[name].flatten()
        if got.dtype == torch.float32:
            assert torch.allclose(got, exp, rtol=2 * 2.0 ** -24, atol=0), name
        else:
            assert int(ulps_apart(got.cpu(), exp.to(got.dtype).cpu()).max()) <= 1, name


# ------------------------------------------------------------------ a piece of the cycle against ReferenceStep
KINK_MAX_INPUT = 1e-6


def engine_signs(eng, cfg):
    """Sign masks of the engine's activations, in the order the reference calls ReLU (G) and
    LeakyReLU (D)."""
    acts = [eng.g_h0] + [eng.g_a[L.name] for L in cfg.g_layers()[:-1]] + [eng.d_a[L.name] for L in cfg.d_layers()]
    return [(m.float() > 0).cpu() for m in acts]


@contextlib.contextmanager
def recording(inputs):
    """Within the block every input of the reference's ReLU / LeakyReLU is appended to `inputs`;
    the reference itself is unchanged."""
    relu, lrelu = torch.relu, R.lrelu

    def relu_r(x):
        inputs.append(x.detach())
        return relu(x)

    def lrelu_r(x, leak=0.2):
        inputs.append(x.detach())
        return lrelu(x, leak)
    torch.relu, R.lrelu = relu_r, lrelu_r
    try:
        yield
    finally:
        torch.relu, R.lrelu = relu, lrelu


@contextlib.contextmanager
def engine_masks(eng, cfg):
    """Within the block the reference's ReLU (G) and LeakyReLU (D) select their branch by the sign
    of the engine's activation instead of their own input's: the same values (the two differ only
    where the input is zero to within rounding) and, at such a kink, the engine's derivative. Only
    used for a step whose differing signs were shown to be kinks (see
    test_hip_d_spectral_norm.py::test_step_matches_reference)."""
    masks = engine_signs(eng, cfg)
    n_g = len(cfg.g_layers())
    it = iter(masks)
    relu, lrelu = torch.relu, R.lrelu

    def relu_m(x):
        return torch.where(next(it).reshape(x.shape), x, torch.zeros_like(x))

    def lrelu_m(x, leak=0.2):
        return torch.where(next(it).reshape(x.shape), x, leak * x)
    torch.relu, R.lrelu = relu_m, lrelu_m
    try:
        yield
        assert next(it, None) is None and n_g + len(cfg.d_layers()) == len(masks)  # every mask was used
    finally:
        torch.relu, R.lrelu = relu, lrelu


def sync_ref(ref_model, eng, sn):
    ref_model.g.flat.copy_(eng.model.g.flat)
    ref_model.d.flat.copy_(eng.model.d.flat)
    if sn:
        ref_model.d_sn.flat.copy_(eng.model.d_sn.flat)


def ref_for(cfg, dtype, seed, sn, **kw):
    rdev = torch.device("cpu") if dtype == "fp32" else dev
    ref_model = DCGAN(cfg, device=rdev, seed=seed)
    return ref_model, ReferenceStep(ref_model, d_spectral_norm=sn, seed=seed, **kw), rdev


def check_piece(eng, ref, ref_model, cfg, real, dtype, sn, full, run, tag):
    """Run one piece of the cycle on the engine (`run`: a D sub-step, or the full step) from the
    engine's own state and compare its losses, gradients and -- for D -- the parameters it wrote
    with the reference on the engine's z. full: compare G's gradients too.

    The comparisons are those of test_hip_d_spectral_norm.py::test_step_matches_reference: fp32 against
    the CPU reference, losses 1e-5, every live gradient 1e-3, activations at a kink compared on the
    engine's side after showing that they are kinks; bf16 losses 3e-2, gradients 0.25 (biases 0.35),
    mean 0.15; fp16 losses 2e-2, D 0.1, G 0.15. Parameters: the engine's new D weights are TF-Adam (fp32
    oracle, the tolerance of test_hip_kernels.py::test_adam_matches_tf_formula) of the engine's own
    gradient, which the gradient comparison ties to the reference's."""
    rdev = next(iter(ref_model.d.tensors.values())).device
    sync_ref(ref_model, eng, sn)
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
        with recording(ins):  # the unmodified reference
            out, gd, gg = grads()
        signs = engine_signs(eng, cfg)
        assert len(ins) == len(signs)
        at_kink = [x.flatten()[(m.flatten() != (x.flatten() > 0))].abs() for x, m in zip(ins, signs)]
        flips = sum(k.numel() for k in at_kink)
        far = max([float(k.max()) for k in at_kink if k.numel()], default=0.0)
        near = sum(int((x.abs() < KINK_MAX_INPUT).sum()) for x in ins)
        print("%s fp32: %d activation(s) with another sign than the reference's, largest |input| %.2e; %d reference "
              "inputs below %.0e" % (tag, flips, far, near, KINK_MAX_INPUT))
        assert flips <= near and far < KINK_MAX_INPUT, (tag, flips, near, far)
        if flips:  # the same piece on the engine's side of those kinks
            with engine_masks(eng, cfg):
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
        copies_match_state(eng)


# ------------------------------------------------------------------ one-rank RCCL DDP against the fused step
def op_names(eng):
    return {"ops": eng.op_names()}


class Ddp(NamedTuple):
    """A feature's one-rank DDP run. Every function is a top-level one of the feature's test module: the
    spawned rank unpickles this by reference."""
    engine: Callable[[bool], Any]               # graph -> an engine with its batches staged
    result: Callable[[Any], dict]               # engine -> CPU tensors, each bitwise the fused step's
    steps: int
    active: Optional[Callable[[Any], Any]] = None  # the feature is on in the rank's engine
    extras: Callable[[Any], dict] = op_names    # saved next to the result, for the test's own asserts


def rccl_worker(out_dir, ddp, schedule, graph, port):
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
    eng = ddp.engine(graph)
    assert eng.ddp and eng._schedule() == schedule
    assert ddp.active is None or ddp.active(eng)
    for _ in range(ddp.steps):
        eng.train_step()
    out = ddp.result(eng)
    out.update({"step": eng.global_step, "backend": tdist.get_backend(), "graph": eng.graph_enabled})
    out.update(ddp.extras(eng))
    torch.save(out, os.path.join(out_dir, "rccl.pt"))
    D.barrier()
    D.shutdown()


def fused_engine(ddp, env, graph=True):
    """The single-process engine of `ddp` after its steps, built and run with `env` out of the environment."""
    old = {k: os.environ.pop(k, None) for k in env}
    try:
        eng = ddp.engine(graph)
        assert not eng.ddp and eng._schedule() == "fused"
        for _ in range(ddp.steps):
            eng.train_step()
        return eng
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


def fused_result(ddp, env, graph=True):
    return ddp.result(fused_engine(ddp, env, graph))


def rccl_run(tmp_path, ddp, schedule, graph, fused):
    """One spawned rank under RCCL (joined before anything else runs): the right backend, step count and
    graph flag, and every tensor of `fused` bitwise. Returns what the rank saved."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=rccl_worker, args=(str(tmp_path), ddp, schedule, graph, free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == ddp.steps and r["graph"] == graph
    for k, v in fused.items():
        assert torch.equal(r[k], v), k
    return r


# ------------------------------------------------------------------ exact resume through the trainer
class Resume(NamedTuple):
    run: Callable      # (checkpoint dir, max_steps, feature flags = the test's) -> the run's output
    load: Callable     # (checkpoint dir, **engine keywords = the test's) -> (info, collected state, engine)
    made: list         # every source the runs built, in order (.i: batches drawn)
    texts: tuple       # the outputs of: the run in one go, the run up to the restart, the resumed run
    a: tuple           # load() of the run in one go
    b: tuple           # load() of the resumed run


def trainer_resume(tmp_path, monkeypatch, flags, load_kw=None, log_line=None, steps=(4, 2)):
    """bf16, 28x28x1, batch 8: `steps[0]` steps in one run (a) == `steps[1]` steps, a restart from the
    checkpoint, the rest (b) -- the same keys and every saved tensor bitwise. The first run prints
    `log_line`, the resumed one loaded the checkpoint at `steps[1]`."""
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

    def run(ck, n, extra=flags):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % n, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + list(extra))
        out = io.StringIO()
        assert T.run(fl, out=out) == 0, out.getvalue()
        return out.getvalue()

    def load(ck, **kw):
        from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
        eng = HipEngine(small(), 8, dev, seed=99, graph=False, **(kw or load_kw or {}))
        info = CK.CheckpointManager(str(ck)).restore_latest(eng)
        torch.cuda.synchronize()
        return info, CK.collect_state(eng), eng
    total, first = steps
    texts = (run(tmp_path / "a", total), run(tmp_path / "b", first), run(tmp_path / "b", total))
    assert log_line is None or log_line in texts[0]
    assert "load success!" in texts[2] and "global_step %d" % first in texts[2]
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    (ia, sa, _), (ib, sb, _) = a, b
    assert ia["global_step"] == ib["global_step"] == total and list(sa) == list(sb)
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    return Resume(run, load, made, texts, a, b)
