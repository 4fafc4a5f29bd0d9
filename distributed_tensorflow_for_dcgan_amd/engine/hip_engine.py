"""Fused HIP training engine: the whole reference DCGAN step on hand-written gfx950 kernels.

The step (``image_train.py:151-158`` semantics) is recorded ONCE into
native ``Program`` objects (``csrc/bindings.cpp``) over statically allocated buffers and replayed
every step from C++ (eager, the default) or as hipGraphs:

  progA[:a_fwd]  z ~ U(-1,1) (Philox, device step counter) -> G forward -> D forward on the 2B
                 batch [real | fake] with per-half BN statistics -> the 3 losses of the objective
                 (``gan_loss``: bce | lsgan | hinge) + both seeds, fused into the head GEMV; with
                 ``instance_noise`` one launch, ``d_noise``, between G and D writes the noisy copy
                 of [real | fake] that D's layer 0 reads (forward here, weight gradient in progB);
                 with ``d_augment`` one launch before it, ``d_aug``, writes the translated / cut-out
                 copy and its draws, and ``d_aug_bwd`` in the G chain takes the image gradient back;
                 with ``d_color_augment`` one launch before that, ``d_color``, writes the brightness /
                 saturation / contrast copy, and ``d_color_bwd`` follows ``d_aug_bwd`` in the G chain
  progA[a_fwd:]  the g_loss chain back through D(fake) and G's data gradients  -- "G chain"; with
                 ``g_topk`` < 1 its first op, ``g_topk``, keeps the seeds of the k(t) best-scored fakes
  progW          G's weight gradients, each tied to the progA position that produces its operand
  progB          D's backward of d_loss, both halves (D grads final)            -- "D chain"
  progC          TF-Adam(G), TF-Adam(D), beta powers, global step (+ 16-bit weight mirrors);
                 with ``g_ema_decay`` > 0 also ``ema_g``, the moving average of G's weights, after
                 the last Adam launch over G; with ``d_spectral_norm`` also ``sn_power`` (4 launches)
                 after the last Adam launch over D

With ``d_steps`` = n > 1 a training step is n - 1 D-only sub-steps, then the step above. Sub-step k
has Programs of its own (``_build_d_substeps``): the forward ops of progA[:a_fwd] on its own z seed
(``_zseed``) and its own [real_k | fake] staging buffer, with G's BN moving averages left alone; the
D chain; then ``progDU``: Adam(D) + mirror + D's beta powers (``adam1``: one launch on the
single-process bf16 step; else ``adam_bf`` + ``d_step_end``) and ``sn_power``. No G chain, no progW,
no Adam(G), no ``ema_g``, and the global step does not move.

With ``d_spectral_norm`` D's conv GEMMs and head read W / sigma(W) (the mirror slices / an fp32
copy of the head hold it) and progB projects each weight gradient back through sigma
(``sn_project``, 2 launches) right behind the launch that finalises it.

Schedules (``_schedule``), all proven free of cross-stream overlaps by ``schedule_check.py``:
  "fused"       one process: both chains on two streams, G weight gradients on a third, one
                Adam launch after the join
  "concurrent"  DDP default: the chains cut into segments with the gradient collectives issued
                between them on the comm stream (D's top layer first, g_h1's slice as soon as its
                weight gradient exists, the rest as each chain ends; bf16 wire without copies)
  "ddp"         the fused schedule with the collectives inside one hipGraph (native RCCL)
  "serial"      forward + G chain, then the D chain (the G all-reduce under D's backward)

Layouts: activations NHWC in the compute dtype; fp32 master weights in TF layout inside the flat
``ParamSet`` buffers (what checkpoints write and DDP reduces); 16-bit runs keep one mirror of every
weight in the same flat layout, which the GEMMs read in either orientation.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from ..models.config import DCGANConfig, same_pads
from ..models.dcgan import DCGAN
from ..optim.adam import TFAdam
from ..ops import hip as H
from ..ops import options as O
from ..ops import reference as R
from ..parallel import dist as D
from .hip_aux import HipEngineAux
from .hip_ddp import HipDDPMixin

RELU, LRELU, TANH, NONE = 1, 2, 3, 0
DTYPES = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16), "fp32": (2, torch.float32)}
SCHEDULES = ("fused", "ddp", "concurrent", "serial")
DDP_SCHEDULES = ("ddp", "concurrent", "serial")  # schedules that issue the gradient all-reduces


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else int(t.data_ptr())


def _kpad(c: int) -> int:
    return -(-25 * c // 16) * 16


_STREAMS: Dict[int, Tuple["torch.cuda.Stream", ...]] = {}


def _engine_streams(dev: torch.device):
    """The side / D-chain streams, created ONCE per device and process: HIP maps each new stream
    onto one of a few hardware queues in turn, so an engine built after many others could get its
    D-chain stream on the main stream's queue -- the two backward chains then serialise (seen as
    28 % slower steps every few engine builds in the in-situ tuner). Shared streams keep the first
    engine's mapping for every later one (engines of a process never run concurrently)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _STREAMS:
        _STREAMS[key] = tuple(torch.cuda.Stream(device=dev) for _ in range(3))
    return _STREAMS[key]


class _TorchExec:
    """Issues a schedule onto real HIP streams (torch.cuda.Stream objects)."""

    def __init__(self, eng: "HipEngine"):
        dev = eng.device
        self.dev = dev
        side, a0, a1 = _engine_streams(dev)
        self.side = side                 # slot 1 of main-stream segments
        self.alt = [a0, a1]              # D chain (+ its slot 1)
        self.comm = eng.comm_stream

    def main(self):
        return torch.cuda.current_stream(self.dev)

    @staticmethod
    def run(prog, streams, begin: int = 0, end: int = -1) -> None:
        H.run(prog, streams, begin, end)

    @staticmethod
    def wait(dst, src) -> None:
        """dst waits for everything queued on src so far."""
        dst.wait_stream(src)

    @staticmethod
    def mark(stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    @staticmethod
    def wait_mark(dst, ev) -> None:
        """dst waits for the work queued on the marked stream up to the mark."""
        dst.wait_event(ev)

    @staticmethod
    def collective(reducer, stream) -> None:
        with torch.cuda.stream(stream):
            reducer.issue()

    @staticmethod
    def replay(graph, stream) -> None:
        with torch.cuda.stream(stream):
            graph.replay()


class _DChain(NamedTuple):
    """One pass back through D (``HipEngine._d_backward``): the rows it covers and where its
    gradients go."""
    prefix: str                   # of its op names
    Bn: int                       # rows: 2B = [real | fake], B = the fake half
    groups: int                   # BN statistics groups among those rows ...
    group_offset: int             # ... from this one on (1: the fake half's statistics)
    view: Callable                # the chain's rows of a [2B, ...] forward buffer (d_x / d_a)
    da: Dict[str, torch.Tensor]   # its own buffers: per layer dL/d(activation),
    dx: Dict[str, torch.Tensor]   # dL/d(pre-activation)
    coef: Dict[str, torch.Tensor]  # and, per BN layer, the BN-backward coefficients
    dl: torch.Tensor              # the seed dL/dlogit
    grads: Optional[object]       # D's gradient set, or None: data gradients only


class _DStage(NamedTuple):
    """One stage between G's RGB layer and D's layer 0: a launch that writes a copy of [real | fake]
    of its own from the copy before it. It names engine attributes and holds no tensor: a buffer
    exists only while the stage's option is on (None otherwise) and keeps its one attribute path."""
    opt: str                            # the option that switches it on: self.<opt>.active
    out: str                            # its copy of [real | fake]
    name: str                           # its recorded name
    # a DiffAugment stage: its Jacobian is not the identity, so the launch records what its transpose
    # (Program.<op>_bwd, recorded as <name>_bwd on the g_loss chain) replays for the fake half
    op: Optional[str] = None            # Program.<op>
    params: Optional[str] = None        # its draws [2B][4] ...
    pdtype: Optional[torch.dtype] = None  # ... of this type
    gates: Optional[str] = None         # under adaptive augmentation, its gate masks int32 [2B]
    grad: Optional[str] = None          # the image gradient [B] behind its transpose


# in the order they run, the published one: color, then translation / cutout, then noise
D_STAGES = (
    _DStage("color", "d_colored", "d_color", "d_color", "color_params", torch.float32, "color_gates", "img_grad_c"),
    _DStage("aug", "d_auged", "d_aug", "d_augment", "aug_params", torch.int32, "aug_gates", "img_grad_t"),
    _DStage("noise", "d_noisy", "d_noise"),
)


class HipEngine(HipDDPMixin, HipEngineAux):
    name = "hip"
    dtype_name = "bf16"
    INIT_LOSS_SCALE = 32768.0   # fp16 dynamic loss scaling (TF/Keras LossScaleOptimizer defaults)
    LOSS_SCALE_GROWTH = 2000

    def __init__(self, cfg: DCGANConfig, batch_size: int, device: torch.device, dtype: str = "bf16",
                 seed: int = 0, lr: float = 2e-4, beta1: float = 0.5, zero_debias: bool = False, rank: int = 0,
                 world: int = 1, graph: bool = True, allreduce_dtype: str = "fp32", bucket_mb: float = 32.0,
                 rank_seeded_z: bool = True, schedule: Optional[str] = None, dry_run: bool = False,
                 ddp: Optional[bool] = None, z_seed: Optional[int] = None, **options):
        if dtype not in DTYPES:
            raise ValueError("HIP engine dtype must be one of %s" % sorted(DTYPES))
        self.dtype_name = dtype
        self.dt, self.edt = DTYPES[dtype]
        self.f16 = dtype == "fp16"
        self.f32 = dtype == "fp32"
        self.dry = bool(dry_run)  # record programs on the CPU for the schedule checker; never runs
        if device.type != "cuda" and not self.dry:
            raise ValueError("HipEngine needs a GPU (dry_run=True only records the step)")
        self.ext = H.ext()
        self.cfg = cfg
        self.B = int(batch_size)
        self.device = device
        self.rank, self.world = rank, world
        # data-parallel path (collectives on the comm stream, segmented step): any W > 1, or a
        # forced one-rank process group (DCGAN_FORCE_DDP=1 / ddp=True: RCCL on a one-GPU box)
        self.ddp = world > 1 or (D.ddp_forced() if ddp is None else bool(ddp))
        self.seed = int(seed)
        # seed of the in-kernel z stream (as ReferenceEngine's z_seed): None = the model seed
        self.z_seed = self.seed if z_seed is None else int(z_seed)
        self.rank_seeded_z = bool(rank_seeded_z)  # False only in equivalence tests
        # The training options (ops.options.TABLE), resolved once -- an explicit keyword, else (None) the
        # option's environment variable, else its default -- and published under their field names. Each
        # at its default: no buffer, launch or Program beyond the plain full step's.
        # d_steps, beta2, lr_d, lr_g: discriminator updates per generator update (d_steps - 1 recorded
        # D-only sub-steps before each full step), Adam's beta2 and the per-network learning rates.
        # lr_sched (ops.reference.LrSchedule): evaluated by every recorded Adam launch from the device step
        # counter: replays follow the live counter, a resume needs no new state. Off: the Adam ops are
        # recorded exactly as without it and never read the counter.
        # noise (ops.reference.InstanceNoise): D's layer 0 reads x + sigma(t) * eps, a noisy copy of
        # [real | fake] that one recorded launch (`d_noise`) writes from the device step counter; the
        # g_loss chain and G keep reading the clean fake.
        # aug, DiffAugment (ops.reference.DAugment): D sees augment([real | fake]), translation and / or
        # cutout per sample, which one recorded launch (`d_aug`) draws from stream 2 of the step's z seed
        # and the device step counter and writes, with its draws, behind G's RGB layer -- before the noise
        # when both are on. Its Jacobian is not the identity: the g_loss chain's image gradient passes
        # through the transposed gather (`d_aug_bwd`, from the recorded draws) before G's tanh backward,
        # which therefore runs unfused.
        # color, DiffAugment's color policy (ops.reference.DColor), a switch of its own: D sees noise(
        # geometric(color([real | fake]))), the published order. One recorded launch (`d_color`) ahead of
        # `d_aug` draws (b, s, c) per sample from stream 3 of the step's z seed and the device step counter
        # and writes the colored copy with (b, s, c, Mx); its Jacobian is a dense linear map per image,
        # which `d_color_bwd` applies transposed to the g_loss chain's image gradient, behind `d_aug_bwd`
        # and ahead of G's tanh backward.
        # ada, adaptive augmentation probability (ops.reference.DAda): each selected policy of the two
        # switches above applies to a sample with probability p = p24 * 2^-24. `d_color` / `d_aug` are then
        # recorded as their gated kernels, which read p24 from the device state `ada_state` and record the
        # per-sample gate masks that the two `_bwd` ops replay. With a target, one more recorded launch per
        # full step (`ada_update`, on the D chain's stream) steers p24 from the real half of the logits, so
        # graph and eager replays follow the live state with no host round trip. D sub-steps gate with the
        # live p24 and record no controller op. Off (p = 1, no target): the ungated kernels.
        # topk, top-k generator updates (ops.reference.GTopK): the g_loss chain's seed keeps the k(t) fakes
        # D scores highest, times B / k, and is +0 on the others; one recorded launch (`g_topk`), the first
        # op behind the forward on the G chain's stream, selects them from the logits and the device step
        # counter into buffers of its own. D's losses, seeds and chain are untouched, D sub-steps record
        # no such op.
        # g_ema_decay: moving average of G's weights (tf.train.ExponentialMovingAverage with num_updates =
        # the global step); 0 = off.
        # gan_loss, label_smooth: objective of the fused head / loss kernel: bce | lsgan | hinge, D's real
        # target = 1 - label_smooth.
        # d_spectral_norm: spectral normalisation of D's conv kernels and head: D computes with W /
        # sigma(W), one power-iteration step after each Adam(D).
        self.options = O.resolve(batch_size, lr=lr, beta1=beta1, **O.known(options))
        vars(self).update(self.options._asdict())
        if self.topk.active and batch_size > R.TOPK_MAX_B:
            raise ValueError("g_topk needs batch_size <= %d (the selection ranks one batch in one workgroup), "
                             "got %d" % (R.TOPK_MAX_B, batch_size))
        if self.g_ema_decay > 0 and os.environ.get("DCGAN_DDP_SHARD", "0") == "1":
            raise ValueError("g_ema_decay > 0 is not supported with DCGAN_DDP_SHARD=1: under the sharded update "
                             "each rank holds only 1/W of G's fp32 masters when the average would be taken")
        if self.d_spectral_norm and os.environ.get("DCGAN_DDP_SHARD", "0") == "1":
            raise ValueError("d_spectral_norm is not supported with DCGAN_DDP_SHARD=1: sigma needs the whole "
                             "matrix, and under the sharded update each rank holds only 1/W of D's fp32 masters")
        if schedule is None and os.environ.get("DCGAN_SERIAL_DBWD") == "1":
            schedule = "serial"
        if schedule is not None and schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s" % (SCHEDULES,))
        self._sched_req = schedule
        self._timing = False
        R.check_d_steps_schedule(self.d_steps, self._schedule(), os.environ.get("DCGAN_DDP_SHARD", "0") == "1")
        self.model = DCGAN(cfg, device=device, seed=seed, zero_debias=zero_debias)
        if self.d_spectral_norm:
            self.model.enable_d_spectral_norm(seed)  # fresh u (CPU generator) + one power step
        if self.ddp and not self.dry:
            D.broadcast_tensors([self.model.g.flat, self.model.d.flat, self.model.g_bn.flat, self.model.d_bn.flat]
                                + ([self.model.d_sn.flat] if self.d_spectral_norm else []))
        self.opt_d = TFAdam(self.model.d, self.lr_d, beta1, self.beta2, power_suffix="")
        self.opt_g = TFAdam(self.model.g, self.lr_g, beta1, self.beta2, power_suffix="_1")
        self.opt_d.use_hip = self.opt_g.use_hip = True
        self.grad_d = self.model.d.like()
        self.grad_g = self.model.g.like()
        self._step_host = 0
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=device)  # device global step
        self.graph_requested = bool(graph) and not self.dry
        self.graph_enabled = False
        self._timing = False
        self._graphs: List[Optional[torch.cuda.CUDAGraph]] = []
        self._sub_graphs: List[List[Optional[torch.cuda.CUDAGraph]]] = []  # per D sub-step, per segment
        self.comm_stream = torch.cuda.Stream(device=device) if (self.ddp and not self.dry) else None
        self.allreduce_dtype = allreduce_dtype
        # bf16 wire of the segmented DDP step (bf16 engine): flat bf16 gradient images that cast
        # kernels inside the step graphs fill, RCCL reduces in place and Adam reads directly
        self.wire_d = self.wire_g = None
        if self.ddp and allreduce_dtype == "bf16" and self.dt == 0:
            self.wire_d = self.model.d.like(torch.bfloat16)
            self.wire_g = self.model.g.like(torch.bfloat16)
        self.bucket_mb = bucket_mb
        self._exec = None
        self._alloc()
        if self.ada.active and self.ddp and not self.dry:
            D.broadcast_tensors([self.ada_state])  # rank 0's, as the parameters above
        self._build()
        if not self.dry:
            self._repack_weights_now()

    def _prog(self):
        return self.ext.Program(self.dt, self.dry)

    # ------------------------------------------------------------------ buffers
    def _t(self, *shape, dtype=None, zero=False):
        dtype = self.edt if dtype is None else dtype
        f = torch.zeros if zero else torch.empty
        return f(*shape, dtype=dtype, device=self.device)

    def _alloc(self):
        cfg, B = self.cfg, self.B
        B2 = 2 * B
        s = cfg.output_size
        self.gl = cfg.g_layers()
        self.dl = cfg.d_layers()
        t = self._t
        self.z = t(B, cfg.z_dim, dtype=torch.float32)
        self.sample_z = t(B, cfg.z_dim, dtype=torch.float32)
        # ---------------- G
        self.g_h0_pre = t(B, cfg.g_lin_out)
        self.g_h0 = t(B, cfg.g_lin_out)
        self.g_x = {}   # pre-BN deconv outputs
        self.g_a = {}   # activations (post BN+ReLU)
        for L in self.gl[:-1]:
            self.g_x[L.name] = t(B, L.out_hw, L.out_hw, L.cout)
            self.g_a[L.name] = t(B, L.out_hw, L.out_hw, L.cout)
        # ---------------- D input [real | fake]
        self.d_in = t(B2, s, s, cfg.c_dim, zero=True)
        self.fake = self.d_in[B:]
        # staging area of d_steps real batches: D sub-step k reads (and G writes the fake half of)
        # its own [real_k | fake] buffer; the last slot is the full step's d_in
        self.d_ins = [t(B2, s, s, cfg.c_dim, zero=True) for _ in range(self.d_steps - 1)] + [self.d_in]
        # the stages on D's input (D_STAGES), each switched on its own: the copy the next stage or D's
        # layer 0 reads. ONE buffer for the sub-steps and the full step: each ends with its D chain (the
        # last reader) joined back into the main stream, where the next forward rewrites it
        # (schedule_check proves it: tests/test_instance_noise.py). A DiffAugment stage also keeps the
        # draws [2B][4] its launch records -- int32 (ty, tx, oy, ox) of `d_aug`, float32 (b, s, c, Mx)
        # of `d_color` -- and, under adaptive augmentation, the gate masks int32 [2B] its gated kernel
        # records (the effective policy per sample). Allocated last stage first, the controller's state
        # ahead of the gates: the order these buffers have always been allocated in, so that every buffer
        # of the process, this engine's and any later one's, keeps the address it had
        for st in reversed(D_STAGES):
            on = getattr(self, st.opt).active
            setattr(self, st.out, torch.zeros_like(self.d_in) if on else None)
            if st.op:
                setattr(self, st.params, t(B2, 4, dtype=st.pdtype, zero=True) if on else None)
        # adaptive augmentation: the controller's state int32 [8] = (p24, acc, cnt, r_acc, windows, 0, 0, 0)
        self.ada_state = None
        if self.ada.active:
            self.ada_state = torch.tensor(R.ada_state(R.ada_p24(self.ada.p)), dtype=torch.int32, device=self.device)
        for st in reversed(D_STAGES):
            if st.op:
                on = getattr(self, st.opt).active and self.ada.active
                setattr(self, st.gates, t(B2, dtype=torch.int32, zero=True) if on else None)
        self.d_x, self.d_a = {}, {}
        for i, L in enumerate(self.dl):
            if L.bn:
                self.d_x[L.name] = t(B2, L.out_hw, L.out_hw, L.cout)
            self.d_a[L.name] = t(B2, L.out_hw, L.out_hw, L.cout)
        self.kp_d0 = _kpad(cfg.c_dim)
        self.d0_col = t(B2 * self.dl[0].out_hw ** 2, self.kp_d0)
        self.logits = t(B2, dtype=torch.float32)
        self.prob = t(B2, dtype=torch.float32)
        self.losses = t(4, dtype=torch.float32, zero=True)
        self.dl_d = t(B2, dtype=torch.float32)
        self.dl_g = t(B, dtype=torch.float32)
        # top-k generator updates: the g_loss chain's seed, the 0 / 1 selection and (g_loss_topk,
        # threshold, B / k, k), all written by `g_topk` alone
        self.dl_g_k = t(B, dtype=torch.float32, zero=True) if self.topk.active else None
        self.topk_sel = t(B, dtype=torch.int32, zero=True) if self.topk.active else None
        self.topk_info = t(4, dtype=torch.float32, zero=True) if self.topk.active else None
        # ---------------- BN state (fwd): mean/rstd/scale/shift per layer [groups][C]
        self.bn = {}
        for name, C in cfg.g_bn_layers():
            self.bn[name] = {k: t(1, C, dtype=torch.float32) for k in ("mean", "rstd", "scale", "shift")}
        for name, C in cfg.d_bn_layers():
            self.bn[name] = {k: t(2, C, dtype=torch.float32) for k in ("mean", "rstd", "scale", "shift")}
        # ---------------- backward buffers
        self.d_da = {L.name: t(B2, L.out_hw, L.out_hw, L.cout) for L in self.dl}
        self.d_dx = {L.name: t(B2, L.out_hw, L.out_hw, L.cout) for L in self.dl}
        # the g_loss chain back through D(fake) has its own gradient buffers (B rows), so it never
        # shares memory with D's d_loss backward (the two run concurrently)
        self.gc_da = {L.name: t(B, L.out_hw, L.out_hw, L.cout) for L in self.dl}
        self.gc_dx = {L.name: t(B, L.out_hw, L.out_hw, L.cout) for L in self.dl}
        self.img_grad = t(B, s, s, cfg.c_dim)
        self.img_g = t(B, s, s, cfg.c_dim)
        # ... and taken back through each DiffAugment stage's transpose (the fake half's rows), in the order it passes
        for st in reversed(D_STAGES):
            if st.grad:
                setattr(self, st.grad, t(B, s, s, cfg.c_dim) if getattr(self, st.opt).active else None)
        Lg = self.gl[-1]
        self.kp_g = _kpad(cfg.c_dim)
        self.g_last_col = t(B * Lg.in_hw ** 2, self.kp_g)
        self.g_da = {}
        self.g_dx = {}
        for L in self.gl[:-1]:
            self.g_da[L.name] = t(B, L.out_hw, L.out_hw, L.cout)
            self.g_dx[L.name] = t(B, L.out_hw, L.out_hw, L.cout)
        self.g_da0 = t(B, cfg.g_lin_out)
        self.g_dx0 = t(B, cfg.g_lin_out)
        self.coef = {name: t(2, C, 3, dtype=torch.float32) for name, C in cfg.d_bn_layers()}
        self.coef.update({name: t(1, C, 3, dtype=torch.float32) for name, C in cfg.g_bn_layers()})
        self.coef_g = {name: t(1, C, 3, dtype=torch.float32) for name, C in cfg.d_bn_layers()}
        # one column-sum scratch per chain: the two chains run concurrently
        self.small_part = {"d": t(64, 16, dtype=torch.float32), "g": t(64, 16, dtype=torch.float32)}
        # ---------------- weights the GEMMs read: 16-bit mirrors in the SAME flat layout as the
        # fp32 masters (TF layouts: HWIO conv, [kh,kw,out,in] deconv), written by the Adam kernel;
        # fp32 runs read the masters themselves
        if self.f32:
            # (with spectral norm the conv GEMMs read W / sigma: a separate fp32 copy of D, of
            # which only the "/w" slices are written and read)
            self.wbf_d = self.model.d.like() if self.d_spectral_norm else self.model.d
            self.wbf_g = self.model.g
        else:
            self.wbf_d = self.model.d.like(self.edt)
            self.wbf_g = self.model.g.like(self.edt)
        # moving average of G's weights (same flat layout, padding included) + the 16-bit mirror of
        # it that the sampler's conv GEMMs read (fp32: they read the average itself)
        self.g_ema = self.wbf_g_ema = None
        if self.g_ema_decay > 0:
            self.g_ema = self.model.g.like()
            self.g_ema.flat.copy_(self.model.g.flat)
            self.wbf_g_ema = self.g_ema if self.f32 else self.model.g.like(self.edt)
            self.model.g_ema = self.g_ema  # (what DCGAN.sampler(ema=True) and the checkpoints see)
        # spectral norm: the head's normalised fp32 copy, one workspace per weight and the kernels'
        # descriptor tuples (W, u, v, sigma, ws, copy, copy is fp32, gradient, K, Cout)
        self.sn_head = None
        self._sn_mats: Dict[str, tuple] = {}
        if self.d_spectral_norm:
            sn = self.model.d_sn
            self.sn_head = t(cfg.d_lin_in, dtype=torch.float32, zero=True)
            self._sn_ws = {}
            for name, K, C in sn.shapes:
                self._sn_ws[name] = t(self.ext.sn_plan(K, C)[4], dtype=torch.float32, zero=True)
                head = name.endswith("/Matrix")
                hat = self.sn_head if head else self.wbf_d[name]
                self._sn_mats[name] = (_p(self.model.d[name]), _p(sn.u[name]), _p(sn.v[name]), _p(sn.sigma[name]),
                                       _p(self._sn_ws[name]), _p(hat), int(head), _p(self.grad_d[name]), K, C)
        # fp16: dynamic loss scale state [scale, overflow flag, good steps] (device-resident, so
        # the whole step incl. skip / halve / grow stays inside the captured graphs)
        self.loss_scale = (torch.tensor([self.INIT_LOSS_SCALE, 0.0, 0.0], dtype=torch.float32, device=self.device)
                           if self.f16 else None)
        # sampler zero-debias factor 1 / (1 - decay^t) (device scalar, set before each sampler run)
        self._debias = torch.ones(1, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ program build
    def _stats_buf(self, key, P, C):
        buf = self._t(P, 2, C, dtype=torch.float32)
        self._keep.append(buf)
        return buf

    def _build(self):
        self._keep: List[torch.Tensor] = []
        self.progA = self._prog()
        self.progB = self._prog()
        self.progW = self._prog()  # G's weight gradients (see _build_gloss_and_g_backward)
        self._g_w: List[Tuple[int, int]] = []
        self._g_w_layer: List[str] = []
        self._build_forward(self.progA, update_ema=True, z=self.z, train_z=True)
        self._a_fwd = self.progA.size()  # forward done: D's d_loss backward may start from here
        self._build_gloss_and_g_backward(self.progA, self.progW)
        self._build_d_backward_dloss(self.progB)  # sets self._b_split (top layer done)
        # adaptive augmentation: the controller, one op on the D chain's stream (behind the head launch that
        # wrote the logits, off the G chain's critical path): behind the chain in the fused step, ahead of
        # it in the DDP schedules (_ada_at_tail). A program of its own: the D sub-steps share progB's
        # layout and record no controller op
        self.progAda = None
        if self.ada.adaptive:
            self.progAda = self._prog()
            a, B = self.ada, self.B
            self.progAda.ada_update("ada_update", _p(self.logits), B, _p(self.ada_state),
                                    R.ada_threshold(self.gan_loss, self.label_smooth),
                                    R.ada_target_n(a.target, B, a.interval),
                                    R.ada_delta24(self.world, B, a.interval, a.kimg), a.interval, 0)
        # D-gradient slice final after the D chain's first segment: the top conv layer (+ its BN)
        # and the head, which the ParamSet lays out last
        self._d_top_off = self.model.d.offsets[self.dl[-1].name + "/w"][0]
        self._g_cuts = self._g_bucket_cuts()
        self._g_split = self._g_split_plan()
        self._build_shards()
        self._build_d_substeps()
        self._build_updates()  # (after the G split: Adam(G) follows its collectives)
        self.progX, self._wire_ops = self._prog(), {}
        if self.wire_d is not None:  # fp32 gradient slice -> its bf16 wire image, one op per collective
            o = self._d_top_off
            nd, ng = self.grad_d.flat.numel(), self.grad_g.flat.numel()
            lo, hi = self._g_split[3:] if self._g_split is not None else (0, ng)
            for name, src, dst, a, b in (("dtop", self.grad_d, self.wire_d, o, nd), ("drest", self.grad_d, self.wire_d, 0, o),
                                         ("g", self.grad_g, self.wire_g, 0, ng), ("g_a", self.grad_g, self.wire_g, lo, hi),
                                         ("g_b", self.grad_g, self.wire_g, hi, ng), ("g_c", self.grad_g, self.wire_g, 0, lo)):
                if b > a:
                    self._wire_ops[name] = self.progX.size()
                    self.progX.cast_to_bf16("wire." + name, _p(src.flat) + 4 * a, 0, _p(dst.flat) + 2 * a, b - a,
                                            1.0, 0.0, 0)
        self.progCast = self._prog()  # fp32 masters -> 16-bit mirrors (init / checkpoint load)
        if not self.f32:
            pairs = [(self.model.d, self.wbf_d), (self.model.g, self.wbf_g)]
            if self.g_ema is not None:
                pairs.append((self.g_ema, self.wbf_g_ema))
            for ps, pb in pairs:
                self.progCast.cast_to_bf16("mirror", _p(ps.flat), 0, _p(pb.flat), ps.flat.numel(), 1.0, 0.0, 0)
        if self.d_spectral_norm:  # the normalised copies from the stored sigma (no iteration)
            self.progCast.sn_apply("sn_copy", list(self._sn_mats.values()), 0)
        self.progS = self.progS_ema = None  # sampler programs (weights / their moving average), built lazily
        self.progEval = None
        self.progSum = None

    def _build_d_substeps(self):
        """d_steps > 1: the d_steps - 1 D-only sub-steps, each a forward program (the full step's
        forward ops on sub-step k's z seed and [real_k | fake] buffer; G's BN moving averages are
        left alone, D's update) and a D chain (``_build_d_backward_dloss``, cut at the same position
        as progB for the DDP collectives). No G chain, no progW. The update (``progDU``) is shared."""
        self._sub: List[Tuple[object, object]] = []
        keep = (self._b_split, self._b_top_dgrad)
        for k in range(self.d_steps - 1):
            pf, pb = self._prog(), self._prog()
            self._build_forward(pf, update_ema=True, z=self.z, train_z=True, update_ema_g=False, sub=k)
            self._build_d_backward_dloss(pb, sub=k)
            assert (self._b_split, self._b_top_dgrad) == keep and pb.size() == self.progB.size()
            self._sub.append((pf, pb))
        self._b_split, self._b_top_dgrad = keep

    def _d_update_fused(self) -> bool:
        """The sub-step's D update as ONE launch (adam1: Adam + mirror + D's powers) on the
        single-process bf16 step, where the full step uses adam2; DCGAN_D_UPDATE=split: adam_bf +
        d_step_end there too (A/B)."""
        return (self._schedule() == "fused" and self.dt == 0
                and (os.environ.get("DCGAN_D_UPDATE") or "fused") != "split")

    def _build_d_update(self):
        """progDU, the D sub-step's update after the D chain (and, under DDP, D's collectives):
        Adam(D) + mirror + D's beta powers, then the power step. fp16: the overflow check over D's
        gradient gates Adam, the powers and sn_power, and d_step_end applies the loss-scale rule."""
        self.progDU = None
        if self.d_steps <= 1:
            return
        prog = self.progDU = self._prog()
        od, Dm = self.opt_d, self.model.d
        n = Dm.flat.numel()
        gs = 1.0 / self.world
        if self._d_update_fused():
            prog.adam1("adam_d1", _p(Dm.flat), _p(self.wbf_d.flat), _p(self.grad_d.flat), _p(od.m.flat), _p(od.v.flat),
                       _p(od.powers), n, od.lr, od.beta1, od.beta2, od.eps, gs, 0, **self._lr_kw())
            self._sn_power(prog)
            return
        ls = _p(self.loss_scale)
        if self.f16:
            prog.nonfinite_check("ls.check_d", _p(self.grad_d.flat), n, ls, 0)
        self._adam(prog, "adam_d", "d", ls=ls, wire=self._wire_direct())
        self._sn_power(prog, ls)
        # a sub-step's step_end: D's powers and the loss-scale rule, never G's powers or the global step
        prog.step_end("d_step_end", _p(od.powers), 0, od.beta1, od.beta2, 0.0, 0.0, 0, 0, ls, self.LOSS_SCALE_GROWTH)

    def _build_updates(self):
        """progC for the current schedule. The one-launch Adam over BOTH models is only used
        where nothing else can be touching D's gradients or weights any more ("fused": after
        the join of the two backward chains). "serial" runs Adam(G) first (progC[:_c_split],
        overlapping D's all-reduces), then Adam(D) + the step counter; "concurrent" -- whose D
        chain ends first -- runs Adam(D) first (overlapping G's all-reduce), then Adam(G) + the
        step counter ("ddp" likewise). fp16: one overflow check gates both, everything in the
        second part."""
        self.progC = self._prog()
        self._build_d_update()
        sch = self._schedule()
        if self._sharded():
            self._build_update_sharded(self.progC)
            self._c_split = self._c_split_a = self.progC.size()
        elif sch == "fused" and self.dt == 0:
            self._build_update_fused(self.progC)
            self._c_split = self._c_split_a = self.progC.size()
        elif sch in ("concurrent", "ddp") and not self.f16:
            self._build_update_d_first(self.progC)
        else:
            self._build_update(self.progC, first=True)
            self._c_split = self._c_split_a = self.progC.size()
            self._build_update(self.progC, first=False)


    # ---- helpers
    def _igemm(self, prog, name, shape, A, Bw, C, pad, out_f32=False, ldc=None, cofs=0, bias=None, act=NONE,
               stats=None, rows_per_group=None, kb_valid=-1, bnb=None, stream=0):
        """One conv-shaped GEMM (shape: ops.hip.GemmShape). Bw is a weight view; shape.bkn reads it as
        [tap][K][N] (D forward, G dgrad, im2col'd layers), else as [tap][N][K]. bnb = (x, y, mean,
        rstd, rows_per_group, act[, store_g]): the epilogue also emits the BN-backward partial sums
        of the layer whose dL/da this GEMM produces (see _dgrad)."""
        plan = shape.plan(rows_per_group, self.dt)
        if plan is None:
            raise RuntimeError("no igemm tile for %s (mode %d, N %d, bkn %d)" % (name, shape.mode, shape.N, shape.bkn))
        cfg, splits = plan
        bx = by = bm = br = 0
        brpg = bact = bstore = 0
        if bnb is not None:
            bx, by, bm, br = _p(bnb[0]), _p(bnb[1]), _p(bnb[2]), _p(bnb[3])
            brpg, bact = bnb[4], bnb[5]
            bstore = int(len(bnb) > 6 and bnb[6])
        prog.igemm_ex(name, shape.mode, _p(A), _p(Bw), _p(C), *shape[1:8], pad, pad, cfg, int(out_f32),
                      ldc or shape.N, cofs, _p(bias), act, self.cfg.lrelu_leak, _p(stats), stream, int(shape.bkn),
                      kb_valid, splits, bx, by, bm, br, brpg, bact, self.cfg.lrelu_leak, bstore)
        return cfg

    def _dgrad(self, prog, name, shape, A, Bw, pad, act, y, da, bn=None, x=None, dx=None, actb=None, groups=1,
               group_offset=0, kb_valid=-1):
        """The data-gradient GEMM that produces dL/da of the layer below (activation output y, same
        layout as the GEMM output), with that layer's backward fused into the store pass when a tile
        allows. Returns (partials, partials per group) for the layer's backward, or None: the plain
        GEMM wrote da and the layer runs its own statistics / activation pass (always in fp32).

        Layer below has BN `bn` (x = its pre-BN input): the epilogue emits the BN-backward statistics
        into a fresh `<bn>.bwd` buffer, per group (`groups` row groups from `group_offset`), and dL/da
        goes to da. The tile must divide a group, so the plan is asked with rows_per_group, and a
        deconv with an odd output is never fused: its four phases have different row counts, and no
        group size divides them all (igemm_ex checks it per phase). (The BN-backward finalize stays
        a separate kernel: fusing it into the GEMM through a per-workgroup arrival measured slower,
        profiles/r2/ab_fused_finalize_r2.txt.)

        No BN: the GEMM stores dx = dL/da * act'(y) itself and emits per-tile column sums of dx (the
        bias gradient) into `<actb>.actb`. Nothing is grouped, so any tile serves (the plan is asked
        without rows_per_group) and odd deconv sizes only round the partial rows up."""
        rpg = None
        fits = not self.f32
        if bn is not None:
            fits = fits and not (shape.mode == 1 and (shape.Hout % 2 or shape.Wout % 2))
            rpg = shape.M // groups
        plan = shape.plan(rpg, self.dt) if fits else None
        if plan is None or shape.N % 8 or not H.bnb_fits(plan[0]):
            self._igemm(prog, name, shape, A, Bw, da, pad, kb_valid=kb_valid)
            return None
        P = shape.stat_rows(plan[0], self.dt)
        if bn is not None:
            part = self._stats_buf(bn + ".bwd", P, shape.N)
            st = self.bn[bn]
            bnb = (x, y, st["mean"][group_offset:], st["rstd"][group_offset:], rpg, act)
            self._igemm(prog, name, shape, A, Bw, da, pad, stats=part, rows_per_group=rpg, kb_valid=kb_valid, bnb=bnb)
            return part, P // groups
        part = self._stats_buf(actb + ".actb", P, shape.N)
        bnb = (y, y, None, None, 0, act, True)
        self._igemm(prog, name, shape, A, Bw, dx, pad, stats=part, kb_valid=kb_valid, bnb=bnb)
        return part, P

    def _deconv_out(self, prog, name, x, w, y, B, L, pad, bias, act):
        """G's output layer: the direct narrow kernel for RGB / gray outputs (16-bit), else the
        implicit GEMM."""
        if not self.f32 and L.cout <= 4 and L.cin % 8 == 0 and L.cin <= 256:
            prog.narrow_deconv(name, _p(x), _p(w), _p(bias), _p(y), B, L.in_hw, L.in_hw, L.cin, L.out_hw, L.out_hw,
                               L.cout, pad, act, self.cfg.lrelu_leak, 0)
        else:
            self._igemm(prog, name, H.GemmShape.fwd(L, B), x, w, y, pad, bias=bias, act=act)

    def _bn_fwd(self, prog, name, x, y, rows, C, groups, act, part, ppg, update_ema, apply=True):
        """BN finalize (+EMA) and apply+act over `groups` row groups (apply=False: the consumer
        applies it, e.g. the head)."""
        cfgm = self.cfg
        st = self.bn[name]
        bnstate = self.model.d_bn if name.startswith("d_") else self.model.g_bn
        P = self.model.d if name.startswith("d_") else self.model.g
        ema_m = bnstate.mean[name] if update_ema else None
        ema_v = bnstate.var[name] if update_ema else None
        prog.bn_finalize(name + ".fin", _p(part), ppg, groups, C, float(rows // groups), _p(P[name + "/gamma"]),
                         _p(P[name + "/beta"]), cfgm.bn_eps, _p(st["mean"]), _p(st["rstd"]), _p(st["scale"]),
                         _p(st["shift"]), _p(ema_m), _p(ema_v), cfgm.bn_momentum, 0)
        if apply:
            prog.bn_apply_act(name + ".apply", _p(x), _p(y), _p(st["scale"]), _p(st["shift"]), rows, C,
                              rows // groups, act, cfgm.lrelu_leak, 0)

    @staticmethod
    def _rows_per_block(rows_per_group: int, C: int) -> int:
        """Rows per column-reduction block: a divisor of rows_per_group (blocks never straddle
        a BN group), as large as possible while keeping >= 256 blocks per group (fill the CUs)."""
        for rpb in (256, 128, 64, 32, 16, 8, 4, 2, 1):
            if rows_per_group % rpb == 0 and (rows_per_group // rpb >= 256 or rpb == 1):
                return rpb
        return 1

    def _gout_applies_bn(self) -> bool:
        """G's RGB layer (narrow MFMA kernel) applies the BN + ReLU of the layer below itself."""
        L = self.gl[-1]
        return (not self.f32 and len(self.gl) > 1 and bool(self.gl[-2].bn) and L.cout <= 4 and L.cin == 64
                and L.out_hw == 2 * L.in_hw)

    def _head_applies_bn(self) -> bool:
        """The D head GEMV applies the top BN layer's BN + LeakyReLU itself (16-bit builds)."""
        L = self.dl[-1]
        return not self.f32 and bool(L.bn) and L.cout % 8 == 0 and 512 % L.cout == 0 and self.cfg.d_lin_in % 2048 == 0

    def _img_dact(self) -> bool:
        """D layer 0's image gradient (g_loss chain) with G's tanh backward + bias gradient fused
        (narrow.hip DACT): 16-bit, 64-channel D layer 0, <= 4 image channels. Not under DiffAugment
        (either switch): the image gradient is then taken at the augmented pixels, tanh' at the clean ones."""
        L = self.dl[0]
        return not self._d_stages(transposed=True) and not self.f32 and L.cin <= 4 and L.cout == 64 and self.gl[-1].cout == L.cin

    def _g_out_direct(self) -> bool:
        """G's 1..4-channel output layer backward on narrow2.hip (nconv data gradient + nwgrad)."""
        L = self.gl[-1]
        return (not self.f32 and L.cout <= 4 and L.cin == 64
                and self.progA.nwgrad_ok(L.out_hw, L.out_hw, L.in_hw, L.in_hw))

    def _d0_direct(self) -> bool:
        """D layer 0 forward on the direct conv3 kernel (16-bit, Cin <= 4, Cout = 64) instead of
        im2col + GEMM."""
        L = self.dl[0]
        return not self.f32 and L.cin <= 4 and L.cout == 64

    def _head_w(self) -> torch.Tensor:
        """The head's weight as the step reads it: the fp32 master, or its normalised copy."""
        return self.sn_head if self.d_spectral_norm else self.model.d[self.cfg.d_lin_name + "/Matrix"]

    def _sn_project(self, prog, names) -> None:
        """Spectral norm: project the finished gradients of `names` (dL/d(W / sigma), as the step's
        kernels produce them) back to dL/dW, in place -- right behind the launch that finalises
        them, so the wire casts, collectives, the nonfinite check and Adam see dL/dW."""
        if self.d_spectral_norm:
            prog.sn_project("sn_project." + names[0].split("/")[0], [self._sn_mats[n] for n in names], 0)

    def _sn_power(self, prog, ls: int = 0) -> None:
        """Spectral norm: one power step on the weights Adam(D) just wrote + the normalised copies
        (over the mirror slices that Adam wrote), on Adam(D)'s stream, before step_end clears the
        fp16 overflow flag (an overflowed step skips it, as it skips Adam)."""
        if self.d_spectral_norm:
            prog.sn_power("sn_power", list(self._sn_mats.values()), ls, 0)

    # ---- forward
    def _zseed(self, sub: Optional[int] = None) -> int:
        """Seed of the in-kernel z stream (Philox keyed by it and the device step counter):
        zseed = z_seed * 1000003 + 17 + 7919 * rank for the full step; D sub-step k, during which the
        step counter does not move, draws from zseed_k = (zseed + (k + 1) * 0x9E3779B97F4A7C15) mod
        2^64 (a fixed odd multiplier: the d_steps seeds of a step are pairwise different). No state:
        a resumed run draws the same z sequence."""
        zseed = self.z_seed * 1000003 + 17 + 7919 * self.rank * int(self.rank_seeded_z)
        if sub is None:
            return zseed
        return (zseed + (sub + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF

    def _d_stages(self, transposed: bool = False) -> List[_DStage]:
        """The stages on D's input that are switched on, in the order they run. transposed: those among
        them with a transpose, in the order the g_loss chain's image gradient passes back through them."""
        on = [st for st in D_STAGES if getattr(self, st.opt).active]
        return [st for st in reversed(on) if st.grad] if transposed else on

    def _d_input(self, sub: Optional[int] = None, noise: bool = True) -> torch.Tensor:
        """What D's layer 0 reads (forward and weight gradient): [real | fake] of the full step or
        of D sub-step `sub`, or its perturbed copy: the output of the last stage that is on (each
        stage reads the one before it: the noise lands on the augmented copy when both are on).
        noise=False: the clean input whatever is switched on."""
        stages = self._d_stages() if noise else []
        if stages:
            return getattr(self, stages[-1].out)
        return self.d_in if sub is None else self.d_ins[sub]

    def noise_sigma(self) -> float:
        """sigma(t) of the instance noise at the current global step (0.0 when off)."""
        n = self.noise
        return float(R.noise_sigma(self.global_step, n.sigma0, n.sigma1, n.steps)) if n.active else 0.0

    def _build_forward(self, prog, update_ema: bool, z, train_z: bool, update_ema_g: Optional[bool] = None,
                       sub: Optional[int] = None, noise: bool = True):
        """update_ema: D's BN moving averages; update_ema_g: G's (None = as D's). sub = k: the forward
        of D sub-step k -- its z seed and its [real_k | fake] buffer, the same ops otherwise. noise:
        with DiffAugment / instance noise on, record `d_aug` / `d_noise` and let D's layer 0 read the
        perturbed copy (False: the sample-time losses, which stay clean of both)."""
        cfg, B = self.cfg, self.B
        B2 = 2 * B
        Pg, Pd = self.model.g, self.model.d
        zseed = self._zseed(sub)
        if update_ema_g is None:
            update_ema_g = update_ema
        d_in = self.d_in if sub is None else self.d_ins[sub]
        fake = d_in[B:]
        # G projection + g_bn0 + relu; train_z: z ~ U(-1,1) generated inside the projection kernel
        # (Philox keyed by the device step counter); g_bn0 partial statistics straight from it:
        # one partial row per (8-row block of z, spatial position) -- see linear_fwd_kernel
        C0 = cfg.g_base_ch
        rows0 = B * cfg.g_base_hw ** 2
        P0 = -(-B // 8) * (cfg.g_lin_out // C0)
        part0 = self._stats_buf("g_bn0", P0, C0)
        prog.linear_fwd("g_h0_lin", _p(z), _p(Pg["g_h0_lin/Matrix"]), _p(Pg["g_h0_lin/bias"]), _p(self.g_h0_pre),
                        B, cfg.z_dim, cfg.g_lin_out, 0, _p(part0), C0,
                        _p(self.step_counter) if train_z else 0, zseed if train_z else 0)
        self._bn_fwd(prog, "g_bn0", self.g_h0_pre, self.g_h0, rows0, C0, 1, RELU, part0, P0, update_ema_g)
        a_prev = self.g_h0
        Wg, Wd = self.wbf_g, self.wbf_d
        for L in self.gl:
            nat = Wg[L.name + "/w"]  # [5,5,co,ci] = [tap][N][K]
            pad = same_pads(L.out_hw)[0]
            if L.bn:
                shape = H.GemmShape.fwd(L, B)
                P = shape.stat_rows(shape.plan(None, self.dt)[0], self.dt)
                part = self._stats_buf(L.bn, P, L.cout)
                rows = B * L.out_hw ** 2
                self._igemm(prog, L.name, shape, a_prev, nat, self.g_x[L.name], pad, bias=Pg[L.name + "/biases"],
                            stats=part)
                out_applies = L is self.gl[-2] and self._gout_applies_bn()
                self._bn_fwd(prog, L.bn, self.g_x[L.name], self.g_a[L.name], rows, L.cout, 1, RELU, part, P,
                             update_ema_g, apply=not out_applies)
                a_prev = self.g_a[L.name]
            elif self._gout_applies_bn():
                # RGB layer: the lower layer's BN apply + ReLU in its halo staging (writes that
                # activation), + bias, tanh into the fake half of D's input
                Lp = self.gl[-2]
                st = self.bn[Lp.bn]
                prog.narrow_deconv_bnin(L.name + "+bn_apply", _p(self.g_x[Lp.name]), _p(nat), _p(Pg[L.name + "/biases"]),
                                        _p(fake), B, L.in_hw, L.in_hw, L.cin, L.out_hw, L.out_hw, L.cout, pad,
                                        TANH, cfg.lrelu_leak, _p(st["scale"]), _p(st["shift"]), RELU, cfg.lrelu_leak,
                                        _p(self.g_a[Lp.name]), 0)
            else:  # last: + bias, tanh, written into the fake half of D's input
                self._deconv_out(prog, L.name, a_prev, nat, fake, B, L, pad, Pg[L.name + "/biases"], TANH)
        # D forward on [real | fake]; DiffAugment / instance noise: on its augmented / noisy copy,
        # written here -- behind the op that wrote the fake half, on the main stream -- from streams
        # 2 / 1 of the step's z seed; the noise lands on the augmented copy when both are on. The color
        # policy (stream 3) comes first: color, then translation / cutout, then noise
        prev = d_in
        for st in self._d_stages() if noise else []:
            dst = getattr(self, st.out)
            if st.op:
                # (adaptive augmentation: the gated kernels, gates from streams 5 / 4 against the live p24)
                gate = dict(gates=_p(getattr(self, st.gates)), ada_state=_p(self.ada_state)) if self.ada.active else {}
                getattr(prog, st.op)(st.name, _p(prev), _p(dst), _p(getattr(self, st.params)), B2, cfg.output_size,
                                     cfg.c_dim, getattr(self, st.opt).mask, zseed, _p(self.step_counter), 0, **gate)
            else:
                prog.instance_noise(st.name, _p(prev), _p(dst), d_in.numel(), zseed, _p(self.step_counter),
                                    R.NOISE_STREAM, self.noise.sigma0, self.noise.sigma1, self.noise.steps, 0)
            prev = dst
        for i, L in enumerate(self.dl):
            w = Wd[L.name + "/w"]  # HWIO [5,5,ci,co] = [tap][K][N]
            pad = same_pads(L.in_hw)[0]
            rows = B2 * L.out_hw ** 2
            shape = H.GemmShape.fwd(L, B2)
            if i == 0 and self._d0_direct():  # persistent direct MFMA conv, no column matrix (narrow2.hip)
                prog.nconv("d0.nconv", _p(prev), _p(w), _p(Pd[L.name + "/biases"]), _p(self.d_a[L.name]), B2,
                           L.in_hw, L.in_hw, L.cin, L.out_hw, L.out_hw, pad, pad, LRELU, cfg.lrelu_leak,
                           H.nconv_grid(prog, B2, L.out_hw, L.out_hw), 0, 0, 0, 0, 0, 0.0, 0, 0)
            elif i == 0 and L.cin % 8 != 0:
                prog.im2col_s2("d0.im2col", _p(prev), _p(self.d0_col), B2, L.in_hw, L.in_hw, L.cin, L.out_hw,
                               L.out_hw, pad, pad, self.kp_d0, 0)
                self._igemm(prog, L.name, H.GemmShape(2, B2, 1, 1, self.kp_d0, L.out_hw, L.out_hw, L.cout, True),
                            self.d0_col, w, self.d_a[L.name], 0, bias=Pd[L.name + "/biases"], act=LRELU,
                            kb_valid=25 * L.cin)
            elif not L.bn:
                self._igemm(prog, L.name, shape, prev, w, self.d_a[L.name], pad, bias=Pd[L.name + "/biases"], act=LRELU)
            else:
                rpg = B * L.out_hw ** 2
                plan = shape.plan(rpg, self.dt)
                if plan is not None:
                    # BN partial statistics straight from the conv epilogue (tiles never straddle
                    # the real/fake boundary)
                    P = shape.stat_rows(plan[0], self.dt)
                    part = self._stats_buf(L.bn, P, L.cout)
                    self._igemm(prog, L.name, shape, prev, w, self.d_x[L.name], pad, bias=Pd[L.name + "/biases"],
                                stats=part, rows_per_group=rpg)
                else:  # odd sizes: no tile divides the group -> separate group-aligned stats pass
                    self._igemm(prog, L.name, shape, prev, w, self.d_x[L.name], pad, bias=Pd[L.name + "/biases"])
                    rpb = self._rows_per_block(rpg, L.cout)
                    P = rows // rpb
                    part = self._stats_buf(L.bn, P, L.cout)
                    prog.colstats(L.bn + ".stats", 0, _p(self.d_x[L.name]), 0, 0, 0, 0, 0, 0.0, rows, L.cout, rpb,
                                  rpg, _p(part), 0)
                head_bn = i == len(self.dl) - 1 and self._head_applies_bn()
                self._bn_fwd(prog, L.bn, self.d_x[L.name], self.d_a[L.name], rows, L.cout, 2, LRELU, part, P // 2,
                             update_ema, apply=not head_bn)
            prev = self.d_a[L.name]
        lin = cfg.d_lin_name
        last = self.dl[-1]
        obj = H.GAN_LOSS_IDS[self.gan_loss]
        if last.bn and self._head_applies_bn():
            # head GEMV with the top BN layer's apply + LeakyReLU fused (writes its activation) + the
            # fused 3 losses of the objective in its last-arriving block
            st = self.bn[last.bn]
            prog.gemv_head_bn("d_head+bn_apply+loss", _p(self.d_x[last.name]), _p(self._head_w()),
                              _p(Pd[lin + "/bias"]), _p(self.logits), B2, cfg.d_lin_in, 0, _p(self.losses),
                              _p(self.dl_d), _p(self.dl_g), _p(self.prob), _p(self.loss_scale), _p(st["scale"]),
                              _p(st["shift"]), last.cout, B, LRELU, cfg.lrelu_leak, _p(self.d_a[last.name]),
                              obj, self.label_smooth)
        else:
            # head GEMV + the fused 3 losses of the objective in its last-arriving block
            prog.gemv_head("d_head+loss", _p(prev), _p(self._head_w()), _p(Pd[lin + "/bias"]), _p(self.logits),
                           B2, cfg.d_lin_in, 0, _p(self.losses), _p(self.dl_d), _p(self.dl_g), _p(self.prob),
                           _p(self.loss_scale), obj, self.label_smooth)

    # ---- the pass back through D: the d_loss chain (2B rows, all D gradients) and the g_loss chain
    def _d_backward(self, prog, ch: "_DChain", wgrad=None) -> int:
        """One walk back through D over the rows of chain `ch`: the head backward with the top BN
        layer's statistics fused in, then per layer its BN backward / bias sum from fused partials /
        activation backward, wgrad(i, L, dx) when given (the chain's weight-gradient step), and the
        data gradient into the layer below (_dgrad). ch.grads None: data gradients only. Ends with
        ch.dx of layer 0; returns the position behind the top layer's data gradient (the chain's last
        read of the top layer's kernel)."""
        Pd, g, leak = self.model.d, ch.grads, self.cfg.lrelu_leak
        lin, last, n = self.cfg.d_lin_name, self.dl[-1], len(self.dl)
        # fused: BN-backward partials emitted by the layer above (head / dgrad GEMM store pass)
        xa, dW, db = (None, None, None) if g is None else (self.d_a[last.name], g[lin + "/Matrix"], g[lin + "/bias"])
        fused = self._head_bwd(prog, ch.prefix + ("d_head.dgrad" if g is None else "d_head.bwd"), xa, ch.dl,
                               ch.da[last.name], dW, db, ch.Bn, last, ch.groups, ch.group_offset)
        top_end = 0
        for i in range(n - 1, -1, -1):
            L = self.dl[i]
            rows = ch.Bn * L.out_hw ** 2
            da, a, dx = ch.da[L.name], ch.view(self.d_a[L.name]), ch.dx[L.name]
            if L.bn:
                self._bn_bwd(prog, L.bn, ch.view(self.d_x[L.name]), da, a, dx, rows, L.cout, ch.groups, LRELU, Pd, g,
                             ch.coef[L.bn], write_param_grads=g is not None, group_offset=ch.group_offset, fused=fused)
            elif fused is not None:  # dx already stored by the upper dgrad GEMM; db from its partials
                if g is not None:
                    prog.sum_partials(ch.prefix + L.name + ".dbias", _p(fused[0]), fused[1], 2 * L.cout, L.cout,
                                      _p(g[L.name + "/biases"]), 0)
            elif g is None:
                prog.act_bwd(ch.prefix + L.name + ".act_bwd", _p(da), _p(a), _p(dx), dx.numel(), LRELU, leak, 0)
            else:  # live bias (no BN after it): db = sum over rows of dx, fused with the act backward
                self._act_bwd_dbias(prog, ch.prefix + L.name + ".act_bwd", da, a, dx, rows, L.cout, LRELU,
                                    g[L.name + "/biases"], "d")
            # weight gradient, then data gradient (dgrad-first measured neutral:
            # profiles/r2/ab_d_dgrad_first_r2.txt)
            if wgrad is not None:
                wgrad(i, L, dx)
            fused = None
            if i > 0:
                P_ = self.dl[i - 1]
                fused = self._dgrad(prog, ch.prefix + L.name + ".dgrad", H.GemmShape.dgrad(L, ch.Bn), dx,
                                    self.wbf_d[L.name + "/w"], same_pads(L.in_hw)[0], LRELU, ch.view(self.d_a[P_.name]),
                                    ch.da[P_.name], bn=P_.bn, x=ch.view(self.d_x[P_.name]) if P_.bn else None,
                                    dx=ch.dx[P_.name], actb=ch.prefix + P_.name, groups=ch.groups,
                                    group_offset=ch.group_offset)
            if i == n - 1:
                top_end = prog.size()
        return top_end

    def _d_wgrad(self, prog, d_in, i, L, dx) -> None:
        """The d_loss chain's weight-gradient step of D layer i (d_in: what layer 0 read)."""
        B2, gD = 2 * self.B, self.grad_d
        pad = same_pads(L.in_hw)[0]
        ws = 0
        if i == 0 and self._d0_direct() and prog.nwgrad_ok(L.in_hw, L.in_hw, L.out_hw, L.out_hw):
            # image window staged per workgroup, no column matrix (narrow2.hip nwgrad)
            prog.nwgrad(L.name + ".nwgrad", _p(d_in), B2, L.in_hw, L.in_hw, L.cin, _p(dx), L.out_hw,
                        L.out_hw, pad, _p(gD[L.name + "/w"]), ws)
        elif i == 0 and L.cin % 8 != 0:
            if self._d0_direct():  # the forward ran without a column matrix: build it here
                prog.im2col_s2("d0.im2col", _p(d_in), _p(self.d0_col), B2, L.in_hw, L.in_hw, L.cin,
                               L.out_hw, L.out_hw, pad, pad, self.kp_d0, ws)
            self._wgrad(prog, L.name, 2, self.d0_col, 1, 1, self.kp_d0, dx, B2 * L.out_hw ** 2, 1, 1, L.cout, 0,
                        gD[L.name + "/w"], stream=ws)
        else:
            src = d_in if i == 0 else self.d_a[self.dl[i - 1].name]
            self._wgrad(prog, L.name, 0, src, L.in_hw, L.in_hw, L.cin, dx, B2, L.out_hw, L.out_hw, L.cout, pad,
                        gD[L.name + "/w"], stream=ws)
        # spectral norm: this kernel's gradient (and, with the top layer, the head's) is final
        top = i == len(self.dl) - 1
        self._sn_project(prog, [L.name + "/w"] + ([self.cfg.d_lin_name + "/Matrix"] if top else []))
        if top:
            # head + top layer gradients final: DDP splits the segment here so their
            # all-reduce (76 % of D's bytes at 64x64) overlaps the rest of D's backward
            self._b_split = prog.size()

    def _build_d_backward_dloss(self, prog, sub: Optional[int] = None):
        """D's backward of d_loss: 2B rows, both statistics groups, all D gradients. sub = k: the D
        chain of D sub-step k (layer 0's weight gradient reads its d_in, or the noisy copy of it that
        the forward wrote). Sets _b_split and _b_top_dgrad."""
        d_in = self._d_input(sub)
        ch = _DChain("", 2 * self.B, 2, 0, lambda t: t, self.d_da, self.d_dx, self.coef, self.dl_d, self.grad_d)
        self._b_top_dgrad = self._d_backward(prog, ch, lambda i, L, dx: self._d_wgrad(prog, d_in, i, L, dx))

    def _w_mark(self, prog, progw, begin: int, layer: str) -> None:
        """progW[begin:] (`layer`'s weight gradient) needs progA up to its current end."""
        if progw.size() > begin:
            self._g_w.append((prog.size(), progw.size()))
            self._g_w_layer.append(layer)

    def _act_bwd_dbias(self, prog, name, dy, y, dx, rows, C, act, db, chain):
        """dx = dy * act'(y) and the bias gradient db = column sums of dx: one fused launch
        when the channel count has a kernel variant, else act_bwd + a column-sum pass."""
        leak = self.cfg.lrelu_leak if act == LRELU else 0.0
        if C in (1, 3) or (C % 8 == 0 and C <= 256 and 256 % (C // 8) == 0):
            prog.act_bwd_dbias(name, _p(dy), _p(y), _p(dx), rows, C, act, leak, _p(db), 0)
        else:
            prog.act_bwd(name, _p(dy), _p(y), _p(dx), dx.numel(), act, leak, 0)
            self._colsum(prog, name + ".dbias", dx, rows, C, db, chain)

    def _head_bwd(self, prog, name, xa, dl, dx, dW, db, R, last, groups, group_offset):
        """D head backward (dx, optional dW / db) with the top BN layer's backward statistics
        fused in: returns (partials, partials per group) for _bn_bwd, or None when the layer
        below the head has no BN / an unsupported channel count (then _bn_bwd runs its own
        statistics pass). group_offset 1 = the fake half only (g_loss chain)."""
        cfg = self.cfg
        Pd = self.model.d
        lin = cfg.d_lin_name
        K = cfg.d_lin_in
        C = last.cout
        if not (bool(last.bn) and C % 64 == 0 and K % C == 0):
            prog.head_bwd(name, _p(xa), _p(dl), _p(self._head_w()), _p(dx), _p(dW), _p(db), R, K, 0)
            return None
        S = K // C
        # row splits: RS x the workgroups of one-per-64-columns (the head's R rows are few)
        RS = 2  # (A/B 1 / 2 / 4 splits: 2 best, profiles/r2/ab_head_nconv_nwgrad_r2.txt)
        while RS > 1 and (R % RS or (R // groups) % (R // RS)):
            RS //= 2
        part = self._stats_buf(name + ".bnstats", groups * RS * S, C)
        st = self.bn[last.bn]
        r0 = 0 if group_offset == 0 else self.B
        prog.head_bwd_rs(name, _p(xa), _p(dl), _p(self._head_w()), _p(dx), _p(dW), _p(db), R, K, 0,
                         _p(self.d_x[last.name][r0:]), _p(self.d_a[last.name][r0:]), _p(st["mean"][group_offset:]),
                         _p(st["rstd"][group_offset:]), C, R // groups, LRELU, cfg.lrelu_leak, _p(part), RS)
        return part, RS * S

    def _colsum(self, prog, name, x, rows, C, dst, chain):
        if C % 8 == 0:
            rpb = self._rows_per_block(rows, C)
            part = self._stats_buf(name, rows // rpb, C)
            prog.colstats(name, 2, _p(x), 0, 0, 0, 0, 0, 0.0, rows, C, rpb, rows, _p(part), 0)
            prog.sum_partials(name + ".sum", _p(part), rows // rpb, 2 * C, C, _p(dst), 0)
        else:
            blocks = 64
            sp = self.small_part[chain]
            prog.colsum_small(name, _p(x), rows, C, _p(sp), blocks, 0)
            prog.sum_partials(name + ".sum", _p(sp), blocks, C, C, _p(dst), 0)

    def _wgrad(self, prog, name, mode, G, Hg, Wg, Mc, Dm, Bn, Hd, Wd, Nc, pad, dst, stream=0):
        """Weight gradient dst [25][Mc][Nc] (fp32): wgrad3 / wgrad5 (16-bit, 25-tap layers, split-K
        reduced on the device, deterministic), else the first-generation slab kernel + reduce."""
        K = Bn * Hd * Wd
        taps = 1 if mode == 2 else 25
        if mode == 0 and not self.f32:  # 25-tap layers: LDS-DMA pipelined kernel, split-K reduced in-kernel
            plan = H.wgrad3_cfg_for(Mc, Nc, Bn, Hd, Wd, Hg)
            if plan is not None:
                prog.wgrad3(name + ".wgrad", _p(G), Hg, Wg, Mc, _p(Dm), Bn, Hd, Wd, Nc, pad, plan[0], plan[1],
                            _p(dst), 1.0, stream)
                return
        cfg, splits = H.pick_wgrad(Mc, Nc, K, taps, dtype=self.dt)
        if mode == 0 and not self.f32:
            splits = H.wgrad_splits_for(Mc, Nc, Bn, Hd, Wd, Hg) or splits
        slabs = self._t(splits, taps, Mc, Nc, dtype=torch.float32)
        self._keep.append(slabs)
        prog.wgrad(name + ".wgrad", mode, _p(G), Hg, Wg, Mc, _p(Dm), Bn, Hd, Wd, Nc, pad, cfg, splits, _p(slabs),
                   _p(dst), dst.numel(), 1.0, stream)

    def _bn_bwd(self, prog, name, x, dy, y, dx, rows, C, groups, act, P, grads, coef, write_param_grads,
                group_offset=0, fused=None):
        """BN + activation backward over `groups` statistics groups from `group_offset` (1: the fake
        half only). fused = (partials, partials per group) when the producing data-gradient GEMM
        already emitted the statistics (else a column-stats pass here)."""
        st = self.bn[name]
        mean, rstd = st["mean"][group_offset:], st["rstd"][group_offset:]
        rpg = rows // groups
        if fused is not None:
            part, ppg = fused[0], fused[1]
            Pn = ppg * groups
        else:
            rpb = self._rows_per_block(rpg, C)
            Pn = rows // rpb
            part = self._stats_buf(name + ".bwd", Pn, C)
            prog.colstats(name + ".bwd_stats", 1, _p(x), _p(dy), _p(y), _p(mean), _p(rstd), act,
                          self.cfg.lrelu_leak, rows, C, rpb, rpg, _p(part), 0)
        dg = grads[name + "/gamma"] if write_param_grads else None
        db = grads[name + "/beta"] if write_param_grads else None
        prog.bn_bwd_finalize(name + ".bwd_fin", _p(part), Pn // groups, groups, C, float(rpg),
                             _p(P[name + "/gamma"]), _p(mean), _p(rstd), _p(dg), _p(db), _p(coef), 0)
        prog.bn_bwd_apply(name + ".bwd_apply", _p(dy), _p(y), _p(x), _p(coef), _p(dx), rows, C, rpg, act,
                          self.cfg.lrelu_leak, 0)

    # ---- g_loss back through D(fake) (fake rows only, no D grads) and G backward
    def _build_gloss_and_g_backward(self, prog, progw):
        """progA: g_loss back through D(fake), then G's data-gradient chain; progw: G's weight
        gradients, each recorded with the progA position it needs (self._g_w). Under the fused
        schedule they run on the D chain's stream once that chain is done, beside the G
        data-gradient chain (which then has nothing else on its critical path)."""
        B, L = self.B, self.dl[0]
        # the fake half only: B rows, one statistics group (group 1), gradient buffers of its own
        seed = self.dl_g
        if self.topk.active:
            # top-k: G learns from the k(t) best-scored fakes; the chain's kernels only see another seed
            seed = self.dl_g_k
            prog.g_topk("g_topk", _p(self.logits[B:]), _p(self.dl_g), _p(seed), _p(self.topk_sel),
                        _p(self.topk_info), B, R.topk_kmin(B, self.topk.nu), self.topk.steps,
                        _p(self.step_counter), H.gan_loss_id(self.gan_loss, self.label_smooth), 0)
        ch = _DChain("g.", B, 1, 1, lambda t: t[B:], self.gc_da, self.gc_dx, self.coef_g, seed, None)
        self._d_backward(prog, ch)
        dx, nat, pad = self.gc_dx[L.name], self.wbf_d[L.name + "/w"], same_pads(L.in_hw)[0]
        if self._img_dact():
            # image gradient with G's tanh backward fused (dL/d(G pre-activation) straight out)
            # + the G output bias gradient from its per-workgroup column sums
            Lg = self.gl[-1]
            prog.narrow_deconv_dact("g." + L.name + ".dgrad_img+tanh_bwd", _p(dx), _p(nat), _p(self.img_g),
                                    _p(self.fake), B, L.out_hw, L.out_hw, L.cout, L.in_hw, L.in_hw, L.cin,
                                    pad, TANH, 0.0, _p(self.grad_g[Lg.name + "/biases"]), 0)
        elif not self.f32 and L.cin <= 4 and L.cout % 8 == 0 and L.cout <= 256:  # 3-channel image gradient
            prog.narrow_deconv("g." + L.name + ".dgrad_img", _p(dx), _p(nat), 0, _p(self.img_grad), B,
                               L.out_hw, L.out_hw, L.cout, L.in_hw, L.in_hw, L.cin, pad, NONE, 0.0, 0)
        else:
            self._igemm(prog, "g." + L.name + ".dgrad_img", H.GemmShape.dgrad(L, B), dx, nat, self.img_grad, pad)
        img_grad = self.img_grad
        for st in self._d_stages(transposed=True):
            # DiffAugment: dL/d(the stage's copy of the fake) -> dL/d(its input), the stage's transpose --
            # the transposed gather of `d_aug`, the transposed color map under (s, c) of `d_color` -- over
            # the draws (and gates) the forward recorded for the fake half (rows B..2B-1)
            gx = getattr(self, st.grad)
            gate = dict(gates=_p(getattr(self, st.gates)[B:])) if self.ada.active else {}
            getattr(prog, st.op + "_bwd")(st.name + "_bwd", _p(img_grad), _p(gx), _p(getattr(self, st.params)[B:]), B,
                                          L.in_hw, L.cin, getattr(self, st.opt).mask, 0, **gate)
            img_grad = gx
        self._build_g_backward(prog, progw, img_grad)

    def _build_g_backward(self, prog, progw, img_grad):
        """G's backward from the image gradient img_g (G's tanh backward already applied when the
        image-gradient kernel fused it; else taken here from img_grad, the g_loss chain's gradient at
        the clean pixels): data gradients into prog, weight gradients into progw."""
        cfg, B = self.cfg, self.B
        Pg, gG = self.model.g, self.grad_g
        self._a_gd_end = prog.size()  # the g_loss chain is done with D's weights / BN parameters
        n = len(self.gl)
        Lg = self.gl[-1]
        if not self._img_dact():  # (else fused into the image-gradient kernel above)
            # (DiffAugment: behind the last transpose, at the clean pixels, where tanh' is taken)
            self._act_bwd_dbias(prog, "g_out.tanh_bwd", img_grad, self.fake, self.img_g, B * Lg.out_hw ** 2,
                                Lg.cout, TANH, gG[Lg.name + "/biases"], "g")

        def below(j):  # what feeds G layer j: (activation, its gradient, pre-BN input, BN layer)
            if j == 0:
                return self.g_h0, self.g_da0, self.g_h0_pre, "g_bn0"
            Lb = self.gl[j - 1]
            return self.g_a[Lb.name], self.g_da[Lb.name], self.g_x[Lb.name], Lb.bn

        a_prev, da_prev, x_prev, bn_prev = below(n - 1)
        padL = same_pads(Lg.out_hw)[0]
        wL = self.wbf_g[Lg.name + "/w"]  # [5,5,co,ci] read as [tap][K=co][N=ci]
        w0 = progw.size()
        if self._g_out_direct():
            # narrow2.hip: the data gradient is the stride-2 conv of the image gradient with the
            # [5,5,co,ci] = HWIO[5,5,3,64] weight (nconv, BN-backward statistics of the layer below
            # fused), the weight gradient reads the image gradient's window directly (nwgrad)
            # persistent grid (one workgroup per tile measured the same beside the D chain)
            grid = H.nconv_grid(prog, B, Lg.in_hw, Lg.in_hw)
            part = self._stats_buf(bn_prev + ".bwd", grid, Lg.cin)
            st = self.bn[bn_prev]
            progw.nwgrad(Lg.name + ".nwgrad", _p(self.img_g), B, Lg.out_hw, Lg.out_hw, Lg.cout, _p(a_prev), Lg.in_hw,
                         Lg.in_hw, padL, _p(gG[Lg.name + "/w"]), 0)
            self._w_mark(prog, progw, w0, Lg.name)
            prog.nconv(Lg.name + ".dgrad", _p(self.img_g), _p(wL), 0, _p(da_prev), B, Lg.out_hw, Lg.out_hw, Lg.cout,
                       Lg.in_hw, Lg.in_hw, padL, padL, NONE, 0.0, grid, _p(x_prev), _p(a_prev), _p(st["mean"]),
                       _p(st["rstd"]), RELU, cfg.lrelu_leak, _p(part), 0)
            fused_next = (part, grid)
        elif Lg.cout % 8 != 0:
            prog.im2col_s2("g_out.im2col", _p(self.img_g), _p(self.g_last_col), B, Lg.out_hw, Lg.out_hw, Lg.cout,
                           Lg.in_hw, Lg.in_hw, padL, padL, self.kp_g, 0)
            self._wgrad(progw, Lg.name, 2, self.g_last_col, 1, 1, self.kp_g, a_prev, B * Lg.in_hw ** 2, 1, 1, Lg.cin,
                        0, gG[Lg.name + "/w"])
            self._w_mark(prog, progw, w0, Lg.name)
            shape = H.GemmShape(2, B, 1, 1, self.kp_g, Lg.in_hw, Lg.in_hw, Lg.cin, True)
            fused_next = self._dgrad(prog, Lg.name + ".dgrad", shape, self.g_last_col, wL, 0, RELU, a_prev, da_prev,
                                     bn=bn_prev, x=x_prev, kb_valid=25 * Lg.cout)
        else:
            self._wgrad(progw, Lg.name, 0, self.img_g, Lg.out_hw, Lg.out_hw, Lg.cout, a_prev, B, Lg.in_hw, Lg.in_hw,
                        Lg.cin, padL, gG[Lg.name + "/w"])
            self._w_mark(prog, progw, w0, Lg.name)
            fused_next = self._dgrad(prog, Lg.name + ".dgrad", H.GemmShape.dgrad(Lg, B), self.img_g, wL, padL, RELU,
                                     a_prev, da_prev, bn=bn_prev, x=x_prev)
        for j in range(n - 2, -1, -1):
            L = self.gl[j]
            rows = B * L.out_hw ** 2
            x, a, da, dx = self.g_x[L.name], self.g_a[L.name], self.g_da[L.name], self.g_dx[L.name]
            self._bn_bwd(prog, L.bn, x, da, a, dx, rows, L.cout, 1, RELU, Pg, gG, self.coef[L.bn],
                         write_param_grads=True, fused=fused_next)
            src, dsrc, xsrc, bsrc = below(j)
            pad = same_pads(L.out_hw)[0]
            w0 = progw.size()
            self._wgrad(progw, L.name, 0, dx, L.out_hw, L.out_hw, L.cout, src, B, L.in_hw, L.in_hw, L.cin, pad,
                        gG[L.name + "/w"])
            self._w_mark(prog, progw, w0, L.name)
            fused_next = self._dgrad(prog, L.name + ".dgrad", H.GemmShape.dgrad(L, B), dx, self.wbf_g[L.name + "/w"],
                                     pad, RELU, src, dsrc, bn=bsrc, x=xsrc)
        # g_bn0 backward + projection gradients
        C0 = cfg.g_base_ch
        rows0 = B * cfg.g_base_hw ** 2
        self._bn_bwd(prog, "g_bn0", self.g_h0_pre, self.g_da0, self.g_h0, self.g_dx0, rows0, C0, 1, RELU, Pg, gG,
                     self.coef["g_bn0"], write_param_grads=True, fused=fused_next)
        prog.linear_wgrad("g_h0_lin.wgrad", _p(self.z), _p(self.g_dx0), _p(gG["g_h0_lin/Matrix"]),
                          _p(gG["g_h0_lin/bias"]), B, cfg.z_dim, cfg.g_lin_out, 0)


    # ---- optimiser (+ 16-bit weight mirrors)
    def _lr_kw(self, with_step: bool = True) -> dict:
        """The schedule's keyword arguments of an Adam op ({} when off: the op as it always was).
        adam2 takes the counter as its own `step` argument (with_step=False)."""
        if not self.lr_sched.active:
            return {}
        kw = dict(zip(("lr_kind", "lr_start", "lr_steps", "lr_end", "lr_warmup"), self.lr_sched.hip_args()))
        if with_step:
            kw["lr_step"] = _p(self.step_counter)
        return kw

    def _net(self, net: str):
        """(parameter set, gradient, 16-bit mirror -- None in fp32 --, optimiser, bf16 wire image or
        None) of network "d" / "g"."""
        if net == "d":
            return self.model.d, self.grad_d, None if self.f32 else self.wbf_d, self.opt_d, self.wire_d
        return self.model.g, self.grad_g, None if self.f32 else self.wbf_g, self.opt_g, self.wire_g

    def _adam(self, prog, name: str, net: str, a: int = 0, b: Optional[int] = None, ls: int = 0,
              wire: bool = False) -> None:
        """One adam_bf op over the flat range [a, b) (default: all) of network `net`: weights, mirror,
        gradient and both slots at the same element offset, the mean over the ranks as gscale.
        wire: the gradient is read from the bf16 wire image instead."""
        ps, grad, mir, opt, img = self._net(net)
        b = ps.flat.numel() if b is None else b
        at = lambda t: _p(t.flat) + t.flat.element_size() * a  # noqa: E731
        prog.adam_bf(name, at(ps), 0 if mir is None else at(mir), at(grad), at(opt.m), at(opt.v), _p(opt.powers),
                     b - a, opt.lr, opt.beta1, opt.beta2, opt.eps, 1.0 / self.world, 0, ls, at(img) if wire else 0,
                     **self._lr_kw())

    def _step_end(self, prog, ls: int = 0) -> None:
        """Both beta-power pairs, the global step and (ls) the fp16 loss-scale rule, after both Adams."""
        od, og = self.opt_d, self.opt_g
        prog.step_end("step_end", _p(od.powers), _p(og.powers), od.beta1, od.beta2, og.beta1, og.beta2,
                      _p(self.step_counter), 0, ls, self.LOSS_SCALE_GROWTH)

    def _ema_g(self, prog, step_bias: int, ls: int = 0) -> None:
        """The moving average of G's weights (+ its 16-bit mirror): one launch on the stream of,
        and after, the last Adam launch that writes G. step_bias = 1 where the step counter is
        advanced by a later launch (step_end), 0 where it already was (adam2)."""
        if self.g_ema is None:
            return
        prog.ema("ema_g", _p(self.g_ema.flat), 0 if self.f32 else _p(self.wbf_g_ema.flat), _p(self.model.g.flat),
                 self.model.g.flat.numel(), self.g_ema_decay, _p(self.step_counter), step_bias, ls, 0)

    def _build_update(self, prog, first: bool):
        """TF-Adam for G (first part) and D + the step counter (last part); each Adam also
        writes the 16-bit mirror the conv GEMMs read (fp32: none, the GEMMs read the masters).
        Under DDP the G all-reduce completes first (it was issued before D's backward ends), so
        Adam(G) runs while D's last bucket is still on the wire. fp16: one overflow check over
        both (all-reduced) gradients gates both Adams, so everything runs in the last part."""
        ls = _p(self.loss_scale)
        do_g = (first and not self.f16) or (not first and self.f16)
        do_d = not first
        if self.f16 and do_d:
            prog.nonfinite_check("ls.check_d", _p(self.grad_d.flat), self.grad_d.flat.numel(), ls, 0)
            prog.nonfinite_check("ls.check_g", _p(self.grad_g.flat), self.grad_g.flat.numel(), ls, 0)
        if do_g:
            self._adam(prog, "adam_g", "g", ls=ls)
            self._ema_g(prog, 1, ls)
        if do_d:
            self._adam(prog, "adam_d", "d", ls=ls)
            self._sn_power(prog, ls)
            self._step_end(prog, ls)

    def _build_update_fused(self, prog):
        """Single-process bf16: both TF-Adams + the beta-power / global-step update in one launch
        (adam2_kernel), G's buffer first -- the same arithmetic as the separate kernels."""
        od, og = self.opt_d, self.opt_g
        G, Dm = self.model.g, self.model.d
        prog.adam2("adam_gd", _p(G.flat), _p(self.wbf_g.flat), _p(self.grad_g.flat), _p(og.m.flat), _p(og.v.flat),
                   _p(og.powers), G.flat.numel(), og.lr, og.beta1, og.beta2, og.eps, _p(Dm.flat), _p(self.wbf_d.flat),
                   _p(self.grad_d.flat), _p(od.m.flat), _p(od.v.flat), _p(od.powers), Dm.flat.numel(), od.lr,
                   od.beta1, od.beta2, od.eps, 1.0 / self.world, _p(self.step_counter), 0, **self._lr_kw(False))
        self._ema_g(prog, 0)
        self._sn_power(prog)

    def _repack_weights_now(self):
        if self.progCast.size():
            H.run(self.progCast)
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ execution
    MAIN, ALT = 0, 1
    # G's weight gradients off the G chain's stream (fused schedule; where: _gw_place): None = by
    # image size. Round 2, behind the D chain (profiles/r2/ab_g_wgrad_after_d_chain_r2.txt): 64x64
    # 1.105 vs 1.13 ms, 28x28 even, 128x128 5.84 vs 5.70 ms, 256x256 106.2 vs 104.6 ms -- at the
    # larger sizes the D chain (2B rows of the bigger images) is the longer one already
    G_WGRAD_ON_D_STREAM: Optional[bool] = None

    def _g_wgrad_on_d_stream(self) -> bool:
        if self.G_WGRAD_ON_D_STREAM is not None:
            return bool(self.G_WGRAD_ON_D_STREAM)
        env = os.environ.get("DCGAN_G_WGRAD_ON_D")
        if env in ("0", "1"):
            return env == "1"
        # 128x128 bf16 with the G weight gradients beside the chains (alt1): 34.4k-34.5k vs
        # 33.8k-33.9k img/s; 256x256 fp16 within the noise, kept on cs
        # (profiles/r5/ab_gw_place_128_256_r5.txt)
        return self.cfg.output_size <= 128

    def _schedule(self) -> str:
        req = self._sched_req
        if self._timing:  # phase timers need the segmented step
            return req if req in ("concurrent", "serial") else "concurrent"
        if self.ddp:
            if req in ("ddp", "concurrent", "serial"):
                return req
            # "concurrent" by default: inside ONE hipGraph the collectives do not overlap the
            # compute branches on ROCm (emulated ring collectives, 64x64: 1.39 ms vs 1.33 for
            # the segmented step; profiles/r3/ab_ddp_one_graph_r3.txt)
            env = os.environ.get("DCGAN_DDP_SCHEDULE") or "concurrent"
            if env not in DDP_SCHEDULES:  # "fused" here would issue no all-reduce at all
                raise ValueError("DCGAN_DDP_SCHEDULE=%r: expected one of %s" % (env, ", ".join(DDP_SCHEDULES)))
            return env
        return req or "fused"

    def _one_graph(self) -> bool:
        return self._schedule() in ("fused", "ddp")

    def _segments(self):
        """The step as a list of (name, runner, stream) segments: runner(ex, stream, sec) issues the
        segment onto `stream` (+ `sec`, its slot-1 stream; multi-stream segments fork the alt
        streams from `stream` and join them back before they end). runner.empty: nothing to run
        (fp16 keeps both Adams in the last segment)."""
        sch = self._schedule()
        A, B, C, W = self.progA, self.progB, self.progC, self.progW
        M = self.MAIN
        lin = self._lin_segment
        ada = [(self.progAda, 0, -1)] if self.progAda is not None else []  # the controller heads the D chain
        if sch in ("fused", "ddp"):
            run = (lambda ex, cs, sec: self._run_fused(ex, cs)) if sch == "fused" else \
                (lambda ex, cs, sec: self._run_ddp(ex, cs))
            run.empty = False
            return [("step", run, M)]
        if sch == "concurrent" and self._sharded():
            return [("fwd", lin([(A, 0, self._a_fwd)]), M), ("D_bwd_top", lin(ada + [(B, 0, self._b_split)]), self.ALT),
                    ("G_chain", lin([]), M), ("D_bwd_rest", lin([(B, self._b_split, -1)]), self.ALT),
                    ("G_tail", lin([]), M), ("update", lin([(C, 0, -1)]), M)]
        if sch == "serial":
            return [("fwd+G_bwd", lin([(A, 0, -1), (W, 0, -1)]), M), ("D_bwd_top", lin(ada + [(B, 0, self._b_split)]), M),
                    ("D_bwd_rest", lin([(B, self._b_split, -1)]), M), ("adam_G", lin([(C, 0, self._c_split)]), M),
                    ("adam_D", lin([(C, self._c_split, -1)]), M)]
        # "concurrent": one graph per chain segment, each on its own stream; the collectives go
        # out between them (ROCm refuses events recorded inside a graph that outside work waits
        # on: profiles/r2/probe_external_event_r2.txt). Graphs that fork and join both streams
        # around the collectives measured slower (profiles/r5/ab_ddp_5graph_joined_r5.txt).
        X = self.progX
        wx = lambda name: ([(X, self._wire_ops[name], self._wire_ops[name] + 1)]  # noqa: E731
                           if self._wire_direct() and name in self._wire_ops else [])
        sp = self._g_split
        if sp is None:
            g_chain, g_tail = [(A, self._a_fwd, -1), (W, 0, -1)] + wx("g"), []
        else:  # G's lowest deconv weight gradient ends the chain; the rest of G's backward follows
            a_need, wb, we = sp[:3]
            g_chain = [(A, self._a_fwd, a_need), (W, wb, we)] + wx("g_a")
            g_tail = [(A, a_need, -1), (W, 0, wb), (W, we, -1)] + wx("g_b") + wx("g_c")
        segs = [("fwd", lin([(A, 0, self._a_fwd)]), M),
                ("D_bwd_top", lin(ada + [(B, 0, self._b_split)] + wx("dtop")), self.ALT),
                ("G_chain", lin(g_chain), M),
                ("D_bwd_rest", lin([(B, self._b_split, -1)] + wx("drest")), self.ALT),
                ("G_tail", lin(g_tail), M)]
        if self._adam_g_split():
            segs.append(("adam_G_a", lin([(C, self._c_split, self._c_split_a)]), M))
        return segs + [("adam_D", lin([(C, 0, self._c_split)]), M),
                       ("adam_G", lin([(C, self._c_split_a, -1)]), M)]

    @staticmethod
    def _lin_segment(parts):
        def run(ex, cs, sec):
            for prog, b, e in parts:
                ex.run(prog, [cs, sec], b, e)
        run.empty = all((prog.size() if e < 0 else e) <= b for prog, b, e in parts)
        return run

    def _w_begin(self, k: int) -> int:
        return self._g_w[k - 1][1] if k > 0 else 0

    def enable_timing(self) -> None:
        """Per-phase GPU timers: the step runs as segments with events between
        them. Call before the first train_step (graphs are captured per segment). Concurrent
        schedule: each phase is reported as ms from the step start to the END of that phase
        (the D and G chains overlap); serial schedule: phase durations. The update program is
        rebuilt for the segmented schedule (Adam(G) and Adam(D) apart)."""
        if self._graphs or self._step_host:
            raise RuntimeError("enable_timing() must precede the first train_step")
        self._timing = True
        self._build_updates()
        self._ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(self._segments()) + 1)]

    def phase_times(self) -> Dict[str, float]:
        """Milliseconds of the last step's phases (synchronises on its last event)."""
        if not self._timing:
            return {}
        ev = self._ev
        ev[-1].synchronize()
        segs = self._segments()
        if self._schedule() == "concurrent":
            return {n + "@end": ev[0].elapsed_time(ev[i + 1]) for i, (n, _, _) in enumerate(segs)}
        return {n: ev[i].elapsed_time(ev[i + 1]) for i, (n, _, _) in enumerate(segs)}

    def _tick(self, i, stream) -> None:
        if self._timing and not self.dry:
            self._ev[i].record(stream)

    def _get_exec(self):
        if self._exec is None:
            self._exec = _TorchExec(self)
        return self._exec

    def _run_fused(self, ex, cs):
        """The "fused" schedule issued onto cs (+ the alt streams); also what gets captured. D's
        backward starts right after the forward (profiles/r4/ab_d_start_after_r4.txt); G's weight
        gradients run on the streams _gw_place() gives."""
        ex.run(self.progA, [cs, ex.side], 0, self._a_fwd)
        ex.wait(ex.alt[0], cs)
        tail = self._ada_at_tail()
        if self.progAda is not None and not tail:
            ex.run(self.progAda, ex.alt)
        ex.run(self.progB, ex.alt)
        if self.progAda is not None and tail:
            ex.run(self.progAda, ex.alt)
        # the G chain: data gradients on cs; each G weight gradient on its _gw_place() stream once
        # cs has produced its operand (a mark after that progA position)
        if not self._g_wgrad_on_d_stream():  # every G gradient on cs
            ex.run(self.progA, [cs, ex.side], self._a_fwd, -1)
            ex.run(self.progW, [cs, ex.side])
            ex.wait(cs, ex.alt[0])
            ex.run(self.progC, [cs, ex.side])
            return
        pos, marks = self._a_fwd, []
        for a_end, _ in self._g_w:
            ex.run(self.progA, [cs, ex.side], pos, a_end)
            marks.append(ex.mark(cs))
            pos = a_end
        ex.run(self.progA, [cs, ex.side], pos, -1)
        place = self._gw_place()
        streams = {"d": ex.alt, "s": [ex.side], "a": [ex.alt[1]]}
        w, segs = 0, []
        for k, (m, (_, w_end)) in enumerate(zip(marks, self._g_w)):
            segs.append((place[k], w, w_end))
            if place[k] != "c":
                st = streams[place[k]]
                ex.wait_mark(st[0], m)
                ex.run(self.progW, st, w, w_end)
            w = w_end
        for q in sorted(set(place) & {"s", "a"}):
            ex.wait(cs, streams[q][0])
        # the G weight gradients placed on cs run after the G chain (their operands are produced
        # there)
        for q, lo, hi in segs:
            if q == "c":
                ex.run(self.progW, [cs, ex.side], lo, hi)
        ex.wait(cs, ex.alt[0])
        ex.run(self.progC, [cs, ex.side])

    def _ada_at_tail(self) -> bool:
        """The fused step's place for `ada_update` on the D chain's stream: behind the chain's last op, ahead
        of the join (default), or with DCGAN_ADA_PLACE=head ahead of its first. Six interleaved pairs each
        against the ungated step: +2.9 us at the tail, +10.3 us at the head, where the launch delays the
        chain that ends the step (profiles/r18/ada_cost_r18.txt). The segmented and one-graph DDP schedules
        keep it at the head of the chain's first segment."""
        return os.environ.get("DCGAN_ADA_PLACE") != "head"

    def _gw_place(self) -> str:
        """Stream of each G weight-gradient segment in the fused step: "a" (default) the idle alt1
        stream as soon as its operand exists, "s" the side stream, "d" behind the D chain, "c" on
        cs after the G chain; DCGAN_GW_PLACE gives one letter per segment ("aaaa" measured best,
        profiles/r5/ab_gw_place_r5.txt)."""
        n = len(self._g_w)
        v = os.environ.get("DCGAN_GW_PLACE")
        if v is None:
            return "a" * n
        if len(v) != n or set(v) - set("dcsa"):
            raise ValueError("DCGAN_GW_PLACE must be %d letters of d/c/s/a, got %r" % (n, v))
        return v

    def _seg(self, ex, i, stream):
        """Run segment i on `stream` (graph replay, or eager replay of its program ranges)."""
        if self.graph_enabled:
            g = self._graphs[i]
            if g is not None:
                ex.replay(g, stream)
            return
        _, run, which = self._segments()[i]
        run(ex, stream, ex.side if which == self.MAIN else ex.alt[1])

    # ---- D-only sub-steps (d_steps > 1)
    def _sub_segments(self, k: int):
        """D sub-step k as (name, runner, stream) segments, as ``_segments`` gives the full step.
        "fused": one segment (forward on cs, the D chain on the alt streams, the join, the update).
        "concurrent": forward | D chain top | D chain rest | update, with D's two collectives issued
        between them (``_run_d_substep``), each gradient slice reduced where it becomes final."""
        F, Bk = self._sub[k]
        M, lin = self.MAIN, self._lin_segment
        if self._schedule() == "fused":
            run = lambda ex, cs, sec: self._run_fused_sub(ex, cs, k)  # noqa: E731
            run.empty = False
            return [("d_step", run, M)]
        X = self.progX
        wx = lambda name: ([(X, self._wire_ops[name], self._wire_ops[name] + 1)]  # noqa: E731
                           if self._wire_direct() and name in self._wire_ops else [])
        return [("d_fwd", lin([(F, 0, -1)]), M), ("d_bwd_top", lin([(Bk, 0, self._b_split)] + wx("dtop")), self.ALT),
                ("d_bwd_rest", lin([(Bk, self._b_split, -1)] + wx("drest")), self.ALT),
                ("d_update", lin([(self.progDU, 0, -1)]), M)]

    def _run_fused_sub(self, ex, cs, k: int) -> None:
        """D sub-step k of the "fused" schedule issued onto cs (+ the alt streams); also what gets
        captured. The D chain runs on its own stream as in the full step; the update waits for it."""
        F, Bk = self._sub[k]
        ex.run(F, [cs, ex.side])
        ex.wait(ex.alt[0], cs)
        ex.run(Bk, ex.alt)
        ex.wait(cs, ex.alt[0])
        ex.run(self.progDU, [cs, ex.side])

    def _sub_seg(self, ex, k: int, i: int, stream) -> None:
        if self.graph_enabled:
            g = self._sub_graphs[k][i]
            if g is not None:
                ex.replay(g, stream)
            return
        _, run, which = self._sub_segments(k)[i]
        run(ex, stream, ex.side if which == self.MAIN else ex.alt[1])

    def _run_d_substep(self, ex, k: int) -> None:
        """Issue D sub-step k. It starts on the main stream behind everything the previous (sub-)step
        queued there and ends with every stream it used joined back into the main stream."""
        cs = ex.main()
        if self._schedule() == "fused":
            self._sub_seg(ex, k, 0, cs)
            return
        alt = ex.alt[0]
        self._sub_seg(ex, k, 0, cs)            # z_k, G fwd, D fwd (real_k | fake), losses
        ex.wait(alt, cs)
        self._sub_seg(ex, k, 1, alt)           # D chain: head + top layer gradients
        self._ar_launch(ex, "dtop", alt)
        self._sub_seg(ex, k, 2, alt)           # D chain: the rest -> grad_d final
        self._ar_launch(ex, "drest", alt)
        self._ar_join(ex, cs)                  # Adam(D) after D's last collective
        ex.wait(cs, alt)
        self._sub_seg(ex, k, 3, cs)            # Adam(D), D's powers, sn_power

    def _run_step(self, ex):
        """One training step: the d_steps - 1 D sub-steps in order, then the full step."""
        for k in range(self.d_steps - 1):
            self._run_d_substep(ex, k)
        self._run_full_step(ex)

    def _run_full_step(self, ex):
        cs = ex.main()
        sch = self._schedule()
        if sch in ("fused", "ddp"):
            if self.graph_enabled:
                self._seg(ex, 0, cs)
            elif sch == "fused":
                self._run_fused(ex, cs)
            else:
                self._run_ddp(ex, cs)
            return
        self._run_segmented(ex, cs, sch)

    def _capture(self):
        """Capture the step: "fused" and "ddp" as ONE hipGraph ("ddp" with its RCCL collectives
        inside), the segmented schedules one graph per segment (their collectives stay outside,
        issued between replays on the comm stream). Capturing does not execute anything; it is
        attempted only after one eager step has loaded every code object, and any failure
        falls back to eager replay of the recorded programs."""
        ex = self._get_exec()
        sch = self._schedule()
        if sch == "ddp" and self.ddp and D.is_initialized() and D.backend() != "nccl":
            return False  # host-synchronous collectives (gloo) cannot be captured
        try:
            torch.cuda.synchronize(self.device)
            graphs = []
            one = self._one_graph()
            for name, run, which in self._segments():
                if run.empty:
                    graphs.append(None)  # empty segment (fp16: no separate G update)
                    continue
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    cs = torch.cuda.current_stream(self.device)
                    if one and self.ddp:
                        ex.wait(ex.comm, cs)  # the comm stream joins the capture from its start
                    run(ex, cs, ex.side if which == self.MAIN else ex.alt[1])
                graphs.append(g)
            sub_graphs = []
            for k in range(self.d_steps - 1):  # one graph per sub-step (segmented: per segment)
                sub_graphs.append([])
                for name, run, which in self._sub_segments(k):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        run(ex, torch.cuda.current_stream(self.device), ex.side if which == self.MAIN else ex.alt[1])
                    sub_graphs[k].append(g)
            self._graphs, self._sub_graphs = graphs, sub_graphs
            return True
        except Exception as e:  # pragma: no cover - depends on runtime
            print("[hip_engine] graph capture failed, running eagerly: %s" % e)
            self._graphs, self._sub_graphs = [], []
            return False

    def _prepare_run(self) -> None:
        if self.dry:
            raise RuntimeError("a dry-run engine only records the step (engine.schedule_check)")
        self._ensure_comm()
        if (self.graph_requested and not self.graph_enabled and self._step_host >= 1
                and not getattr(self, "_cap_tried", 0)):
            self._cap_tried = 1
            self.graph_enabled = self._capture()

    def _count_d_bn(self) -> None:
        for s in range(self.model.d_bn.slots):
            self.model.d_bn.count_step(s)

    def train_step(self) -> None:
        """d_steps - 1 D sub-steps (each on its own staged batch and z), then the full step."""
        for k in range(self.d_steps - 1):
            self.train_d_step(k)
        self.train_full_step()

    def train_full_step(self) -> None:
        """The full step alone: what train_step runs after the sub-steps (tests)."""
        self._prepare_run()
        self._run_full_step(self._get_exec())
        self._step_host += 1
        # one EMA update per BN slot per step (zero-debias bookkeeping, host-side counters)
        self.model.g_bn.count_step(0)
        self._count_d_bn()

    def train_d_step(self, k: int) -> None:
        """D sub-step k alone (tests; its losses are readable through last_losses())."""
        if not 0 <= k < self.d_steps - 1:
            raise ValueError("sub-step %d out of range for d_steps = %d" % (k, self.d_steps))
        self._prepare_run()
        self._run_d_substep(self._get_exec(), k)
        self._count_d_bn()  # D's BN moving averages update in every sub-step, G's do not

    @property
    def global_step(self) -> int:
        return int(self.step_counter.item())

    @global_step.setter
    def global_step(self, v: int) -> None:
        self.step_counter.fill_(int(v))

    def set_synthetic_batch(self, real: torch.Tensor) -> None:
        """The same batch into every staging slot."""
        for k in range(self.d_steps):
            self.set_batch(real, k)

    def set_batch(self, real: torch.Tensor, slot: int = 0) -> None:
        """Copy a [B,H,W,C] batch (any float dtype, values already in [-1,1]) into the real half of
        staging slot `slot`: slot k < d_steps - 1 is D sub-step k's batch, slot d_steps - 1 the full
        step's (d_steps = 1: the only one)."""
        B = self.B
        if real.shape[0] != B:
            raise ValueError("batch %d != engine batch %d" % (real.shape[0], B))
        if not 0 <= slot < self.d_steps:
            raise ValueError("batch slot %d out of range for d_steps = %d" % (slot, self.d_steps))
        self.d_ins[slot][:B].copy_(real.to(self.device, non_blocking=True))

    def last_losses(self) -> Dict[str, float]:
        l = self.losses.tolist()
        return {"d_loss_real": l[0], "d_loss_fake": l[1], "g_loss": l[2], "d_loss": l[3]}

    def losses_tensor(self) -> torch.Tensor:
        return self.losses

    def last_topk(self):
        """(k, g_loss_topk, threshold logit) of the last full step's top-k selection; None when off."""
        if not self.topk.active:
            return None
        g, thr, _, k = self.topk_info.tolist()
        return int(k), g, thr

    def topk_selection(self) -> Optional[torch.Tensor]:
        """The bool mask [B] of the fakes G learned from in the last full step (None: top-k off)."""
        return self.topk_sel.ne(0) if self.topk.active else None

    def ada_status(self):
        """The adaptive-augmentation state as Python ints {p24, acc, cnt, r_acc, windows} plus p and r_t
        (= r_acc / (B * interval), of the last finished window); None when no gate is recorded."""
        if not self.ada.active:
            return None
        st = dict(zip(R.ADA_KEYS, (int(v) for v in self.ada_state.tolist())))
        st["p"] = st["p24"] / float(R.ADA_ONE)
        st["r_t"] = st["r_acc"] / float(self.B * self.ada.interval)
        return st

    def sync_state_for_checkpoint(self) -> None:
        torch.cuda.synchronize(self.device)
        # the controller's state for the checkpoint dictionary (only with the controller on)
        self.model.ada = None
        if self.ada.adaptive:
            self.model.ada = {k: int(v) for k, v in zip(R.ADA_KEYS, self.ada_state.tolist())}

    def sync_bn_state(self) -> None:
        """Average BN moving averages over ranks (collective; see ReferenceEngine) -- and, after
        sharded updates, gather the conv kernels' fp32 masters and Adam slots (checkpoints)."""
        self.gather_sharded_state()
        D.all_reduce_mean_(self.model.g_bn.flat)
        D.all_reduce_mean_(self.model.d_bn.flat)

    def after_state_load(self) -> None:
        """Call after loading weights/slots from a checkpoint: refresh the 16-bit weight mirrors
        (the moving average's too) and, with spectral norm, the normalised copies from the loaded
        state. Adaptive augmentation: the controller's state from the loaded dictionary (``model.ada``;
        None = a checkpoint without one: the initial p), then rank 0's on every rank."""
        if self.ada.adaptive and not self.dry:
            st = getattr(self.model, "ada", None)
            vals = R.ada_state(R.ada_p24(self.ada.p)) if st is None else \
                [int(st[k]) for k in R.ADA_KEYS] + [0] * (R.ADA_STATE_WORDS - len(R.ADA_KEYS))
            self.ada_state.copy_(torch.tensor(vals, dtype=torch.int32))
            if self.ddp and D.is_initialized():
                D.broadcast_tensors([self.ada_state])
        self._repack_weights_now()

    def reset_d_sn(self) -> None:
        """Fresh spectral-norm state from the current weights (a checkpoint without one)."""
        if not self.dry:
            torch.cuda.synchronize(self.device)
        self.model.d_sn.reset(self.model.d.tensors, self.seed)
