"""Engine selection: the fused HIP engine on an MI355X (bf16, fp16 or fp32), the reference
(PyTorch autograd) engine on the CPU or when asked for explicitly.

Both expose the same small interface used by the trainer and ``bench.py``:
``set_synthetic_batch(real)``, ``set_batch(real)``, ``train_step()``, ``last_losses()``,
``model`` (parameters + BN state), ``opt_d``/``opt_g`` (TF-Adam state), ``global_step``.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from ..models.config import DCGANConfig
from ..models.dcgan import DCGAN
from ..ops import reference as R
from ..parallel import dist as D
from .reference_step import ReferenceStep


class ReferenceEngine:
    """Autograd reference step (PyTorch ops) + gloo/RCCL gradient averaging."""

    name = "reference"
    dtype_name = "fp32"

    def __init__(self, cfg: DCGANConfig, batch_size: int, device: torch.device, seed: int = 0,
                 lr: float = 2e-4, beta1: float = 0.5, zero_debias: bool = False, rank: int = 0,
                 world: int = 1, z_seed: Optional[int] = None, g_ema_decay: Optional[float] = None,
                 gan_loss: Optional[str] = None, label_smooth: Optional[float] = None,
                 d_spectral_norm: Optional[bool] = None, d_steps: Optional[int] = None,
                 beta2: Optional[float] = None, lr_d: Optional[float] = None, lr_g: Optional[float] = None,
                 lr_decay: Optional[str] = None,
                 lr_decay_start: Optional[int] = None, lr_decay_steps: Optional[int] = None,
                 lr_end: Optional[float] = None, lr_warmup: Optional[int] = None,
                 instance_noise: Optional[float] = None, instance_noise_end: Optional[float] = None,
                 instance_noise_steps: Optional[int] = None, d_augment: Optional[str] = None,
                 d_color_augment: Optional[str] = None, g_topk: Optional[float] = None,
                 g_topk_steps: Optional[int] = None, d_augment_p: Optional[float] = None,
                 ada_target: Optional[float] = None, ada_interval: Optional[int] = None,
                 ada_kimg: Optional[float] = None, **_):
        self.cfg = cfg
        self.batch_size = batch_size
        self.device = device
        self.seed = int(seed)
        self.model = DCGAN(cfg, device=device, seed=seed, zero_debias=zero_debias)
        self.world = world
        if d_spectral_norm is None:
            d_spectral_norm = R.env_spectral_norm()
        if R.check_spectral_norm(d_spectral_norm):
            self.model.enable_d_spectral_norm(seed)
        if world > 1:
            D.broadcast_tensors([self.model.g.flat, self.model.d.flat, self.model.g_bn.flat,
                                 self.model.d_bn.flat] + ([self.model.d_sn.flat] if self.model.d_sn else []))
        if g_ema_decay is None:  # (the HIP engine's switch, so both engines follow one environment)
            g_ema_decay = float(os.environ.get("DCGAN_G_EMA_DECAY") or 0.0)
        if gan_loss is None:
            gan_loss = os.environ.get("DCGAN_GAN_LOSS") or "bce"
        if label_smooth is None:
            label_smooth = float(os.environ.get("DCGAN_LABEL_SMOOTH") or 0.0)
        # D updates per G update, Adam's beta2, per-network learning rates: None = DCGAN_D_STEPS /
        # DCGAN_BETA2 / DCGAN_LR_D / DCGAN_LR_G, as the HIP engine
        d_steps, beta2, lr_d, lr_g = R.resolve_d_steps(d_steps, beta2, lr_d, lr_g, lr)
        # learning-rate schedule: None = DCGAN_LR_DECAY / _START / _STEPS / DCGAN_LR_END / DCGAN_LR_WARMUP
        self.lr_sched = R.resolve_lr_schedule(lr_decay, lr_decay_start, lr_decay_steps, lr_end, lr_warmup)
        # instance noise: None = DCGAN_INSTANCE_NOISE / _END / _STEPS; drawn from the HIP engine's seed
        # formula (HipEngine._zseed), so both engines add the same noise for the same flags
        self.noise = R.resolve_instance_noise(instance_noise, instance_noise_end, instance_noise_steps)
        # DiffAugment of D's inputs: None = DCGAN_D_AUGMENT; drawn from the same seed as the noise
        self.aug = R.resolve_d_augment(d_augment)
        self.color = R.resolve_d_color(d_color_augment)  # its color policy; None = DCGAN_D_COLOR_AUGMENT
        # adaptive augmentation probability: None = DCGAN_D_AUGMENT_P / DCGAN_ADA_TARGET / _INTERVAL / _KIMG
        self.ada = R.resolve_ada(d_augment_p, ada_target, ada_interval, ada_kimg,
                                 augmented=self.aug.active or self.color.active, batch_size=batch_size)
        # top-k generator updates: None = DCGAN_G_TOPK / DCGAN_G_TOPK_STEPS
        self.topk = R.resolve_g_topk(g_topk, g_topk_steps)
        zs = self.seed if z_seed is None else int(z_seed)
        self.step_impl = ReferenceStep(self.model, lr, beta1, grad_hook=self._allreduce if world > 1 else None,
                                       instance_noise=self.noise, noise_seed=zs * 1000003 + 17 + 7919 * rank,
                                       d_augment=self.aug, d_color_augment=self.color, g_topk=self.topk,
                                       d_ada=self.ada, world=world, g_ema_decay=g_ema_decay, gan_loss=gan_loss, label_smooth=label_smooth,
                                       d_spectral_norm=bool(d_spectral_norm), seed=seed, d_steps=d_steps,
                                       beta2=beta2, lr_d=lr_d, lr_g=lr_g, lr_decay=self.lr_sched)
        self.d_steps = self.step_impl.d_steps
        self.d_spectral_norm = self.step_impl.d_spectral_norm
        self.g_ema_decay = self.step_impl.g_ema_decay
        self.gan_loss, self.label_smooth = self.step_impl.gan_loss, self.step_impl.label_smooth
        self.opt_d, self.opt_g = self.step_impl.opt_d, self.step_impl.opt_g
        self.z_gen = torch.Generator(device=device if device.type == "cuda" else "cpu")
        self.z_gen.manual_seed((z_seed if z_seed is not None else seed) + 7919 * rank + 1)
        self._reals = [None] * self.d_steps  # slot k < d_steps - 1: D sub-step k's batch; last: the full step's
        self._losses: Dict[str, float] = {}

    def _allreduce(self, which: str, flat: torch.Tensor) -> None:
        D.all_reduce_mean_(flat)

    @property
    def global_step(self) -> int:
        return self.step_impl.global_step

    @global_step.setter
    def global_step(self, v: int) -> None:
        self.step_impl.global_step = int(v)

    @property
    def _real(self):
        return self._reals[-1]

    def set_synthetic_batch(self, real: torch.Tensor) -> None:
        self._reals = [real.to(self.device, torch.float32)] * self.d_steps

    def set_batch(self, real: torch.Tensor, slot: int = 0) -> None:
        """Slot k < d_steps - 1 is D sub-step k's batch, slot d_steps - 1 the full step's."""
        if not 0 <= slot < self.d_steps:
            raise ValueError("batch slot %d out of range for d_steps = %d" % (slot, self.d_steps))
        self._reals[slot] = real.to(self.device, torch.float32, non_blocking=True)

    def sample_z(self, n: int) -> torch.Tensor:
        return torch.rand(n, self.cfg.z_dim, generator=self.z_gen, device=self.device) * 2 - 1

    def train_d_step(self, k: int) -> None:
        """D sub-step k alone (its losses: last_losses())."""
        z = self.sample_z(self._reals[k].shape[0])
        self._last_z = z
        self._losses = self.step_impl.d_step(self._reals[k], z, sub=k)

    def train_step(self) -> None:
        for k in range(self.d_steps - 1):
            self.train_d_step(k)
        z = self.sample_z(self._real.shape[0])
        self._last_z = z
        self._losses = self.step_impl.step(self._real, z)

    def activations(self) -> "Dict[str, torch.Tensor]":
        """Re-run the last step's forward (pre-update weights are gone; uses current ones,
        no EMA update) and return the summary tensors."""
        from collections import OrderedDict
        rec: Dict[str, torch.Tensor] = {}
        B = self._real.shape[0]
        with torch.no_grad():
            out = self.step_impl.forward_losses(self._real, self._last_z, update_ema=False, record=rec, noise=False,
                                                augment=False, color=False, topk=False)
        a = OrderedDict()
        a["z"] = self._last_z
        a["d"] = torch.sigmoid(out["logits_real"])
        a["d_"] = torch.sigmoid(out["logits_fake"])
        a["G"] = out["fake"]
        a["g_h0_relu"] = rec["g_h0"]
        gl = self.cfg.g_layers()
        for L in gl[:-1]:
            a[L.name + "_relu"] = rec[L.name]
        a[gl[-1].name] = rec[gl[-1].name]
        for L in self.cfg.d_layers():
            a[L.name] = rec[L.name][:B]
        a[self.cfg.d_lin_name] = out["logits_real"]
        return a

    def last_losses(self) -> Dict[str, float]:
        return dict(self._losses)

    def noise_sigma(self) -> float:
        """sigma(t) of the instance noise at the current global step (0.0 when off)."""
        return self.step_impl.noise_sigma()

    def topk_selection(self) -> Optional[torch.Tensor]:
        """The bool mask [B] of the fakes G learned from in the last full step (None: top-k off)."""
        sel = self.step_impl.last.get("topk_sel") if self.topk.active else None
        return None if sel is None else sel.clone()

    def last_topk(self):
        """(k, g_loss_topk, threshold logit) of the last full step; None when top-k is off."""
        sel = self.topk_selection()
        if sel is None:
            return None
        last = self.step_impl.last
        k = int(sel.sum())
        return k, float(last["g_loss_topk"].detach()), float(R.topk_threshold(last["logits_fake"].detach(), k))

    @property
    def g_ema(self):
        """Moving average of G's weights (a ParamSet laid out like model.g), None when off."""
        return self.model.g_ema

    def sampler(self, z: torch.Tensor, ema: Optional[bool] = None) -> torch.Tensor:
        return self.model.sampler(z.to(self.device), ema=ema)

    def eval_losses(self, real: torch.Tensor, z: torch.Tensor) -> Dict[str, float]:
        """Sample-time d_loss/g_loss (image_train.py:181-184) without mutating BN EMAs."""
        with torch.no_grad():
            out = self.step_impl.forward_losses(real.to(self.device, torch.float32), z.to(self.device),
                                                update_ema=False, noise=False, augment=False, color=False,
                                                topk=False)
        return {"d_loss": float(out["d_loss"]), "g_loss": float(out["g_loss"])}

    def ada_status(self):
        """The adaptive-augmentation state {p24, acc, cnt, r_acc, windows, p, r_t}; None when off."""
        if not self.ada.active:
            return None
        st = dict(zip(R.ADA_KEYS, self.step_impl.ada_state))
        st["p"] = st["p24"] / float(R.ADA_ONE)
        st["r_t"] = st["r_acc"] / float(self.batch_size * self.ada.interval)
        return st

    def sync_state_for_checkpoint(self) -> None:
        self.model.ada = dict(zip(R.ADA_KEYS, self.step_impl.ada_state)) if self.ada.adaptive else None

    def after_state_load(self) -> None:
        """Adaptive augmentation: the controller's state from the loaded dictionary (None: the initial p)."""
        if self.ada.adaptive:
            st = getattr(self.model, "ada", None)
            self.step_impl.ada_state = R.ada_state(R.ada_p24(self.ada.p)) if st is None else \
                [int(st[k]) for k in R.ADA_KEYS] + [0] * (R.ADA_STATE_WORDS - len(R.ADA_KEYS))

    def sync_check_tensors(self):
        """What the cross-rank divergence check compares."""
        return [self.model.g.flat, self.model.d.flat] + ([self.model.d_sn.flat] if self.model.d_sn else [])

    def reset_d_sn(self) -> None:
        """Fresh spectral-norm state from the current weights (a checkpoint without one)."""
        self.model.d_sn.reset(self.model.d.tensors, self.seed)

    def sync_bn_state(self) -> None:
        """Average the BN moving averages over ranks (collective; every rank must call it).
        Each rank tracks its own local-batch statistics; the reference's shared PS copy saw
        every worker's updates, which the mean over ranks approximates."""
        D.all_reduce_mean_(self.model.g_bn.flat)
        D.all_reduce_mean_(self.model.d_bn.flat)


def build_engine(cfg: DCGANConfig, batch_size: int, device: torch.device, engine: str = "auto",
                 dtype: str = "bf16", seed: int = 0, rank: int = 0, world: int = 1, graph: bool = True,
                 allreduce_dtype: str = "fp32", lr: float = 2e-4, beta1: float = 0.5,
                 zero_debias: bool = False, bucket_mb: float = 32.0, g_ema_decay: Optional[float] = None,
                 gan_loss: Optional[str] = None, label_smooth: Optional[float] = None,
                 d_spectral_norm: Optional[bool] = None, d_steps: Optional[int] = None,
                 beta2: Optional[float] = None, lr_d: Optional[float] = None, lr_g: Optional[float] = None,
                 lr_decay: Optional[str] = None,
                 lr_decay_start: Optional[int] = None, lr_decay_steps: Optional[int] = None,
                 lr_end: Optional[float] = None, lr_warmup: Optional[int] = None,
                 instance_noise: Optional[float] = None, instance_noise_end: Optional[float] = None,
                 instance_noise_steps: Optional[int] = None, d_augment: Optional[str] = None,
                 d_color_augment: Optional[str] = None, g_topk: Optional[float] = None,
                 g_topk_steps: Optional[int] = None, d_augment_p: Optional[float] = None,
                 ada_target: Optional[float] = None, ada_interval: Optional[int] = None,
                 ada_kimg: Optional[float] = None):
    ada_kw = dict(d_augment_p=d_augment_p, ada_target=ada_target, ada_interval=ada_interval, ada_kimg=ada_kimg)
    if engine == "auto":  # every dtype (bf16 / fp16 / fp32) runs on the HIP kernels on an MI355X
        engine = "hip" if device.type == "cuda" else "reference"
    if engine == "reference":
        return ReferenceEngine(cfg, batch_size, device, seed=seed, lr=lr, beta1=beta1,
                               zero_debias=zero_debias, rank=rank, world=world, g_ema_decay=g_ema_decay,
                               gan_loss=gan_loss, label_smooth=label_smooth, d_spectral_norm=d_spectral_norm,
                               d_steps=d_steps, beta2=beta2, lr_d=lr_d, lr_g=lr_g, lr_decay=lr_decay,
                               lr_decay_start=lr_decay_start, lr_decay_steps=lr_decay_steps, lr_end=lr_end,
                               lr_warmup=lr_warmup, instance_noise=instance_noise,
                               instance_noise_end=instance_noise_end, instance_noise_steps=instance_noise_steps,
                               d_augment=d_augment, d_color_augment=d_color_augment, g_topk=g_topk,
                               g_topk_steps=g_topk_steps, **ada_kw)
    if engine == "hip":
        from .hip_engine import HipEngine
        return HipEngine(cfg, batch_size, device, dtype=dtype, seed=seed, lr=lr, beta1=beta1,
                         zero_debias=zero_debias, rank=rank, world=world, graph=graph,
                         allreduce_dtype=allreduce_dtype, bucket_mb=bucket_mb, g_ema_decay=g_ema_decay,
                         gan_loss=gan_loss, label_smooth=label_smooth, d_spectral_norm=d_spectral_norm,
                         d_steps=d_steps, beta2=beta2, lr_d=lr_d, lr_g=lr_g, lr_decay=lr_decay,
                         lr_decay_start=lr_decay_start, lr_decay_steps=lr_decay_steps, lr_end=lr_end,
                         lr_warmup=lr_warmup, instance_noise=instance_noise,
                         instance_noise_end=instance_noise_end, instance_noise_steps=instance_noise_steps,
                         d_augment=d_augment, d_color_augment=d_color_augment, g_topk=g_topk,
                         g_topk_steps=g_topk_steps, **ada_kw)
    raise ValueError("unknown engine %r" % engine)
