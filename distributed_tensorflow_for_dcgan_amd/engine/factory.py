"""Engine selection: the fused HIP engine on an MI355X (bf16, fp16 or fp32), the reference
(PyTorch autograd) engine on the CPU or when asked for explicitly.

Both expose the same small interface used by the trainer and ``bench.py``:
``set_synthetic_batch(real)``, ``set_batch(real)``, ``train_step()``, ``last_losses()``,
``model`` (parameters + BN state), ``opt_d``/``opt_g`` (TF-Adam state), ``global_step``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..models.config import DCGANConfig
from ..models.dcgan import DCGAN
from ..ops import options as O
from ..ops import reference as R
from ..parallel import dist as D
from .reference_step import ReferenceStep


class ReferenceEngine:
    """Autograd reference step (PyTorch ops) + gloo/RCCL gradient averaging."""

    name = "reference"
    dtype_name = "fp32"

    def __init__(self, cfg: DCGANConfig, batch_size: int, device: torch.device, seed: int = 0,
                 lr: float = 2e-4, beta1: float = 0.5, zero_debias: bool = False, rank: int = 0,
                 world: int = 1, z_seed: Optional[int] = None, **options):
        self.cfg = cfg
        self.batch_size = batch_size
        self.device = device
        self.seed = int(seed)
        self.model = DCGAN(cfg, device=device, seed=seed, zero_debias=zero_debias)
        self.world = world
        # the training options (ops.options.TABLE; None = the environment's default, as the HIP engine),
        # published as self.noise, self.aug, self.ada, self.d_steps, self.gan_loss, ...
        self.options = O.resolve(batch_size, lr=lr, beta1=beta1, **O.known(options))
        vars(self).update(self.options._asdict())
        if self.d_spectral_norm:
            self.model.enable_d_spectral_norm(seed)
        if world > 1:
            D.broadcast_tensors([self.model.g.flat, self.model.d.flat, self.model.g_bn.flat,
                                 self.model.d_bn.flat] + ([self.model.d_sn.flat] if self.model.d_sn else []))
        # the instance noise and DiffAugment draw from the HIP engine's seed formula (HipEngine._zseed),
        # so both engines add the same noise for the same flags
        zs = self.seed if z_seed is None else int(z_seed)
        self.step_impl = ReferenceStep(self.model, grad_hook=self._allreduce if world > 1 else None,
                                       options=self.options, noise_seed=zs * 1000003 + 17 + 7919 * rank,
                                       world=world, seed=seed)
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
                 zero_debias: bool = False, bucket_mb: float = 32.0, **options):
    """options: the training options (ops.options.TABLE), forwarded to the engine as they are."""
    if engine == "auto":  # every dtype (bf16 / fp16 / fp32) runs on the HIP kernels on an MI355X
        engine = "hip" if device.type == "cuda" else "reference"
    if engine == "reference":
        return ReferenceEngine(cfg, batch_size, device, seed=seed, lr=lr, beta1=beta1,
                               zero_debias=zero_debias, rank=rank, world=world, **options)
    if engine == "hip":
        from .hip_engine import HipEngine
        return HipEngine(cfg, batch_size, device, dtype=dtype, seed=seed, lr=lr, beta1=beta1,
                         zero_debias=zero_debias, rank=rank, world=world, graph=graph,
                         allreduce_dtype=allreduce_dtype, bucket_mb=bucket_mb, **options)
    raise ValueError("unknown engine %r" % engine)
