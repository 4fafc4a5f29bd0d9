"""Reference (autograd) GAN training step -- the oracle for the fused HIP engine.

Semantics = ``image_train.py:151-158``: ONE forward of G,
D(real), D(fake) (separate BN statistics per D call), ``d_loss = d_real + d_fake``,
``g_loss`` non-saturating; D grads from ``d_loss`` w.r.t. ``d_`` vars, G grads from
``g_loss`` w.r.t. ``g_`` vars through D(fake) with *pre-update* D weights; both TF-Adam
updates applied in the same step; ``global_step`` incremented once (by G's optimiser).

Runs on any device (CPU for tests/plumbing, or GPU through PyTorch ops) and is also the
fallback engine when no HIP extension is available on CPU.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from ..models.dcgan import DCGAN
from ..ops import options as O
from ..ops import reference as R
from ..optim.adam import TFAdam


class ReferenceStep:
    def __init__(self, model: DCGAN, lr: float = 2e-4, beta1: float = 0.5,
                 grad_hook: Optional[Callable[[str, torch.Tensor], None]] = None,
                 options: Optional[O.StepOptions] = None, noise_seed: int = 0, seed: int = 0, world: int = 1,
                 d_ada=None, **keywords):
        """options: the resolved record; else `keywords` are the training options (ops.options.TABLE;
        d_ada: the ADA group as an ops.reference.DAda), at their defaults where not given -- the
        environment is never read here."""
        self.model = model
        if options is None:
            if d_ada is not None:
                keywords["d_augment_p"] = d_ada
            options = O.resolve(env=False, lr=lr, beta1=beta1, **keywords)
        o = self.options = options
        # top-k generator updates (ops.reference.GTopK): g_loss is differentiated over the k(t) fakes D
        # scores highest only, k annealed from B to ceil(nu B) over the global step; D's losses and
        # gradients and the reported g_loss stay those of all B samples
        self.topk = o.topk
        # DiffAugment (ops.reference.DAugment): D sees augment([real | fake]) -- translation and / or
        # cutout, drawn per sample from Philox stream 2 of `noise_seed` at the global step (D sub-step
        # k: substep_seed(noise_seed, k)) -- before the additive noise; G's gradient flows through it
        self.aug = o.aug
        # its color policy (ops.reference.DColor), ahead of translation / cutout: brightness, saturation,
        # contrast per sample, (b, s, c) from Philox stream 3 of the same seed at the global step
        self.color = o.color
        # adaptive augmentation probability (ops.reference.DAda): each selected policy applies to a sample
        # iff its gate -- Philox streams 4 (translation, cutout) and 5 (color) of the same seed -- falls
        # below p24; with a target, ``step`` steers p24 from its own real logits (ops.reference.ada_update),
        # `world` entering the step size only. D sub-steps gate with the live p24 and leave the state alone
        self.ada = o.ada
        self.ada_world = int(world)
        self.ada_state = R.ada_state(R.ada_p24(self.ada.p))
        # instance noise (ops.reference.InstanceNoise): D sees [real | fake] + sigma(t) * eps, eps from
        # Philox stream 1 of `noise_seed` (the HIP engine's z seed) at the global step; D sub-step k
        # draws from ops.reference.substep_seed(noise_seed, k). G's gradient flows through it unchanged
        self.noise = o.noise
        self.noise_seed = int(noise_seed)
        self._sub_k = 0  # D sub-steps taken since the last full step
        # learning-rate schedule (ops.reference.LrSchedule): both Adam rates times lr_factor at the
        # global step before its increment; the D sub-steps see the step of the full step after them
        self.lr_sched = o.lr_sched
        # discriminator updates per generator update (d_steps - 1 D sub-steps, ``d_step``, before
        # each full ``step``), Adam's beta2 and the per-network learning rates (TTUR)
        self.d_steps, self.beta2, self.lr_d, self.lr_g = o.d_steps, o.beta2, o.lr_d, o.lr_g
        # spectral normalisation of D's conv kernels and head (model.d_sn; ops.reference.sn_power /
        # spectral_normalize): D computes with W / sigma(W), one power step after each Adam(D)
        self.d_spectral_norm = o.d_spectral_norm
        if self.d_spectral_norm and model.d_sn is None:
            model.enable_d_spectral_norm(seed)
        # objective (ops.reference.gan_losses): bce | lsgan | hinge, D's real target = 1 - label_smooth
        self.gan_loss, self.label_smooth = o.gan_loss, o.label_smooth
        # moving average of G's weights (model.g_ema; ops.reference.ema_update_), 0 = none kept
        self.g_ema_decay = o.g_ema_decay
        if self.g_ema_decay > 0:
            model.g_ema = model.g.like()
            model.g_ema.flat.copy_(model.g.flat)
        self.opt_d = TFAdam(model.d, self.lr_d, o.beta1, self.beta2, power_suffix="")
        self.opt_g = TFAdam(model.g, self.lr_g, o.beta1, self.beta2, power_suffix="_1")
        self.global_step = 0
        self.grad_hook = grad_hook  # e.g. DDP all-reduce of the flat grad buffer
        self.last: Dict[str, torch.Tensor] = {}

    def lr_factor(self) -> float:
        """The schedule's factor (fp32 oracle) at the current global step."""
        return float(R.lr_factor(self.lr_sched, self.global_step)) if self.lr_sched.active else 1.0

    def noise_sigma(self) -> float:
        """sigma(t) of the instance noise (fp32 oracle) at the current global step; 0.0 when off."""
        n = self.noise
        return float(R.noise_sigma(self.global_step, n.sigma0, n.sigma1, n.steps)) if n.active else 0.0

    def topk_k(self, B: int) -> int:
        """k(t) of the top-k selection among B fakes at the current global step; B when it is off."""
        if not self.topk.active:
            return int(B)
        return R.topk_k(self.global_step, B, R.topk_kmin(B, self.topk.nu), self.topk.steps)

    def draw_noise(self, shape, sub: Optional[int] = None) -> Optional[torch.Tensor]:
        """The additive sigma(t) * eps over a [2B, ...] input at the current global step: the full
        step's (sub None) or D sub-step `sub`'s; None when the noise is off."""
        if not self.noise.active:
            return None
        return R.instance_noise(shape, self.noise, R.substep_seed(self.noise_seed, sub), self.global_step)

    def draw_augment(self, shape, sub: Optional[int] = None) -> Optional[torch.Tensor]:
        """The augmentation's params int64 [2B, 4] = (ty, tx, oy, ox) over a [2B, S, S, C] input at the
        current global step: the full step's (sub None) or D sub-step `sub`'s; None when it is off."""
        if not self.aug.active:
            return None
        return R.augment_params(shape[0], shape[1], R.substep_seed(self.noise_seed, sub), self.global_step)

    def draw_color(self, shape, sub: Optional[int] = None) -> Optional[torch.Tensor]:
        """The color policy's params float32 [2B, 3] = (b, s, c) over a [2B, S, S, C] input at the current
        global step: the full step's (sub None) or D sub-step `sub`'s; None when it is off."""
        if not self.color.active:
            return None
        return R.color_params(shape[0], R.substep_seed(self.noise_seed, sub), self.global_step)

    def draw_gates(self, n: int, sub: Optional[int] = None):
        """(color gates, geometric gates), int32 [2B] each (None where that switch is off), at the current
        global step and p24; None when no gate is active."""
        if not self.ada.active:
            return None
        seed, p24 = R.substep_seed(self.noise_seed, sub), self.ada_state[0]
        cg = R.gate_masks(n, seed, self.global_step, R.COLOR_GATE_STREAM, p24, self.color.mask) if self.color.active else None
        ag = R.gate_masks(n, seed, self.global_step, R.AUG_GATE_STREAM, p24, self.aug.mask) if self.aug.active else None
        return cg, ag

    def forward_losses(self, real: torch.Tensor, z: torch.Tensor, Pg=None, Pd=None, update_ema=True,
                       record=None, update_ema_g=None, noise=None, sub: Optional[int] = None, augment=None,
                       color=None, topk=None, gates=None):
        """update_ema: D's BN moving averages; update_ema_g: G's (None = as D's). noise: the additive
        sigma * eps on D's input [2B, ...]; None = drawn (``draw_noise``, `sub` = the D sub-step) when
        instance noise is on; False = none (sample-time losses stay clean). augment: the params [2B, 4]
        of DiffAugment, applied before the noise; None = drawn (``draw_augment``) when it is on; False =
        none. color: the params [2B, 3 or 4] of the color policy, applied before `augment`; None = drawn
        (``draw_color``) when it is on; False = none. topk: the bool mask [B] of the fakes G learns from;
        None = the selection on this forward's own fake logits (``topk_k`` of them) when top-k is on; False
        = none. The result carries it as ``topk_sel`` (None when unused) beside ``g_loss_topk``, the mean
        of G's loss over the selected (``g_loss`` itself when unused). gates: (color gates, geometric
        gates) of adaptive augmentation, int [2B] each or None; None = drawn (``draw_gates``) when it is on;
        False = none."""
        m = self.model
        if self.d_spectral_norm:  # D computes with W / sigma(W); autograd projects the gradient
            Pd = m.d_sn_weights(Pd)
        fake = m.generator(z, train=True, P=Pg, update_ema=update_ema if update_ema_g is None else update_ema_g,
                           record=record)
        B = real.shape[0]
        both = torch.cat([real, fake], 0)
        if gates is None:
            gates = self.draw_gates(both.shape[0], sub)
        cg, ag = (None, None) if gates is None or gates is False else gates
        if color is None:
            color = self.draw_color(both.shape, sub)
        if color is not None and color is not False:
            both = R.color_augment(both, color, self.color, gates=cg)
        if augment is None:
            augment = self.draw_augment(both.shape, sub)
        if augment is not None and augment is not False:
            both = R.augment(both, augment, self.aug, gates=ag)
        if noise is None:
            noise = self.draw_noise(both.shape, sub)
        if noise is not None and noise is not False:
            both = both + noise.to(both.device, both.dtype)
        _, logits = m.discriminator(both, groups=2, slots=(0, 1), train=True, P=Pd,
                                    update_ema=update_ema, record=record)
        lr_, lf = logits[:B], logits[B:]
        d_real, d_fake, g_loss, d_loss = R.gan_losses(lr_, lf, self.gan_loss, self.label_smooth)
        if topk is None:
            topk = R.topk_select(lf, self.topk_k(B)) if self.topk.active else False
        if topk is False:
            topk, g_topk = None, g_loss
        else:
            topk = torch.as_tensor(topk).to(lf.device, torch.bool).reshape(-1)
            g_topk = R.topk_g_loss(lf, topk, self.gan_loss)
        return {"fake": fake, "logits_real": lr_, "logits_fake": lf, "d_loss_real": d_real,
                "d_loss_fake": d_fake, "g_loss": g_loss, "d_loss": d_loss, "g_loss_topk": g_topk, "topk_sel": topk}

    def compute_grads(self, real: torch.Tensor, z: torch.Tensor, update_ema: bool = True, noise=None, augment=None,
                      color=None, topk=None, gates=None):
        """Returns (losses dict, flat D grads, flat G grads) without applying them. G's gradients are
        those of ``g_loss_topk`` (which is ``g_loss`` without a top-k selection)."""
        m = self.model
        Pg = {k: v.detach().clone().requires_grad_(True) for k, v in m.g.tensors.items()}
        Pd = {k: v.detach().clone().requires_grad_(True) for k, v in m.d.tensors.items()}
        out = self.forward_losses(real, z, Pg, Pd, update_ema=update_ema, noise=noise, augment=augment, color=color,
                                  topk=topk, gates=gates)
        d_names, g_names = m.d.names(), m.g.names()
        dg = torch.autograd.grad(out["d_loss"], [Pd[n] for n in d_names], retain_graph=True,
                                 allow_unused=True)
        gg = torch.autograd.grad(out["g_loss_topk"], [Pg[n] for n in g_names], allow_unused=True)
        gd_flat = m.d.like()
        gg_flat = m.g.like()
        for n, g in zip(d_names, dg):
            if g is not None:
                gd_flat[n].copy_(g)
        for n, g in zip(g_names, gg):
            if g is not None:
                gg_flat[n].copy_(g)
        return out, gd_flat.flat, gg_flat.flat

    def compute_d_grads(self, real: torch.Tensor, z: torch.Tensor, noise=None, sub: Optional[int] = None,
                        augment=None, color=None, gates=None):
        """(losses dict, flat D grads) of a D sub-step: G's forward in training mode on batch
        statistics with its BN moving averages left alone, only d_loss differentiated, through D."""
        m = self.model
        Pd = {k: v.detach().clone().requires_grad_(True) for k, v in m.d.tensors.items()}
        out = self.forward_losses(real, z, None, Pd, update_ema=True, update_ema_g=False, noise=noise,
                                  sub=self._sub_k if sub is None else sub, augment=augment, color=color, topk=False,
                                  gates=gates)
        d_names = m.d.names()
        dg = torch.autograd.grad(out["d_loss"], [Pd[n] for n in d_names], allow_unused=True)
        gd_flat = m.d.like()
        for n, g in zip(d_names, dg):
            if g is not None:
                gd_flat[n].copy_(g)
        return out, gd_flat.flat

    def d_step(self, real: torch.Tensor, z: torch.Tensor, noise=None, sub: Optional[int] = None,
               augment=None, color=None, gates=None) -> Dict[str, float]:
        """One D sub-step: a fresh z through G, D on [real | fake], the d_loss backward through D,
        TF-Adam(D) (D's beta powers advance) and the power step. Nothing of G changes -- parameters,
        Adam slots and powers, BN moving averages, weight EMA -- nor does the global step; D's BN
        moving averages (both slots) update as in a full step."""
        out, gd = self.compute_d_grads(real, z, noise=noise, sub=sub, augment=augment, color=color, gates=gates)
        self._sub_k += 1
        for s in range(2):
            self.model.d_bn.count_step(s)
        if self.grad_hook is not None:
            self.grad_hook("d", gd)
        self.opt_d.step(gd, self.lr_factor())
        if self.d_spectral_norm:
            self.model.d_sn.power_step_(self.model.d.tensors)
        self.last = out
        return {k: float(out[k].detach()) for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss")}

    def ada_step(self, real_logits: torch.Tensor) -> None:
        """The controller's step of a full training step, from that step's real logits (no-op without a
        target)."""
        if not self.ada.adaptive:
            return
        a, B = self.ada, int(real_logits.numel())
        self.ada_state = R.ada_update(self.ada_state, real_logits, R.ada_threshold(self.gan_loss, self.label_smooth),
                                      R.ada_target_n(a.target, B, a.interval),
                                      R.ada_delta24(self.ada_world, B, a.interval, a.kimg), a.interval)

    def step(self, real: torch.Tensor, z: torch.Tensor, noise=None, augment=None, color=None,
             topk=None, gates=None) -> Dict[str, float]:
        """topk: the mask of the fakes G learns from (an engine's recorded one); None = the reference's
        own selection when top-k is on; False = none."""
        out, gd, gg = self.compute_grads(real, z, noise=noise, augment=augment, color=color, topk=topk, gates=gates)
        self.ada_step(out["logits_real"].detach())  # (follows the global step, whatever the update does)
        self._sub_k = 0
        for s in range(2):  # one EMA update per BN slot per step (as the HIP engine counts)
            self.model.d_bn.count_step(s)
        self.model.g_bn.count_step(0)
        if self.grad_hook is not None:
            self.grad_hook("d", gd)
            self.grad_hook("g", gg)
        f = self.lr_factor()
        self.opt_d.step(gd, f)
        self.opt_g.step(gg, f)
        self.global_step += 1
        if self.d_spectral_norm:  # after Adam(D): one power step on the new weights
            self.model.d_sn.power_step_(self.model.d.tensors)
        if self.g_ema_decay > 0:  # after Adam(G), with the step count after its increment
            with torch.no_grad():
                R.ema_update_(self.model.g_ema.flat, self.model.g.flat, self.g_ema_decay, self.global_step)
        self.last = out
        return {k: float(out[k].detach()) for k in ("d_loss_real", "d_loss_fake", "g_loss", "d_loss")}
