"""TF-exact reference ops in plain PyTorch (NHWC, any device, any float dtype).

These are the semantics contract and the oracle every HIP kernel
is tested against. They reproduce, with explicit padding/cropping:

* ``tf.nn.conv2d(..., padding='SAME')`` with HWIO weights (``distriubted_model.py:183``):
  asymmetric TF padding (pad_lo, pad_hi) -- *not* PyTorch's symmetric ``padding=2``.
* ``tf.nn.conv2d_transpose`` with ``[kh, kw, out, in]`` weights (``:200-201``): the exact
  adjoint of the SAME conv = full transposed conv cropped to ``[pad_lo : pad_lo + out]``.
* ``batch_norm_with_global_normalization`` with biased batch moments over N,H,W (``:37,49``).
* ``lrelu`` = max(x, leak*x) (``:157``), ``sigmoid_cross_entropy_with_logits``
  (``image_train.py:91-95``).
"""
from __future__ import annotations

import math
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ..models.config import same_pads


def conv2d_same(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None,
                stride: int = 2) -> torch.Tensor:
    """x: [B,H,W,Cin] NHWC, w: [kh,kw,Cin,Cout] (HWIO) -> [B,ceil(H/s),ceil(W/s),Cout]."""
    kh, kw = w.shape[0], w.shape[1]
    ph = same_pads(x.shape[1], kh, stride)
    pw = same_pads(x.shape[2], kw, stride)
    xn = x.permute(0, 3, 1, 2)
    xn = F.pad(xn, (pw[0], pw[1], ph[0], ph[1]))
    y = F.conv2d(xn, w.permute(3, 2, 0, 1), None, stride=stride)
    y = y.permute(0, 2, 3, 1)
    if b is not None:
        y = y + b
    return y


def conv2d_transpose_same(x: torch.Tensor, w: torch.Tensor, out_hw: Tuple[int, int],
                          b: Optional[torch.Tensor] = None, stride: int = 2) -> torch.Tensor:
    """x: [B,Hi,Wi,Cin], w: [kh,kw,Cout,Cin] -> [B,Ho,Wo,Cout] (TF 'SAME' conv2d_transpose)."""
    kh, kw = w.shape[0], w.shape[1]
    ho, wo = out_hw
    ph = same_pads(ho, kh, stride)
    pw = same_pads(wo, kw, stride)
    xn = x.permute(0, 3, 1, 2)
    full = F.conv_transpose2d(xn, w.permute(3, 2, 0, 1), None, stride=stride)
    y = full[:, :, ph[0]:ph[0] + ho, pw[0]:pw[0] + wo]
    y = y.permute(0, 2, 3, 1)
    if b is not None:
        y = y + b
    return y


def moments(x: torch.Tensor, groups: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-group, per-channel biased mean/variance over (N,H,W) (or (N) for 2-D x).

    ``groups`` splits the batch into equal contiguous groups with independent statistics
    (used to run D's real and fake passes as one 2B batch while keeping TF's separate
    per-call statistics). Returns [groups, C] tensors.
    """
    C = x.shape[-1]
    xg = x.reshape(groups, -1, C)
    mean = xg.mean(dim=1)
    var = (xg - mean[:, None, :]).pow(2).mean(dim=1)
    return mean, var


def batch_norm(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, beta: torch.Tensor,
               gamma: torch.Tensor, eps: float = 1e-5, groups: int = 1) -> torch.Tensor:
    """TF batch_norm_with_global_normalization(scale_after_normalization=True).

    mean/var: [C] or [groups, C]."""
    if mean.dim() == 1:
        return (x - mean) * torch.rsqrt(var + eps) * gamma + beta
    shp = x.shape
    C = shp[-1]
    xg = x.reshape(groups, -1, C)
    y = (xg - mean[:, None, :]) * torch.rsqrt(var[:, None, :] + eps) * gamma + beta
    return y.reshape(shp)


def lrelu(x: torch.Tensor, leak: float = 0.2) -> torch.Tensor:
    return torch.maximum(x, leak * x)


def sigmoid_cross_entropy_with_logits(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """TF formula: max(x,0) - x*t + log(1 + exp(-|x|))."""
    return logits.clamp(min=0) - logits * targets + torch.log1p(torch.exp(-logits.abs()))


GAN_LOSSES = ("bce", "lsgan", "hinge")  # (the position is the kernel's objective id, ops.hip.GAN_LOSS_IDS)


def check_gan_loss(kind, label_smooth=0.0):
    """Validated (objective name, one-sided label smoothing s): a known name, 0 <= s < 0.5, and no
    smoothing with hinge (its real-side margin is not a target that could be smoothed)."""
    if not isinstance(kind, str) or kind not in GAN_LOSSES:
        raise ValueError("gan_loss must be one of %s, got %r" % ("|".join(GAN_LOSSES), kind))
    s = float(label_smooth)
    if not 0.0 <= s < 0.5:
        raise ValueError("label_smooth must satisfy 0 <= s < 0.5, got %r" % (label_smooth,))
    if kind == "hinge" and s > 0:
        raise ValueError("label_smooth > 0 is not defined for gan_loss=hinge (got %r)" % (label_smooth,))
    return kind, s


def gan_losses(d_logits_real: torch.Tensor, d_logits_fake: torch.Tensor, kind: str = "bce",
               label_smooth: float = 0.0):
    """(d_loss_real, d_loss_fake, g_loss, d_loss). ``bce`` (default) is image_train.py:91-96 exactly;
    ``lsgan`` the least-squares and ``hinge`` the hinge objective. ``label_smooth`` s lowers D's
    real target to t = 1 - s (one-sided: neither the fake target nor G's target moves)."""
    kind, s = check_gan_loss(kind, label_smooth)
    xr, xf = d_logits_real, d_logits_fake
    t = 1.0 - s
    if kind == "bce":
        d_real = sigmoid_cross_entropy_with_logits(xr, torch.full_like(xr, t)).mean()
        d_fake = sigmoid_cross_entropy_with_logits(xf, torch.zeros_like(xf)).mean()
        g = sigmoid_cross_entropy_with_logits(xf, torch.ones_like(xf)).mean()
    elif kind == "lsgan":
        d_real = 0.5 * (xr - t).pow(2).mean()
        d_fake = 0.5 * xf.pow(2).mean()
        g = 0.5 * (xf - 1.0).pow(2).mean()
    else:
        d_real = torch.relu(1.0 - xr).mean()
        d_fake = torch.relu(1.0 + xf).mean()
        g = -xf.mean()
    return d_real, d_fake, g, d_real + d_fake


def tf_adam_update(param: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                   beta1_power: float, beta2_power: float, lr: float, beta1: float,
                   beta2: float = 0.999, eps: float = 1e-8) -> None:
    """One TF ``ApplyAdam`` (in place). beta*_power are the values *before* this step's
    update, i.e. beta^t for the t-th step (TF keeps them as variables initialised to beta)."""
    lr_t = lr * (1.0 - beta2_power) ** 0.5 / (1.0 - beta1_power)
    m.mul_(beta1).add_(grad, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
    param.sub_(lr_t * m / (v.sqrt() + eps))


def env_value(name, conv):
    """conv(environment variable `name`); None when it is unset or empty. Read at call time."""
    v = os.environ.get(name)
    if v is None or v.strip() == "":
        return None
    try:
        return conv(v)
    except ValueError:
        raise ValueError("%s=%r is not a number" % (name, v)) from None


ADAM_BETA2 = 0.999   # TF-Adam's beta2 where none is given (optim.adam.TFAdam's default)
MAX_D_STEPS = 16


def check_d_steps(d_steps=1, beta2=ADAM_BETA2, lr_d=None, lr_g=None, lr=2e-4):
    """Validated (d_steps, beta2, lr_d, lr_g): 1 <= d_steps <= 16 discriminator updates per generator
    update, 0 <= beta2 < 1, and the per-network learning rates -- None or 0 = the common `lr`,
    negative values are errors."""
    if isinstance(d_steps, bool) or int(d_steps) != d_steps or not 1 <= int(d_steps) <= MAX_D_STEPS:
        raise ValueError("d_steps must be an integer with 1 <= d_steps <= %d, got %r" % (MAX_D_STEPS, d_steps))
    b2 = float(beta2)
    if not 0.0 <= b2 < 1.0:
        raise ValueError("beta2 must satisfy 0 <= beta2 < 1, got %r" % (beta2,))
    if not float(lr) >= 0.0:
        raise ValueError("learning_rate must not be negative, got %r" % (lr,))
    out = []
    for name, v in (("d_learning_rate", lr_d), ("g_learning_rate", lr_g)):
        v = 0.0 if v is None else float(v)
        if not v >= 0.0:
            raise ValueError("%s must not be negative (0 = the common learning rate), got %r" % (name, v))
        out.append(v if v > 0 else float(lr))
    return int(d_steps), b2, out[0], out[1]


def resolve_d_steps(d_steps=None, beta2=None, lr_d=None, lr_g=None, lr=2e-4):
    """check_d_steps over the engines' arguments: None = the environment default (DCGAN_D_STEPS,
    DCGAN_BETA2, DCGAN_LR_D, DCGAN_LR_G), then 1 / ADAM_BETA2 / `lr`. An explicit argument wins."""
    from .options import resolve_group
    return resolve_group("d_steps", (d_steps, beta2, lr_d, lr_g), lr=lr)


def check_d_steps_schedule(d_steps: int, schedule: str, sharded: bool) -> None:
    """d_steps > 1 runs on the single-process step and the default (segmented, all-reduce) DDP step
    only: the sharded update and the "ddp" / "serial" schedules have no D sub-step."""
    if d_steps <= 1:
        return
    if sharded:
        raise ValueError("d_steps > 1 is not supported with DCGAN_DDP_SHARD=1: the D sub-step updates D from "
                         "all-reduced gradients, the sharded update has no sub-step schedule")
    if schedule in ("ddp", "serial"):
        raise ValueError("d_steps > 1 is not supported with the %r schedule: the D sub-step is recorded for the "
                         "single-process (\"fused\") and the default DDP (\"concurrent\") schedules only" % schedule)


# --------------------------------------------------------------------------- learning-rate schedule
LR_KINDS = ("none", "linear", "cosine", "exponential")  # index = the kernels' id (kernels.h LrKind)
LR_MAX_STEPS = 1 << 24  # decay and warm-up lengths: exact as fp32


class LrSchedule(NamedTuple):
    """Factor f(t) of the global step t (its value before the step's increment, TF's global_step)
    that multiplies both networks' Adam rates:

        k = 0 if t <= start else min(t - start, steps);  p = float(k) / float(steps)
        none 1 | linear 1 - (1 - end) p | cosine 1 - (1 - end) (1 - cos(pi p)) / 2 | exponential end^p
        k == 0 -> exactly 1, k == steps -> exactly end;  t < warmup: f *= float(t + 1) / float(warmup)

    (tf polynomial_decay with power 1, cosine_decay with alpha = end, exponential_decay clamped at
    `steps`). The schedule follows the global step: an fp16 step skipped on overflow advances it too."""
    kind: str = "none"
    start: int = 0
    steps: int = 1
    end: float = 1.0
    warmup: int = 0

    @property
    def active(self) -> bool:
        return self.kind != "none" or self.warmup > 0

    def hip_args(self) -> tuple:
        """(lr_kind, lr_start, lr_steps, lr_end, lr_warmup) of the Adam bindings."""
        return (LR_KINDS.index(self.kind), self.start, self.steps, self.end, self.warmup)

    def describe(self) -> str:
        if not self.active:
            return "constant"
        s = "constant" if self.kind == "none" else "%s to %g x over steps %d..%d" % (
            self.kind, self.end, self.start, self.start + self.steps)
        return s + (", linear warm-up over %d steps" % self.warmup if self.warmup else "")


def _lr_int(name, v, lo, hi):
    if isinstance(v, bool) or isinstance(v, float) and not v.is_integer() or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer with %d <= %s <= %d, got %r" % (name, lo, name, hi, v))
    return int(v)


def check_lr_schedule(kind="none", start=0, steps=0, end=0.0, warmup=0, total_steps=None,
                      open_ended=False) -> LrSchedule:
    """Validated LrSchedule; errors name the flag. kind in LR_KINDS, start >= 0, 1 <= steps <= 2^24,
    0 <= end <= 1 (> 0 for exponential), 0 <= warmup <= 2^24. steps = 0 with a decay kind means
    "until the end of training": total_steps - start when `total_steps` is given (an error when
    that is < 1), left at 0 for a later resolution when `open_ended`, else an error. With kind
    "none" start / steps / end are not read."""
    if not isinstance(kind, str) or kind.strip().lower() not in LR_KINDS:
        raise ValueError("lr_decay must be one of %s, got %r" % (LR_KINDS, kind))
    kind = kind.strip().lower()
    warmup = _lr_int("lr_warmup_steps", warmup, 0, LR_MAX_STEPS)
    if kind == "none":
        return LrSchedule("none", 0, 1, 1.0, warmup)
    start = _lr_int("lr_decay_start", start, 0, (1 << 62))
    steps = _lr_int("lr_decay_steps", steps, 0, LR_MAX_STEPS)
    if steps == 0:
        if total_steps is not None:
            steps = int(total_steps) - start
            if not 1 <= steps <= LR_MAX_STEPS:
                raise ValueError("lr_decay_steps=0 decays until the end of training, but %d steps of training minus "
                                 "lr_decay_start=%d leaves %d (need 1 .. 2^24)" % (int(total_steps), start, steps))
        elif not open_ended:
            raise ValueError("lr_decay_steps must be an integer with 1 <= lr_decay_steps <= %d, got 0 (only the "
                             "trainer resolves 0 = until the end of training)" % LR_MAX_STEPS)
    end = float(end)
    if not 0.0 <= end <= 1.0:
        raise ValueError("lr_end must satisfy 0 <= lr_end <= 1, got %r" % (end,))
    if kind == "exponential" and not end > 0.0:
        raise ValueError("lr_end must be > 0 with lr_decay=exponential, got %r" % (end,))
    return LrSchedule(kind, start, steps, end, warmup)


def resolve_lr_schedule(kind=None, start=None, steps=None, end=None, warmup=None, total_steps=None) -> LrSchedule:
    """check_lr_schedule over the engines' arguments: None = the environment default (DCGAN_LR_DECAY,
    DCGAN_LR_DECAY_START, DCGAN_LR_DECAY_STEPS, DCGAN_LR_END, DCGAN_LR_WARMUP), then none / 0 / 0 /
    0.0 / 0. An explicit argument wins. An LrSchedule as `kind` is validated as it is."""
    from .options import resolve_group
    return resolve_group("lr_sched", (kind, start, steps, end, warmup), total_steps=total_steps)


def lr_factor(sched: LrSchedule, t, dtype=torch.float32) -> torch.Tensor:
    """The schedule's factor at global step(s) t (int or int64 tensor), evaluated in `dtype`: fp32
    is the device's arithmetic (`end` rounded to fp32 first), fp64 the closed form."""
    t = torch.as_tensor(t, dtype=torch.int64)
    one = torch.ones(t.shape, dtype=dtype)
    f = one
    if sched.kind != "none":
        k = (t - sched.start).clamp(0, sched.steps)
        p = k.to(dtype) / torch.tensor(float(sched.steps), dtype=dtype)
        end = torch.tensor(sched.end, dtype=dtype)
        if sched.kind == "linear":
            g = 1 - (1 - end) * p
        elif sched.kind == "cosine":
            g = 1 - (1 - end) * (0.5 * (1 - torch.cos(torch.tensor(math.pi, dtype=dtype) * p)))
        else:
            g = torch.pow(end, p)
        f = torch.where(k == 0, one, torch.where(k == sched.steps, end.expand(t.shape), g))
    if sched.warmup > 0:
        w = (t + 1).clamp(max=sched.warmup).to(dtype) / torch.tensor(float(sched.warmup), dtype=dtype)
        f = torch.where(t < sched.warmup, f * w, f)
    return f


# --------------------------------------------------------------------------- instance noise (D's input)
NOISE_MAX_SIGMA = 2.0
NOISE_MAX_STEPS = 1 << 24  # length of the anneal: exact as fp32
NOISE_STREAM = 1           # Philox stream of the noise (z draws from stream 0)
SUBSTEP_SEED_STRIDE = 0x9E3779B97F4A7C15  # seed of D sub-step k = seed + (k + 1) * this, mod 2^64


class InstanceNoise(NamedTuple):
    """D is trained on x + sigma(t) * eps, eps ~ N(0, I), over the stacked [real | fake] input, with
    sigma annealed linearly over the global step t (its value before the step's increment):

        sigma(t) = sigma1 if t >= steps else fma(sigma1 - sigma0, float(t) / float(steps), sigma0)

    in fp32; sigma0 == sigma1 is a constant (steps is not read). Active when either end is > 0."""
    sigma0: float = 0.0
    sigma1: float = 0.0
    steps: int = 1

    @property
    def active(self) -> bool:
        return self.sigma0 > 0.0 or self.sigma1 > 0.0

    def describe(self) -> str:
        if not self.active:
            return "off"
        if self.sigma0 == self.sigma1:
            return "sigma %g" % self.sigma0
        return "sigma %g to %g over %d steps" % (self.sigma0, self.sigma1, self.steps)


def check_instance_noise(sigma0=0.0, sigma1=0.0, steps=0, total_steps=None, open_ended=False) -> InstanceNoise:
    """Validated InstanceNoise; errors name the flag. 0 <= sigma0, sigma1 <= 2, both finite; with
    sigma0 != sigma1, 1 <= steps <= 2^24. steps = 0 then means "until the end of training":
    `total_steps` when given (an error when that is < 1), left at 0 for a later resolution when
    `open_ended`, else an error. With sigma0 == sigma1 steps is not read."""
    out = []
    for name, v in (("instance_noise", sigma0), ("instance_noise_end", sigma1)):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (name, v)) from None
        if not (math.isfinite(v) and 0.0 <= v <= NOISE_MAX_SIGMA):
            raise ValueError("%s must be finite with 0 <= %s <= %g, got %r" % (name, name, NOISE_MAX_SIGMA, v))
        out.append(v)
    s0, s1 = out
    if s0 == s1:
        return InstanceNoise(s0, s1, 1)
    steps = _lr_int("instance_noise_steps", steps, 0, NOISE_MAX_STEPS)
    if steps == 0:
        if total_steps is not None:
            steps = int(total_steps)
            if not 1 <= steps <= NOISE_MAX_STEPS:
                raise ValueError("instance_noise_steps=0 anneals until the end of training, but that is %d steps "
                                 "(need 1 .. 2^24)" % steps)
        elif not open_ended:
            raise ValueError("instance_noise_steps must be an integer with 1 <= instance_noise_steps <= %d, got 0 "
                             "(only the trainer resolves 0 = until the end of training)" % NOISE_MAX_STEPS)
    return InstanceNoise(s0, s1, steps)


def resolve_instance_noise(sigma0=None, sigma1=None, steps=None, total_steps=None) -> InstanceNoise:
    """check_instance_noise over the engines' arguments: None = the environment default
    (DCGAN_INSTANCE_NOISE, DCGAN_INSTANCE_NOISE_END, DCGAN_INSTANCE_NOISE_STEPS), then 0 / 0 / 0. An
    explicit argument wins. An InstanceNoise as `sigma0` is validated as it is."""
    from .options import resolve_group
    return resolve_group("noise", (sigma0, sigma1, steps), total_steps=total_steps)


def noise_sigma(t, sigma0: float, sigma1: float, steps: int, dtype=torch.float32) -> torch.Tensor:
    """sigma(t) of InstanceNoise at global step(s) t (int or int64 tensor): fp32 is the device's
    arithmetic (both ends rounded to fp32, one fused multiply-add), fp64 the closed form."""
    t = torch.as_tensor(t, dtype=torch.int64)
    if dtype == torch.float64:
        s0, s1 = torch.tensor(float(sigma0), dtype=dtype), torch.tensor(float(sigma1), dtype=dtype)
        if float(sigma0) == float(sigma1):
            return s0.expand(t.shape).clone()
        p = t.clamp(0, int(steps)).to(dtype) / float(steps)
        return torch.where(t >= int(steps), s1.expand(t.shape), s0 + (s1 - s0) * p)
    f = torch.float32
    s0, s1 = torch.tensor(float(sigma0), dtype=f), torch.tensor(float(sigma1), dtype=f)
    if float(s0) == float(s1):
        return s0.expand(t.shape).clone()
    p = t.clamp(0, int(steps)).to(f) / torch.tensor(float(steps), dtype=f)
    # fma in fp32: the product of two fp32 numbers is exact in fp64, the sum is rounded once there
    g = ((s1 - s0).double() * p.double() + s0.double()).to(f)
    return torch.where(t >= int(steps), s1.expand(t.shape), g)


def substep_seed(seed: int, sub: Optional[int] = None) -> int:
    """Seed of the Philox streams of D sub-step `sub` (None: the full step's, `seed` itself)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if sub is None:
        return seed
    return (seed + (int(sub) + 1) * SUBSTEP_SEED_STRIDE) & 0xFFFFFFFFFFFFFFFF


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Random123) over numpy arrays: counter [..., 4] and key [..., 2] of 32-bit
    words (broadcast against each other) -> uint32 [..., 4]."""
    import numpy as np
    c = np.asarray(counter).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def philox_words(n: int, seed: int, step: int, stream: int = 0):
    """The kernels' counter layout: element e of a flat buffer draws lane e % 4 of the block at counter
    (lo32(e / 4), hi32(e / 4), lo32(step), hi32(step) ^ stream), key = the 64-bit seed. Returns the
    uint32 [ceil(n / 4), 4] blocks."""
    import numpy as np
    m = (int(n) + 3) // 4
    i4 = np.arange(m, dtype=np.uint64)
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((m, 4), dtype=np.uint64)
    ctr[:, 0] = i4 & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = i4 >> np.uint64(32)
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = ((step >> 32) ^ int(stream)) & 0xFFFFFFFF
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def philox_normal(n: int, seed: int, step: int, stream: int = NOISE_STREAM, dtype=torch.float64) -> torch.Tensor:
    """n standard normals of the Philox stream (seed, step, stream): Box-Muller per pair of lanes.
    Lanes 0, 1 of a block come from its words (c0, c1), lanes 2, 3 from (c2, c3): u0 = ((a >> 8) + 1)
    2^-24 in (0, 1], u1 = (b >> 8) 2^-24 in [0, 1), r = sqrt(-2 ln u0), even lane r cos(2 pi u1), odd
    lane r sin(2 pi u1). dtype float64: the closed form; float32: every operation in fp32, the angle
    float32(2 pi) * u1."""
    import numpy as np
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("philox_normal: dtype must be torch.float64 or torch.float32")
    ft = np.float64 if dtype == torch.float64 else np.float32
    w = philox_words(n, seed, step, stream).reshape(-1, 2)  # [pairs, (a, b)]
    u0 = ((w[:, 0] >> np.uint32(8)).astype(ft) + ft(1)) * ft(2.0 ** -24)
    u1 = (w[:, 1] >> np.uint32(8)).astype(ft) * ft(2.0 ** -24)
    r = np.sqrt(ft(-2) * np.log(u0))
    ang = ft(2 * math.pi) * u1
    out = np.stack([r * np.cos(ang), r * np.sin(ang)], -1).astype(ft).reshape(-1)[:int(n)]
    return torch.from_numpy(np.ascontiguousarray(out))


def instance_noise(shape, noise: InstanceNoise, seed: int, step: int, dtype=torch.float32) -> torch.Tensor:
    """The additive sigma(step) * eps of InstanceNoise over a [2B, ...] input of `shape` (fp64 normals,
    fp32 sigma), as the kernel lays it out: eps over the flat buffer, stream NOISE_STREAM."""
    n = 1
    for d in shape:
        n *= int(d)
    sig = float(noise_sigma(int(step), noise.sigma0, noise.sigma1, noise.steps))
    eps = philox_normal(n, seed, int(step), NOISE_STREAM)
    return (eps * sig).to(dtype).reshape(tuple(shape))


# --------------------------------------------------------------------------- DiffAugment (D's input)
AUG_STREAM = 2  # Philox stream of the augmentation draws (z: 0, instance noise: 1)
AUG_POLICIES = ("translation", "cutout")  # bit i of the kernels' policy mask (kernels.h AugPolicy)


class DAugment(NamedTuple):
    """Differentiable augmentation of what D sees (Zhao et al. 2020), reals and fakes alike, G's
    gradient passing through its transpose. Two geometric policies, as published for CIFAR-10:
    translation by up to 1/8 of the image (zero fill) and a cutout of half the image's side."""
    translation: bool = False
    cutout: bool = False

    @property
    def active(self) -> bool:
        return self.translation or self.cutout

    @property
    def mask(self) -> int:
        """The kernels' policy bitmask."""
        return int(self.translation) | int(self.cutout) << 1

    def describe(self) -> str:
        return ",".join(n for n, on in zip(AUG_POLICIES, self) if on) or "off"


def _check_policy_list(option: str, cls, names, spec):
    """The policy tuple `cls` (one bool per name of `names`) from a comma-separated list, any subset in
    any order; "", None and "none" mean off. Anything else is a ValueError naming the offending token."""
    if isinstance(spec, cls):
        return cls(*(bool(v) for v in spec))
    if spec is None:
        spec = ""
    if not isinstance(spec, str):
        raise ValueError("%s must be a comma-separated list of %s, got %r" % (option, names, spec))
    toks = [t.strip().lower() for t in spec.split(",")]
    toks = [t for t in toks if t]
    if toks == ["none"]:
        toks = []
    for t in toks:
        if t not in names:
            raise ValueError("%s: unknown policy %r (known: %s, or none)" % (option, t, ", ".join(names)))
    return cls(*(n in toks for n in names))


def check_d_augment(spec="") -> DAugment:
    """Validated DAugment from a comma-separated policy list: "", "none", "translation", "cutout" or
    both in any order. Anything else is a ValueError naming the offending token."""
    return _check_policy_list("d_augment", DAugment, AUG_POLICIES, spec)


def resolve_d_augment(spec=None) -> DAugment:
    """check_d_augment over the engines' argument: None = the environment default DCGAN_D_AUGMENT,
    then off. An explicit argument wins."""
    from .options import resolve_group
    return resolve_group("aug", (spec,))


def augment_params(n: int, S: int, seed: int, step: int) -> torch.Tensor:
    """int64 [n, 4] = (ty, tx, oy, ox) of samples 0..n-1 of an S x S image: sample i takes the words
    w0..w3 of the Philox block at counter (i, step, AUG_STREAM) under `seed`. With s = (S + 4) // 8,
    k = (S + 1) // 2, r = S + (1 - k % 2) and mulhi(w, m) = (w * m) >> 32: ty, tx = mulhi(w0 | w1,
    2s + 1) - s in [-s, s]; oy, ox = mulhi(w2 | w3, r) in [0, r). All four are always drawn."""
    import numpy as np
    S = int(S)
    w = philox_words(4 * int(n), seed, step, AUG_STREAM).astype(np.uint64)[:int(n)]
    s, k = (S + 4) // 8, (S + 1) // 2
    r = S + (1 - k % 2)
    out = np.empty((int(n), 4), dtype=np.int64)
    sh = np.uint64(32)
    out[:, 0] = ((w[:, 0] * np.uint64(2 * s + 1)) >> sh).astype(np.int64) - s
    out[:, 1] = ((w[:, 1] * np.uint64(2 * s + 1)) >> sh).astype(np.int64) - s
    out[:, 2] = ((w[:, 2] * np.uint64(r)) >> sh).astype(np.int64)
    out[:, 3] = ((w[:, 3] * np.uint64(r)) >> sh).astype(np.int64)
    return torch.from_numpy(out)


def _gate_rows(gates, N: int, mask: int, device) -> torch.Tensor:
    """int64 [N]: the effective policy of each sample, `mask` & its recorded gate mask."""
    g = torch.as_tensor(gates).to(device=device, dtype=torch.int64).reshape(-1)
    if g.numel() != N:
        raise ValueError("gates must hold one mask per sample (%d), got %d" % (N, g.numel()))
    return g & int(mask)


def _augment_gather(x: torch.Tensor, params: torch.Tensor, aug: DAugment, transpose: bool, gates=None) -> torch.Tensor:
    if x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise ValueError("augment: x must be [N, S, S, C], got %s" % (tuple(x.shape),))
    N, S = x.shape[0], x.shape[1]
    p = torch.as_tensor(params, dtype=torch.int64).to(x.device)
    if tuple(p.shape) != (N, 4):
        raise ValueError("augment: params must be [N, 4] = (ty, tx, oy, ox), got %s" % (tuple(p.shape),))
    zero = torch.zeros((), dtype=torch.int64, device=x.device)
    ty, tx = (p[:, 0], p[:, 1]) if aug.translation else (zero.expand(N), zero.expand(N))
    eff = None if gates is None else _gate_rows(gates, N, aug.mask, x.device)
    if eff is not None:  # a sample with translation gated off: ty = tx = 0, as under the smaller policy
        on = (eff & 1) != 0
        ty, tx = torch.where(on, ty, zero), torch.where(on, tx, zero)
    if transpose:
        ty, tx = -ty, -tx
    a = torch.arange(S, device=x.device)
    si, sj = a[None, :] + ty[:, None], a[None, :] + tx[:, None]  # source row / column of each output one
    keep = ((si >= 0) & (si < S))[:, :, None] & ((sj >= 0) & (sj < S))[:, None, :]
    if aug.cutout:
        k = (S + 1) // 2
        by, bx = (si, sj) if transpose else (a[None, :].expand(N, S), a[None, :].expand(N, S))
        y0, x0 = (p[:, 2] - k // 2)[:, None], (p[:, 3] - k // 2)[:, None]
        box = ((by >= y0) & (by < y0 + k))[:, :, None] & ((bx >= x0) & (bx < x0 + k))[:, None, :]
        if eff is not None:
            box = box & ((eff & 2) != 0)[:, None, None]
        keep = keep & ~box
    g = x[torch.arange(N, device=x.device)[:, None, None], si.clamp(0, S - 1)[:, :, None],
          sj.clamp(0, S - 1)[:, None, :]]
    return torch.where(keep[..., None], g, torch.zeros((), dtype=x.dtype, device=x.device))


def augment(x: torch.Tensor, params: torch.Tensor, aug: DAugment, gates=None) -> torch.Tensor:
    """The augmentation of x [N, S, S, C] (NHWC) under params [N, 4] = (ty, tx, oy, ox), k = (S + 1) // 2:

        y[n,i,j,c] = +0                     if cutout and oy - k//2 <= i < oy - k//2 + k (and j, ox alike)
                   = x[n, i+ty, j+tx, c]    if that pixel is inside the image (translation off: ty = tx = 0)
                   = +0                     otherwise

    the published rand_translation followed by rand_cutout for those draws. A gather and a
    torch.where: values pass through bit for bit, every zero is +0, and autograd gives the backward.
    gates: int [N], the recorded gate masks of adaptive augmentation (``gate_masks``): sample n is
    augmented under the policy ``aug.mask & gates[n]``. None: every sample under ``aug``."""
    return _augment_gather(x, params, aug, False, gates)


def augment_transpose(g: torch.Tensor, params: torch.Tensor, aug: DAugment, gates=None) -> torch.Tensor:
    """The transpose of ``augment`` as a gather of its own: gx[n,p,q,c] = g[n, p-ty, q-tx, c] if that
    index is inside the image and outside the box, else +0. gates: as ``augment``."""
    return _augment_gather(g, params, aug, True, gates)


# --------------------------------------------------------------------------- DiffAugment's color policy
COLOR_STREAM = 3  # Philox stream of the color draws (z: 0, instance noise: 1, translation / cutout: 2)
COLOR_POLICIES = ("brightness", "saturation", "contrast")  # bit i of the kernels' mask (kernels.h ColorPolicy)


class DColor(NamedTuple):
    """The color policy of DiffAugment (Zhao et al. 2020) on what D sees, reals and fakes alike, ahead
    of translation / cutout: per sample a brightness shift b in [-0.5, 0.5), a saturation scale s in
    [0, 2) about the pixel's channel mean and a contrast scale c in [0.5, 1.5] about the image's
    mean. Each is switched on its own (the paper's `color` is all three)."""
    brightness: bool = False
    saturation: bool = False
    contrast: bool = False

    @property
    def active(self) -> bool:
        return self.brightness or self.saturation or self.contrast

    @property
    def mask(self) -> int:
        """The kernels' policy bitmask."""
        return int(self.brightness) | int(self.saturation) << 1 | int(self.contrast) << 2

    def describe(self) -> str:
        return ",".join(n for n, on in zip(COLOR_POLICIES, self) if on) or "off"


def check_d_color(spec="") -> DColor:
    """Validated DColor from a comma-separated list of brightness, saturation, contrast (any subset, any
    order); "" and "none" mean off. Anything else is a ValueError naming the offending token."""
    return _check_policy_list("d_color_augment", DColor, COLOR_POLICIES, spec)


def resolve_d_color(spec=None) -> DColor:
    """check_d_color over the engines' argument: None = the environment default
    DCGAN_D_COLOR_AUGMENT, then off. An explicit argument wins."""
    from .options import resolve_group
    return resolve_group("color", (spec,))


def color_params(n: int, seed: int, step: int) -> torch.Tensor:
    """float32 [n, 3] = (b, s, c) of samples 0..n-1: sample i takes the words w0..w2 of the Philox block
    at counter (i, step, COLOR_STREAM) under `seed`; u_k = float(w_k >> 8) * 2^-24 and, in fp32,
    b = u0 - 0.5, s = 2 * u1, c = u2 + 0.5. All three are always drawn."""
    import numpy as np
    w = philox_words(4 * int(n), seed, step, COLOR_STREAM)[:int(n)]
    u = (w[:, :3] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    out = np.stack([u[:, 0] - np.float32(0.5), np.float32(2) * u[:, 1], u[:, 2] + np.float32(0.5)], -1)
    return torch.from_numpy(np.ascontiguousarray(out.astype(np.float32)))


def _color_setup(x: torch.Tensor, params) -> Tuple[torch.Tensor, torch.Tensor, torch.dtype]:
    if x.dim() != 4:
        raise ValueError("color_augment: x must be [N, S, S, C], got %s" % (tuple(x.shape),))
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    p = torch.as_tensor(params).to(device=x.device, dtype=ct)
    if p.dim() != 2 or p.shape[0] != x.shape[0] or p.shape[1] not in (3, 4):
        raise ValueError("color_augment: params must be [N, 3] = (b, s, c) or [N, 4] = (b, s, c, Mx), got %s"
                         % (tuple(p.shape),))
    return x.to(ct), p, ct


def _count(v: torch.Tensor, n: int) -> torch.Tensor:
    # a tensor divisor: a correctly rounded division on every device (a Python number may turn into a
    # multiplication by its reciprocal)
    return torch.full((), float(n), dtype=v.dtype, device=v.device)


def _channel_mean(v: torch.Tensor) -> torch.Tensor:
    m = v[..., 0]
    for ch in range(1, v.shape[-1]):  # in channel order
        m = m + v[..., ch]
    return (m / _count(v, v.shape[-1]))[..., None]


def _image_mean(v: torch.Tensor) -> torch.Tensor:
    n = v.shape[1] * v.shape[2] * v.shape[3]
    return v.reshape(v.shape[0], -1).sum(1) / _count(v, n)


def color_mean(x: torch.Tensor) -> torch.Tensor:
    """Mx [N] of the definition below: the sum of an image's elements in the compute type, divided by
    their count (the kernel records its own in column 3 of its params; the two differ by the order of
    the sum)."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    return _image_mean(x.to(ct))


def _color_gated(x, params, color: DColor, eff: torch.Tensor) -> torch.Tensor:
    """``color_augment`` with per-sample effective policies eff [N]: each stage computed as below and
    kept only on the samples whose bit is set (a select: the others pass through bit for bit)."""
    v, p, ct = _color_setup(x, params)
    col = lambda i: p[:, i].reshape(-1, 1, 1, 1)  # noqa: E731
    bit = lambda i: ((eff >> i) & 1).ne(0).reshape(-1, 1, 1, 1)  # noqa: E731
    bri, sat, con = bit(0), bit(1), bit(2)
    if color.brightness:
        v = torch.where(bri, v + col(0), v)
    if color.saturation:
        m = _channel_mean(v)
        v = torch.where(sat, col(1) * (v - m) + m, v)
    if color.contrast:
        M = (p[:, 3] if p.shape[1] == 4 else _image_mean(x.to(ct))).reshape(-1, 1, 1, 1)
        if color.brightness:
            M = torch.where(bri, M + col(0), M)
        v = torch.where(con, col(2) * (v - M) + M, v)
    return v.to(x.dtype)


def color_augment(x: torch.Tensor, params: torch.Tensor, color: DColor, gates=None) -> torch.Tensor:
    """The color policy over x [N, S, S, C] (NHWC) under params [N, 3] = (b, s, c), every operation a
    separately rounded fp32 one (fp64 for an fp64 x), the stages that `color` switches off skipped:

        brightness : v = v + b
        saturation : m = (v_0 + .. + v_{C-1}) / C per pixel, in channel order;  v = s * (v - m) + m
        contrast   : M = Mx + b if brightness else Mx, Mx = sum(x[n]) / (S*S*C);  v = c * (v - M) + M

    M is the published mean of the image after brightness and saturation, in exact arithmetic
    (saturation keeps a pixel's channel mean): one reduction over the input serves. A fourth column of
    params gives Mx (what the kernel recorded); else it is ``color_mean(x)``. Differentiable.
    gates: int [N], the recorded gate masks of adaptive augmentation (``gate_masks``): sample n is
    processed under the policy ``color.mask & gates[n]`` (brightness gated off: M = Mx; contrast gated
    off: Mx is not read). None: every sample under ``color``."""
    if gates is not None:
        return _color_gated(x, params, color, _gate_rows(gates, x.shape[0], color.mask, x.device))
    v, p, ct = _color_setup(x, params)
    col = lambda i: p[:, i].reshape(-1, 1, 1, 1)  # noqa: E731
    if color.brightness:
        v = v + col(0)
    if color.saturation:
        m = _channel_mean(v)
        v = col(1) * (v - m) + m
    if color.contrast:
        M = (p[:, 3] if p.shape[1] == 4 else _image_mean(x.to(ct))).reshape(-1, 1, 1, 1)
        if color.brightness:
            M = M + col(0)
        v = col(2) * (v - M) + M
    return v.to(x.dtype)


def color_augment_transpose(g: torch.Tensor, params: torch.Tensor, color: DColor, mean=None, gates=None) -> torch.Tensor:
    """The transpose of ``color_augment``'s linear part over g = dL/dy: each stage is a symmetric map,
    so it is the same stage functions in reverse order on the gradient's own mean (brightness is the
    identity):

        contrast   : Gm = sum(g[n]) / (S*S*C);  v = c * (v - Gm) + Gm
        saturation : m over the channels of those values;  v = s * (v - m) + m

    mean: Gm [N] given instead of summed here. gates: as ``color_augment``."""
    v, p, ct = _color_setup(g, params)
    col = lambda i: p[:, i].reshape(-1, 1, 1, 1)  # noqa: E731
    if gates is not None:
        eff = _gate_rows(gates, g.shape[0], color.mask, g.device)
        sat, con = (((eff >> i) & 1).ne(0).reshape(-1, 1, 1, 1) for i in (1, 2))
        if color.contrast:
            Gm = (_image_mean(v) if mean is None else torch.as_tensor(mean).to(device=v.device, dtype=ct)).reshape(-1, 1, 1, 1)
            v = torch.where(con, col(2) * (v - Gm) + Gm, v)
        if color.saturation:
            m = _channel_mean(v)
            v = torch.where(sat, col(1) * (v - m) + m, v)
        return v.to(g.dtype)
    if color.contrast:
        Gm = (_image_mean(v) if mean is None else torch.as_tensor(mean).to(device=v.device, dtype=ct)).reshape(-1, 1, 1, 1)
        v = col(2) * (v - Gm) + Gm
    if color.saturation:
        m = _channel_mean(v)
        v = col(1) * (v - m) + m
    return v.to(g.dtype)


# --------------------------------------------------------------------------- adaptive augmentation (ADA)
AUG_GATE_STREAM = 4    # Philox stream of the gates of translation (w0) and cutout (w1)
COLOR_GATE_STREAM = 5  # ... and of brightness (w0), saturation (w1), contrast (w2)
ADA_ONE = 1 << 24      # p24 of p = 1
ADA_MAX_INTERVAL = 1 << 16
ADA_STATE_WORDS = 8    # int32 (p24, acc, cnt, r_acc, windows, 0, 0, 0)
ADA_KEYS = ("p24", "acc", "cnt", "r_acc", "windows")  # the checkpoint's ada/<key>


class DAda(NamedTuple):
    """Adaptive discriminator augmentation (Karras et al. 2020): every selected policy of DAugment /
    DColor is applied to a sample with probability p, and p is steered by r_t = E[sign(D(real))] over
    windows of `interval` steps: up by a fixed step while r_t is above `target`, down while below,
    sized so that p can cross [0, 1] in `kimg` thousand real images. p is kept as the integer p24 = p *
    2^24, so the gate, the controller and a resume are exact. target = 0: a fixed p (p = 1: off, no
    gate at all). `p` here is the resolved start value."""
    p: float = 1.0
    target: float = 0.0
    interval: int = 4
    kimg: float = 500.0

    @property
    def adaptive(self) -> bool:
        return self.target > 0.0

    @property
    def active(self) -> bool:
        """Gated kernels and a device state are recorded."""
        return self.adaptive or self.p < 1.0

    def describe(self) -> str:
        if not self.active:
            return "off"
        if not self.adaptive:
            return "fixed p = %g" % self.p
        return "adaptive p from %g, target r_t = %g, every %d steps, %g kimg from 0 to 1" % (
            self.p, self.target, self.interval, self.kimg)


def check_ada(p=-1.0, target=0.0, interval=4, kimg=500.0, augmented: Optional[bool] = None,
              batch_size: Optional[int] = None) -> DAda:
    """Validated DAda; errors name the flag. p = -1 resolves to 1 without a target (off) and to 0 with
    one (the published start); else 0 <= p <= 1. 0 <= target < 1 (0 = no controller), interval in 1 ..
    2^16, kimg > 0 and finite; batch_size (when given) * interval < 2^31. augmented=False: neither
    d_augment nor d_color_augment selects a policy -- an error when a gate or the controller is on."""
    if isinstance(p, DAda):
        p, target, interval, kimg = p
    try:
        p, target, kimg = float(p), float(target), float(kimg)
    except (TypeError, ValueError):
        raise ValueError("d_augment_p, ada_target and ada_kimg must be numbers, got %r, %r, %r"
                         % (p, target, kimg)) from None
    if not (math.isfinite(target) and 0.0 <= target < 1.0):
        raise ValueError("ada_target must satisfy 0 < ada_target < 1 (0 = off), got %r" % (target,))
    if p == -1.0:
        p = 0.0 if target > 0.0 else 1.0
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError("d_augment_p must satisfy 0 <= d_augment_p <= 1 (or -1 = the default), got %r" % (p,))
    interval = _lr_int("ada_interval", interval, 1, ADA_MAX_INTERVAL)
    if not (math.isfinite(kimg) and kimg > 0.0):
        raise ValueError("ada_kimg must be finite and > 0, got %r" % (kimg,))
    ada = DAda(p, target, interval, kimg)
    if batch_size is not None and int(batch_size) * interval >= 1 << 31:
        raise ValueError("ada_interval: batch_size * ada_interval must stay below 2^31, got %d * %d"
                         % (int(batch_size), interval))
    if ada.active and augmented is False:
        raise ValueError("d_augment_p / ada_target need a policy to gate: set d_augment and / or d_color_augment")
    return ada


def resolve_ada(p=None, target=None, interval=None, kimg=None, augmented: Optional[bool] = None,
                batch_size: Optional[int] = None) -> DAda:
    """check_ada over the engines' arguments: None = the environment default (DCGAN_D_AUGMENT_P,
    DCGAN_ADA_TARGET, DCGAN_ADA_INTERVAL, DCGAN_ADA_KIMG), then -1 / 0 / 4 / 500. An explicit argument
    wins. A DAda as `p` is validated as it is."""
    from .options import resolve_group
    return resolve_group("ada", (p, target, interval, kimg), augmented=augmented, batch_size=batch_size)


def ada_p24(p: float) -> int:
    """round_half_even(p * 2^24) in [0, 2^24]."""
    p = float(p)
    if not (0.0 <= p <= 1.0):
        raise ValueError("ada_p24: p must satisfy 0 <= p <= 1, got %r" % (p,))
    return int(round(p * ADA_ONE))


def ada_delta24(world: int, B: int, interval: int, kimg: float) -> int:
    """The controller's step of p24 per window: clamp(round_half_even(2^24 * W * B * interval / (1000
    * kimg)), 1, 2^24) -- W * B * interval real images per window out of 1000 * kimg for the whole range."""
    d = int(round(ADA_ONE * float(int(world) * int(B) * int(interval)) / (1000.0 * float(kimg))))
    return max(1, min(ADA_ONE, d))


def ada_target_n(target: float, B: int, interval: int) -> int:
    """Tn = round_half_even(target * B * interval): the window's sum of signs at r_t = target."""
    return int(round(float(target) * int(B) * int(interval)))


def ada_threshold(kind: str = "bce", label_smooth: float = 0.0) -> float:
    """The logit at which D calls a sample real, as the fp32 the kernel takes: 0 for bce and hinge,
    (1 - label_smooth) / 2 for lsgan (halfway between its targets 0 and 1 - label_smooth)."""
    import numpy as np
    kind, label_smooth = check_gan_loss(kind, label_smooth)
    return float(np.float32((1.0 - label_smooth) / 2.0)) if kind == "lsgan" else 0.0


def ada_state(p24: int = 0) -> list:
    """A fresh controller state (p24, acc, cnt, r_acc, windows, 0, 0, 0)."""
    return [int(p24)] + [0] * (ADA_STATE_WORDS - 1)


def gate_masks(n: int, seed: int, step: int, stream: int, p24: int, policy_mask: int) -> torch.Tensor:
    """int32 [n]: the gate mask each gated kernel records for samples 0..n-1. Sample i draws the Philox
    block at counter (i, step, stream) under `seed`; policy bit k is on iff (w_k >> 8) < p24, so p24 =
    2^24 gates nothing off and p24 = 0 everything. Bits outside `policy_mask` are cleared: the mask is
    the effective policy of the sample."""
    import numpy as np
    w = philox_words(4 * int(n), seed, step, stream)[:int(n)].astype(np.int64) >> 8
    m = np.zeros(int(n), dtype=np.int64)
    for k in range(3):
        m |= (w[:, k] < int(p24)).astype(np.int64) << k
    return torch.from_numpy((m & int(policy_mask)).astype(np.int32))


def ada_sign_sum(real_logits, thr: float = 0.0) -> int:
    """a = sum_i ((x_i > thr) - (x_i < thr)) over the fp32 logits, thr as fp32; NaN counts 0."""
    import numpy as np
    x = torch.as_tensor(real_logits).detach().to(torch.float32).cpu().numpy().reshape(-1)
    t = np.float32(thr)
    return int((x > t).sum()) - int((x < t).sum())


def ada_update(state, real_logits, thr: float, target_n: int, delta24: int, interval: int) -> list:
    """One controller step on Python ints: `state` = (p24, acc, cnt, r_acc, windows, ...) -> the new
    state. The kernel (misc.hip ada_update_kernel) is this, word for word."""
    s = [int(v) for v in state]
    s += [0] * (ADA_STATE_WORDS - len(s))
    p24, acc, cnt, r_acc, windows = s[:5]
    acc += ada_sign_sum(real_logits, thr)
    cnt += 1
    if cnt == int(interval):
        d = int(acc > int(target_n)) - int(acc < int(target_n))
        p24 = max(0, min(ADA_ONE, p24 + d * int(delta24)))
        r_acc, windows, acc, cnt = acc, windows + 1, 0, 0
    return [p24, acc, cnt, r_acc, windows] + s[5:ADA_STATE_WORDS]


# --------------------------------------------------------------------------- top-k generator updates
TOPK_MAX_B = 4096          # the kernel stages one batch of keys in LDS
TOPK_MAX_STEPS = 1 << 24   # length of the anneal of k


class GTopK(NamedTuple):
    """Top-k training of G (Sinha et al., NeurIPS 2020): in G's update only, the B - k fakes D scores
    lowest are dropped. k is annealed linearly, in integers, over the global step t (its value before
    the step's increment) from B down to kmin = ceil(B * nu):

        k(t) = B - ((B - kmin) * min(t, steps)) // steps

    nu = 1 is off. D's losses, its gradients and the logged g_loss are those of all B samples."""
    nu: float = 1.0
    steps: int = 1

    @property
    def active(self) -> bool:
        return self.nu < 1.0

    def describe(self) -> str:
        if not self.active:
            return "off"
        return "k from B to ceil(%g B) over %d steps" % (self.nu, self.steps)


def check_g_topk(nu=1.0, steps=0, total_steps=None, open_ended=False) -> GTopK:
    """Validated GTopK; errors name the flag. 0 < nu <= 1 and finite; when active (nu < 1), 1 <= steps
    <= 2^24. steps = 0 then means "until the end of training": `total_steps` when given (an error when
    that is < 1), left at 0 for a later resolution when `open_ended`, else an error. With nu = 1 steps
    is not read."""
    try:
        nu = float(nu)
    except (TypeError, ValueError):
        raise ValueError("g_topk must be a number, got %r" % (nu,)) from None
    if not (math.isfinite(nu) and 0.0 < nu <= 1.0):
        raise ValueError("g_topk must be finite with 0 < g_topk <= 1, got %r" % (nu,))
    if nu == 1.0:
        return GTopK(1.0, 1)
    steps = _lr_int("g_topk_steps", steps, 0, TOPK_MAX_STEPS)
    if steps == 0:
        if total_steps is not None:
            steps = int(total_steps)
            if not 1 <= steps <= TOPK_MAX_STEPS:
                raise ValueError("g_topk_steps=0 anneals until the end of training, but that is %d steps "
                                 "(need 1 .. 2^24)" % steps)
        elif not open_ended:
            raise ValueError("g_topk_steps must be an integer with 1 <= g_topk_steps <= %d, got 0 "
                             "(only the trainer resolves 0 = until the end of training)" % TOPK_MAX_STEPS)
    return GTopK(nu, steps)


def resolve_g_topk(nu=None, steps=None, total_steps=None) -> GTopK:
    """check_g_topk over the engines' arguments: None = the environment default (DCGAN_G_TOPK,
    DCGAN_G_TOPK_STEPS), then 1 / 0. An explicit argument wins. A GTopK as `nu` is validated as it is."""
    from .options import resolve_group
    return resolve_group("topk", (nu, steps), total_steps=total_steps)


def topk_kmin(B: int, nu: float) -> int:
    """The final k: max(1, min(B, ceil(B * nu - 1e-9))) in Python floats (the kernel takes it as a
    launch constant; the 1e-9 keeps B * nu = an integer + rounding noise at that integer)."""
    B = int(B)
    if B < 1:
        raise ValueError("topk_kmin: B must be >= 1, got %r" % (B,))
    return max(1, min(B, int(math.ceil(B * float(nu) - 1e-9))))


def topk_k(t, B: int, kmin: int, steps: int) -> int:
    """k(t) = B - ((B - kmin) * min(t, steps)) // steps: B at t = 0, kmin from t = steps on."""
    B, kmin, steps = int(B), int(kmin), int(steps)
    if not (1 <= kmin <= B and steps >= 1):
        raise ValueError("topk_k: need 1 <= kmin <= B and steps >= 1, got B=%d kmin=%d steps=%d" % (B, kmin, steps))
    t = min(max(int(t), 0), steps)
    return B - ((B - kmin) * t) // steps


def topk_keys(x_fake: torch.Tensor) -> torch.Tensor:
    """The kernel's sort key of each fp32 logit as int64 in [0, 2^32): monotone in x, -0 below +0,
    NaNs ordered by their bits (positive ones above +inf, negative ones below -inf)."""
    bits = x_fake.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)


def topk_rank(x_fake: torch.Tensor) -> torch.Tensor:
    """rank(i) = #{j : key_j > key_i} + #{j < i : key_j == key_i}: a permutation of 0..B-1 (int64)."""
    key = topk_keys(x_fake.reshape(-1))
    order = torch.sort(-key, stable=True).indices  # descending keys, the lower index first among ties
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), dtype=order.dtype, device=order.device)
    return rank


def topk_select(x_fake: torch.Tensor, k: int) -> torch.Tensor:
    """bool [B]: the samples with rank < k -- exactly k of them, whatever the input."""
    B = x_fake.numel()
    if not 1 <= int(k) <= B:
        raise ValueError("topk_select: need 1 <= k <= B, got k=%r, B=%d" % (k, B))
    return topk_rank(x_fake) < int(k)


def topk_threshold(x_fake: torch.Tensor, k: int) -> torch.Tensor:
    """The logit of the sample with rank k - 1 (the lowest one selected), bits untouched."""
    return x_fake.reshape(-1)[topk_rank(x_fake) == int(k) - 1][0]


def topk_seed(dl_g: torch.Tensor, sel: torch.Tensor, B: int, k: int) -> torch.Tensor:
    """G's seed under top-k: dl_g[i] * (float32(B) / float32(k)) on the selected rows (one fp32 divide,
    one fp32 multiply), +0 elsewhere. dl_g = d g_loss / d logit_fake of the all-sample mean, so the
    result is the gradient of the mean over the selected k."""
    scale = torch.tensor(float(B), dtype=torch.float32) / torch.tensor(float(k), dtype=torch.float32)
    g = dl_g.detach().to(torch.float32)
    return torch.where(sel.to(torch.bool), g * scale.to(g.device), torch.zeros_like(g))


def topk_g_term(x_fake: torch.Tensor, kind: str = "bce") -> torch.Tensor:
    """G's per-sample loss: bce (target 1, never smoothed), lsgan 0.5 (x - 1)^2, hinge -x."""
    if kind not in GAN_LOSSES:
        raise ValueError("gan_loss must be one of %s, got %r" % ("|".join(GAN_LOSSES), kind))
    if kind == "bce":
        return sigmoid_cross_entropy_with_logits(x_fake, torch.ones_like(x_fake))
    if kind == "lsgan":
        return 0.5 * (x_fake - 1.0).pow(2)
    return -x_fake


def topk_g_loss(x_fake: torch.Tensor, sel: torch.Tensor, kind: str = "bce") -> torch.Tensor:
    """g_loss_topk = (1 / k) * the sum of G's per-sample loss over the selected (x's dtype: fp32 or
    fp64); differentiable in x."""
    sel = sel.to(torch.bool)
    return topk_g_term(x_fake[sel], kind).sum() / int(sel.sum())


def zero_fraction(x: torch.Tensor) -> torch.Tensor:
    """tf.nn.zero_fraction (sparsity summary, distriubted_model.py:80)."""
    return (x == 0).float().mean()


def ema_decay_t(decay: float, t: int) -> float:
    """Effective decay of tf.train.ExponentialMovingAverage(decay, num_updates=t), in fp32:
    min(decay, (1 + t) / (10 + t)); t = the global step after this step's increment."""
    f = torch.float32
    d = torch.minimum(torch.tensor(float(decay), dtype=f),
                      (1 + torch.tensor(float(t), dtype=f)) / (10 + torch.tensor(float(t), dtype=f)))
    return float(d)


def ema_update_(s: torch.Tensor, w: torch.Tensor, decay: float, t: int) -> torch.Tensor:
    """TF assign_moving_average (in place, fp32): s -= (1 - d_t) * (s - w)."""
    one_minus = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(ema_decay_t(decay, t), dtype=torch.float32))
    s.sub_((s - w.to(s.dtype)) * one_minus)
    return s


def check_ema_decay(decay) -> float:
    """Validated weight-EMA decay: 0 <= decay < 1 (0 = no moving average is kept)."""
    d = float(decay)
    if not 0.0 <= d < 1.0:
        raise ValueError("g_ema_decay must satisfy 0 <= decay < 1, got %r" % (decay,))
    return d


# --------------------------------------------------------------------------- spectral norm (D)
SN_EPS = 1e-12


def sn_power(W2d: torch.Tensor, u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One power-iteration step on W2d [K, Cout] from u [Cout]: t = W u, v = t / max(|t|, eps),
    s = W^T v, sigma = max(|s|, eps), u' = s / sigma. Returns (u', v, sigma); none of them
    carries a gradient."""
    with torch.no_grad():
        t = W2d @ u
        v = t / t.norm().clamp_min(SN_EPS)
        s = W2d.t() @ v
        sigma = s.norm().clamp_min(SN_EPS)
        return s / sigma, v, sigma


def spectral_normalize(W2d: torch.Tensor, u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """W / sigma with sigma = v^T W u and u, v constants (differentiable in W: autograd of this
    expression is the oracle of the projected gradient)."""
    sigma = (v.detach() @ W2d @ u.detach()).clamp_min(SN_EPS)
    return W2d / sigma


def sn_project(G: torch.Tensor, W2d: torch.Tensor, u: torch.Tensor, v: torch.Tensor, sigma) -> torch.Tensor:
    """dL/dW from G = dL/d(W / sigma): (G - <G, W / sigma> v u^T) / sigma, <G, W / sigma> taken as
    <G, W> / sigma."""
    sigma = torch.as_tensor(sigma, dtype=G.dtype).reshape(())
    d = (G * W2d).sum() / sigma
    return (G - d * torch.outer(v, u)) / sigma


def sn_init_u(shapes: Sequence[Tuple[str, int, int]], seed: int) -> "Dict[str, torch.Tensor]":
    """Fresh u vectors: randn from torch.Generator().manual_seed(seed) on the CPU, one draw per
    weight in the order given ((name, K, Cout), d_variables() order), each normalised."""
    gen = torch.Generator().manual_seed(int(seed))
    out = {}
    for name, _, cout in shapes:
        u = torch.randn(cout, generator=gen)
        out[name] = u / u.norm().clamp_min(SN_EPS)
    return out


def check_spectral_norm(flag) -> bool:
    """Validated d_spectral_norm switch: a bool, 0 / 1, or one of their usual spellings."""
    if isinstance(flag, str):
        s = flag.strip().lower()
        if s in ("1", "true", "yes", "on"):
            return True
        if s in ("", "0", "false", "no", "off"):
            return False
        raise ValueError("d_spectral_norm must be a boolean, got %r" % (flag,))
    if isinstance(flag, bool) or (isinstance(flag, int) and flag in (0, 1)):
        return bool(flag)
    raise ValueError("d_spectral_norm must be a boolean, got %r" % (flag,))

