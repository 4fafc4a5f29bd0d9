"""The training options of a step, in one table: how each is spelled as an engine keyword, a
trainer flag and an environment variable, its default, and the ``ops.reference.check_*`` function
that validates its group. The flag parser, the trainer, both engines, ``ReferenceStep`` and the
benchmarks read this table; none of them lists the options again.

A value is taken from, in this order: the explicit keyword, the environment variable (read when
``resolve`` is called; set but empty counts as unset), the default.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, NamedTuple, Optional, Tuple

from . import reference as R

_UNSET = object()  # a keyword that was not given (None is a value: "the environment's default")


class Group(NamedTuple):
    fields: Tuple[str, ...]            # the StepOptions fields that `check`'s result fills
    keywords: Tuple[str, ...]          # engine keywords, in `check`'s argument order
    env: Tuple[str, ...]               # their environment variables
    conv: Tuple[Callable, ...]         # string -> value of each variable
    defaults: Tuple[Any, ...]          # where neither keyword nor variable is given
    check: Callable                    # the validator: check(*values, **context) -> the field(s)
    flags: Optional[Tuple[str, ...]] = None  # trainer flag names where they differ from the keywords
    record: Optional[type] = None      # the resolved NamedTuple, accepted in place of the first keyword
    context: Optional[Callable] = None  # (fields resolved so far, batch_size) -> further arguments of `check`
    # annealed groups: the keyword whose 0 means "until the end of training", and the total_steps the
    # trainer stands in for it in sample-only mode (which never steps: any valid length)
    steps: Optional[str] = None
    stand_in: Optional[Callable] = None

    @property
    def flag_names(self) -> Tuple[str, ...]:
        return self.flags or self.keywords

    @property
    def steps_flag(self) -> str:
        return self.flag_names[self.keywords.index(self.steps)]

    def resolve(self, values, env: bool = True, **context):
        """The validated field(s) from one value per keyword. _UNSET, and None when `env`, fall back to
        the environment variable (when `env`), then to the default."""
        if self.record is not None and isinstance(values[0], self.record):
            return self.check(*values[0], **context)
        args = []
        for v, name, conv, default in zip(values, self.env, self.conv, self.defaults):
            if v is _UNSET or (env and v is None):
                v = R.env_value(name, conv) if env else None
                v = default if v is None else v
            args.append(v)
        return self.check(*args, **context)

    def is_open(self, kw) -> bool:
        """`steps` = 0 on a group that anneals: the length is still to be resolved."""
        return int(kw[self.steps]) == 0 and self.check(*(kw[k] for k in self.keywords), open_ended=True).steps == 0

    def until_end(self, kw, total_steps: Optional[int]) -> int:
        """The length that `steps` = 0 stands for in a run of `total_steps` steps (None: sample-only)."""
        total = self.stand_in(kw) if total_steps is None else total_steps
        return self.check(*(kw[k] for k in self.keywords), total_steps=total).steps


# In the order the engines resolve them. (DCGAN_D_SPECTRAL_NORM's spellings are check_spectral_norm's.)
TABLE: Dict[str, Group] = {g.fields[0]: g for g in (
    Group(("d_steps", "beta2", "lr_d", "lr_g"), ("d_steps", "beta2", "lr_d", "lr_g"),
          ("DCGAN_D_STEPS", "DCGAN_BETA2", "DCGAN_LR_D", "DCGAN_LR_G"), (int, float, float, float),
          (1, R.ADAM_BETA2, None, None), R.check_d_steps,
          flags=("d_steps", "beta2", "d_learning_rate", "g_learning_rate"),
          context=lambda o, batch_size: {"lr": o["lr"]}),
    Group(("lr_sched",), ("lr_decay", "lr_decay_start", "lr_decay_steps", "lr_end", "lr_warmup"),
          ("DCGAN_LR_DECAY", "DCGAN_LR_DECAY_START", "DCGAN_LR_DECAY_STEPS", "DCGAN_LR_END", "DCGAN_LR_WARMUP"),
          (str, int, int, float, int), ("none", 0, 0, 0.0, 0), R.check_lr_schedule,
          flags=("lr_decay", "lr_decay_start", "lr_decay_steps", "lr_end", "lr_warmup_steps"),
          record=R.LrSchedule, steps="lr_decay_steps", stand_in=lambda kw: int(kw["lr_decay_start"]) + 1),
    Group(("noise",), ("instance_noise", "instance_noise_end", "instance_noise_steps"),
          ("DCGAN_INSTANCE_NOISE", "DCGAN_INSTANCE_NOISE_END", "DCGAN_INSTANCE_NOISE_STEPS"), (float, float, int),
          (0.0, 0.0, 0), R.check_instance_noise, record=R.InstanceNoise, steps="instance_noise_steps",
          stand_in=lambda kw: 1),
    Group(("aug",), ("d_augment",), ("DCGAN_D_AUGMENT",), (str,), ("",), R.check_d_augment),
    Group(("color",), ("d_color_augment",), ("DCGAN_D_COLOR_AUGMENT",), (str,), ("",), R.check_d_color),
    Group(("ada",), ("d_augment_p", "ada_target", "ada_interval", "ada_kimg"),
          ("DCGAN_D_AUGMENT_P", "DCGAN_ADA_TARGET", "DCGAN_ADA_INTERVAL", "DCGAN_ADA_KIMG"),
          (float, float, int, float), (-1.0, 0.0, 4, 500.0), R.check_ada, record=R.DAda,
          context=lambda o, batch_size: {"augmented": o["aug"].active or o["color"].active,
                                         "batch_size": batch_size}),
    Group(("topk",), ("g_topk", "g_topk_steps"), ("DCGAN_G_TOPK", "DCGAN_G_TOPK_STEPS"), (float, int), (1.0, 0),
          R.check_g_topk, record=R.GTopK, steps="g_topk_steps", stand_in=lambda kw: 1),
    Group(("g_ema_decay",), ("g_ema_decay",), ("DCGAN_G_EMA_DECAY",), (float,), (0.0,), R.check_ema_decay),
    Group(("gan_loss", "label_smooth"), ("gan_loss", "label_smooth"), ("DCGAN_GAN_LOSS", "DCGAN_LABEL_SMOOTH"),
          (str, float), ("bce", 0.0), R.check_gan_loss),
    Group(("d_spectral_norm",), ("d_spectral_norm",), ("DCGAN_D_SPECTRAL_NORM",), (str,), (False,),
          R.check_spectral_norm),
)}

KEYWORDS = frozenset(k for g in TABLE.values() for k in g.keywords)
ENV_NAMES = tuple(n for g in TABLE.values() for n in g.env)
ANNEALED = tuple(g for g in TABLE.values() if g.steps)


class StepOptions(NamedTuple):
    """Every option of a training step, validated."""
    lr: float
    beta1: float
    d_steps: int
    beta2: float
    lr_d: float
    lr_g: float
    lr_sched: R.LrSchedule
    noise: R.InstanceNoise
    aug: R.DAugment
    color: R.DColor
    ada: R.DAda
    topk: R.GTopK
    g_ema_decay: float
    gan_loss: str
    label_smooth: float
    d_spectral_norm: bool


def known(keywords: Dict[str, Any]) -> Dict[str, Any]:
    """The option keywords among `keywords` (the engines are handed shared dictionaries)."""
    return {k: v for k, v in keywords.items() if k in KEYWORDS}


def resolve(batch_size: Optional[int] = None, env: bool = True, lr: float = 2e-4, beta1: float = 0.5,
            **keywords) -> StepOptions:
    """The validated record of the option keywords. env: a keyword that is None or not given takes
    its environment variable, then its default. Not env: one that is not given takes its default,
    and the environment is not read."""
    out: Dict[str, Any] = {"lr": float(lr), "beta1": float(beta1)}
    for g in TABLE.values():
        res = g.resolve([keywords.pop(k, _UNSET) for k in g.keywords], env,
                        **(g.context(out, batch_size) if g.context else {}))
        out.update(zip(g.fields, res if len(g.fields) > 1 else (res,)))
    if keywords:
        raise TypeError("unknown training option(s): %s" % ", ".join(sorted(keywords)))
    return StepOptions(**out)


def resolve_group(name: str, values, **context):
    """One group of TABLE from the engines' arguments (None = the environment's default)."""
    return TABLE[name].resolve(values, True, **context)


def open_ended(keywords: Dict[str, Any]) -> List[Group]:
    """The annealed groups whose `*_steps` = 0 still means "until the end of training"."""
    return [g for g in ANNEALED if g.is_open(keywords)]


def from_flags(flags, total_steps: Optional[int] = None) -> Dict[str, Any]:
    """The trainer's flags as engine keywords. An open-ended `*_steps` = 0 is resolved against
    `total_steps` when that is given; else it is left at 0 (see ``open_ended``)."""
    kw = {"lr": flags.learning_rate, "beta1": flags.beta1}
    for g in TABLE.values():
        kw.update((k, getattr(flags, f)) for k, f in zip(g.keywords, g.flag_names))
    if total_steps is not None:
        for g in open_ended(kw):
            kw[g.steps] = g.until_end(kw, total_steps)
    return kw


def validate_flags(ns, error: Callable[[str], Any]) -> None:
    """Every group's validator over the parsed flags; a failure goes to `error` (which exits) as
    "--flag / --flag: message". An open-ended `*_steps` = 0 stays open: the trainer resolves it."""
    out: Dict[str, Any] = {"lr": ns.learning_rate}
    for g in TABLE.values():
        context = g.context(out, ns.batch_size) if g.context else {}
        if g.steps:
            context["open_ended"] = True
        try:
            res = g.check(*(getattr(ns, f) for f in g.flag_names), **context)
        except (ValueError, TypeError, OverflowError) as e:
            error("--%s: %s" % (" / --".join(g.flag_names), e))
        out.update(zip(g.fields, res if len(g.fields) > 1 else (res,)))
