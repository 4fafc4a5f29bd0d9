"""``image_train.py``-compatible flag system.

Reproduces the 22 ``tf.app.flags`` definitions of the reference
(``/root/reference/image_train.py:10-40``) with the same names, types, defaults and
syntax (``--name=value``, ``--name value``, bare ``--bool``, ``--nobool``), and wires
every one of them for real (the reference ignores most of them).
New, additive flags (dtype, synthetic data, max_steps, seed, gf/df dims, DDP knobs,
profiling) are registered in the same table so ``FLAGS.__flags``-style pprint shows
the full effective configuration (reference ``image_train.py:223``).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Any, Dict, List, Optional, Sequence, Tuple

# (name, type, default, help)  -- reference flags first, in reference order.
REFERENCE_FLAGS: List[Tuple[str, str, Any, str]] = [
    ("epoch", "int", 25, "Epoch to train [25]"),
    ("learning_rate", "float", 0.0002, "Learning rate of for adam [0.0002]"),
    ("beta1", "float", 0.5, "Momentum term of adam [0.5]"),
    ("train_size", "int", math.inf, "The size of train images [np.inf]"),
    ("batch_size", "int", 64, "The size of batch images [64]"),
    ("image_size", "int", 108, "The size of image to use (will be center cropped) [108]"),
    ("output_size", "int", 64, "The size of the output images to produce [64]"),
    ("c_dim", "int", 3, "Dimension of image color. [3]"),
    ("dataset", "str", "celebA", "The name of dataset [celebA, mnist, lsun]"),
    ("checkpoint_dir", "str", "checkpoint", "Directory name to save the checkpoints [checkpoint]"),
    ("sample_dir", "str", "samples", "Directory name to save the image samples [samples]"),
    ("is_train", "bool", False, "True for training, False for testing [False]"),
    ("is_crop", "bool", False, "True for training, False for testing [False]"),
    ("visualize", "bool", False, "True for visualizing, False for nothing [False]"),
    ("data_dir", "str", "train", "dir for train set"),
    ("sample_image_dir", "str", "sample_data", "dir for train set"),
    ("ps_hosts", "str", "", "Comma-separated list of hostname:port pairs"),
    ("worker_hosts", "str", "", "Comma-separated list of hostname:port pairs"),
    ("job_name", "str", "", "One of 'ps', 'worker'"),
    ("task_index", "int", 0, "Index of task within the job"),
    ("log_device_placement", "bool", True, "whether to log the device placement"),
    ("save_summaries_secs", "int", 10, "Save summaries interval seconds."),
]

# Additive flags of this framework (not in the reference).
EXTRA_FLAGS: List[Tuple[str, str, Any, str]] = [
    ("dtype", "str", "bf16", "compute dtype: bf16 | fp16 (dynamic loss scaling) | fp32 (reference precision)"),
    ("device", "str", "auto", "auto | cpu | cuda (cuda == the local MI355X via HIP)"),
    ("synthetic", "bool", False, "use synthetic images of the configured shape instead of TFRecords"),
    ("max_steps", "int", 1200000, "stop after this many global steps (reference hard-codes 1,200,000)"),
    ("seed", "int", 0, "base RNG seed; rank r uses seed + r for z and data order"),
    ("gf_dim", "int", 64, "generator base channel count"),
    ("df_dim", "int", 64, "discriminator base channel count"),
    ("z_dim", "int", 100, "latent dimension"),
    ("depth", "int", 0, "number of stride-2 stages (0 = auto from output_size)"),
    ("max_channels", "int", 0, "cap on per-layer channels (0 = no cap)"),
    ("save_model_secs", "float", 600.0,"chief checkpoint interval in seconds (reference Supervisor default 600)"),
    ("keep_checkpoints", "int", 5, "number of checkpoints to keep (TF Saver default 5)"),
    ("sample_every", "int", 100, "sample when global_step %% sample_every == 1 (reference: 100)"),
    ("engine", "str", "auto", "auto | hip | reference : which training step implementation"),
    ("graph", "bool", False, "replay the HIP training step as hipGraph(s) instead of the C++ launch replay "
                              "(measured 1-3 %% slower: profiles/r5/ab_eager_vs_graph_r5.txt)"),
    ("bucket_mb", "float", 32.0, "gradient all-reduce bucket size in MiB (HIP engine: one call per overlap window)"),
    ("allreduce_dtype", "str", "fp32", "gradient all-reduce wire dtype: fp32 | bf16"),
    ("shard_data", "bool", True, "give every rank a disjoint shard of the input files"),
    ("shuffle_buffer", "int", 10776, "shuffle-buffer min_after_dequeue (reference: 10% of 107,766)"),
    ("loader_threads", "int", 16, "native TFRecord reader threads (reference: 16 queue runners)"),
    ("bn_zero_debias", "bool", False, "apply TF>=0.12 zero-debiasing to BN moving averages"),
    ("profile_steps", "str", "", "a:b -> run torch.profiler over global steps [a, b)"),
    ("log_every", "int", 1, "print the step line every N steps (reference: every step)"),
    ("summaries", "bool", True, "write TensorBoard event files on the chief"),
    ("verbose", "bool", False, "verbose device / placement logging"),
    ("timing", "bool", False, "per-phase GPU timers (fwd+D bwd / G bwd / optimiser / comm) on log steps"),
    ("check_sync_every", "int", 0, "every N steps assert that parameters are bit-identical across ranks"),
    ("cache_on_device", "bool", False, "decode the whole TFRecord dataset once into GPU memory (288 GB HBM)"),
    ("collective_timeout", "float", 600.0, "seconds before a hung collective is an error (RCCL watchdog)"),
    ("num_samples", "int", 64, "images per grid in sample-only mode (--nois_train)"),
    ("g_ema_decay", "float", 0.0, "keep an exponential moving average of the generator's weights with this decay "
                                  "(tf.train.ExponentialMovingAverage with num_updates = global step, e.g. 0.999; "
                                  "0 = off); saved in checkpoints as <var>/ExponentialMovingAverage"),
    ("sample_ema", "bool", True, "sample grids / --nois_train / --visualize draw from the generator's moving "
                                 "average when --g_ema_decay keeps one (--nosample_ema: the last iterate)"),
    ("gan_loss", "str", "bce", "GAN objective: bce (the reference's sigmoid cross-entropy losses) | lsgan "
                               "(least squares) | hinge"),
    ("label_smooth", "float", 0.0, "one-sided label smoothing s, 0 <= s < 0.5: D's real target becomes 1 - s "
                                   "(bce and lsgan; the fake target and G's target do not move)"),
    ("d_spectral_norm", "bool", False, "spectral normalisation of the discriminator's conv kernels and head: D "
                                       "computes with W / sigma(W), sigma from one power-iteration step per "
                                       "training step. In front of a batch norm it mostly acts on layer 0 and the "
                                       "head (BN is scale-invariant); the SN-GAN recipe is --gan_loss=hinge "
                                       "--d_spectral_norm --nod_batch_norm"),
    ("d_batch_norm", "bool", True, "batch norm in the discriminator (--nod_batch_norm: a BN-free D, no d_bn* "
                                   "variables); SN-GAN recipe: --gan_loss=hinge --d_spectral_norm --nod_batch_norm"),
    ("d_steps", "int", 1, "discriminator updates per generator update, 1..16: each training step runs d_steps - 1 "
                          "D-only sub-steps (fresh z, own real batch, Adam over D alone) before the full step; "
                          "SN-GAN / WGAN-style training uses 5. An epoch counts d_steps x W x B images per step"),
    ("beta2", "float", 0.999, "Adam's second-moment decay, 0 <= beta2 < 1 (SN-GAN: --beta1=0 --beta2=0.9)"),
    ("d_learning_rate", "float", 0.0, "learning rate of the discriminator's Adam (TTUR); 0 = --learning_rate"),
    ("g_learning_rate", "float", 0.0, "learning rate of the generator's Adam (TTUR); 0 = --learning_rate"),
    ("lr_decay", "str", "none", "learning-rate schedule, one of none, linear, cosine, exponential: both networks' "
                                "rates times a factor of the global step that falls from 1 to --lr_end over "
                                "--lr_decay_steps steps from --lr_decay_start on (SN-GAN: --lr_decay=linear; pix2pix: "
                                "a constant first half with --lr_decay_start)"),
    ("lr_decay_start", "int", 0, "first step of the decay: the factor is 1 up to and including this global step"),
    ("lr_decay_steps", "int", 0, "length of the decay in steps, 1..2^24; 0 = until the end of training (max_steps after "
                                 "the --epoch cap, minus --lr_decay_start)"),
    ("lr_end", "float", 0.0, "final factor, 0 <= lr_end <= 1, reached exactly (> 0 with --lr_decay=exponential)"),
    ("lr_warmup_steps", "int", 0, "linear warm-up: for the first n steps the factor is also times (step + 1) / n"),
    ("instance_noise", "float", 0.0, "instance noise on the discriminator's inputs: D is trained on x + sigma * eps, "
                                     "eps ~ N(0, I), for the real and the fake half alike; sigma at step 0, "
                                     "0 <= sigma <= 2, annealed linearly to --instance_noise_end. 0 (with "
                                     "--instance_noise_end=0) turns it off"),
    ("instance_noise_end", "float", 0.0, "sigma at the end of the anneal, 0 <= sigma <= 2 (equal to --instance_noise: "
                                         "a constant sigma)"),
    ("instance_noise_steps", "int", 0, "length of the anneal in steps, 1..2^24; 0 = until the end of training "
                                       "(max_steps after the --epoch cap)"),
    ("d_augment", "str", "", "differentiable augmentation (DiffAugment) of the discriminator's inputs, reals and "
                                "fakes alike, G's gradient passing through it: a comma-separated list of "
                                "translation (up to 1/8 of the image, zero fill) and cutout (half the image's "
                                "side); empty or none turns it off"),
    ("d_color_augment", "str", "", "DiffAugment's color policy on the discriminator's inputs, ahead of --d_augment: "
                                      "a comma-separated list of brightness, saturation and contrast, each drawn per "
                                      "sample and step; empty or none turns it off"),
    ("d_augment_p", "float", -1.0, "probability of each policy selected by --d_augment / --d_color_augment per sample, "
                                   "0 <= p <= 1. -1: 1 without --ada_target (every policy on every sample) and 0 with "
                                   "it (the start of the adaptive run); a value below 1 without --ada_target is a fixed p"),
    ("ada_target", "float", 0.0, "adaptive augmentation probability (ADA): the target for r_t = E[sign(D(real))], "
                                 "0 < target < 1 (0.6 as published); p rises while r_t is above it and falls while "
                                 "below. 0 turns the controller off"),
    ("ada_interval", "int", 4, "steps per adjustment of p, 1..2^16"),
    ("ada_kimg", "float", 500.0, "thousands of real images over which p can move from 0 to 1, > 0"),
    ("g_topk", "float", 1.0, "top-k generator updates: G learns only from the k fakes the discriminator scores "
                             "highest, k annealed linearly from the batch size down to ceil(g_topk * batch_size); "
                             "the final fraction, 0 < g_topk <= 1. 1 turns it off"),
    ("g_topk_steps", "int", 0, "length of the anneal of k in steps, 1..2^24; 0 = until the end of training "
                               "(max_steps after the --epoch cap)"),
]

ALL_FLAGS = REFERENCE_FLAGS + EXTRA_FLAGS


class Flags:
    """Attribute bag that also exposes ``__flags`` like TF 0.x's ``FLAGS``."""

    def __init__(self, values: Dict[str, Any], explicit: Optional[Sequence[str]] = None):
        object.__setattr__(self, "_values", dict(values))
        object.__setattr__(self, "_explicit", frozenset(explicit or ()))

    def explicitly_set(self, name: str) -> bool:
        """True when the flag appeared on the command line (``--x``, ``--x=v``, ``--nox``)."""
        return name in object.__getattribute__(self, "_explicit")

    def __getattr__(self, name: str) -> Any:
        values = object.__getattribute__(self, "_values")
        if name == "__flags":
            return dict(values)
        if name in values:
            return values[name]
        raise AttributeError(name)

    def __setattr__(self, name: str, value: Any) -> None:
        self._values[name] = value

    def as_dict(self) -> Dict[str, Any]:
        return dict(self._values)

    def __repr__(self) -> str:  # pragma: no cover - cosmetic
        return "Flags(%r)" % (self._values,)


def _parse_bool(text: str) -> bool:
    low = text.strip().lower()
    if low in ("1", "true", "t", "yes", "y"):
        return True
    if low in ("0", "false", "f", "no", "n"):
        return False
    raise argparse.ArgumentTypeError("invalid boolean value: %r" % text)


def _parse_int(text: str) -> Any:
    low = text.strip().lower()
    if low in ("inf", "np.inf", "infinity"):
        return math.inf
    return int(text)


_CONVERTERS = {"int": _parse_int, "float": float, "str": str, "bool": _parse_bool}


def build_parser(defaults_override: Optional[Dict[str, Any]] = None) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="image_train.py",
        description="MI355X-native distributed DCGAN training (image_train.py-compatible flags)",
        allow_abbrev=False,
    )
    overrides = defaults_override or {}
    for name, typ, default, help_text in ALL_FLAGS:
        default = overrides.get(name, default)
        if typ == "bool":
            # --name, --name=true/false, --noname  (absl/tf.app.flags semantics)
            p.add_argument("--" + name, dest=name, nargs="?", const=True, default=default,
                           type=_parse_bool, help=help_text)
            p.add_argument("--no" + name, dest=name, action="store_false", help=argparse.SUPPRESS)
        else:
            p.add_argument("--" + name, dest=name, type=_CONVERTERS[typ], default=default, help=help_text)
    return p


def parse_flags(argv: Optional[Sequence[str]] = None,
                defaults_override: Optional[Dict[str, Any]] = None) -> Flags:
    """Parse ``argv`` (without the program name). Unknown flags are an error."""
    parser = build_parser(defaults_override)
    argv = list(argv) if argv is not None else sys.argv[1:]
    ns = parser.parse_args(argv)
    if not 0.0 <= float(ns.g_ema_decay) < 1.0:
        parser.error("--g_ema_decay must satisfy 0 <= decay < 1, got %r" % (ns.g_ema_decay,))
    from ..ops.options import validate_flags  # (an open-ended --*_steps=0 stays open here: the trainer resolves it)
    validate_flags(ns, parser.error)
    names = {n for n, _, _, _ in ALL_FLAGS}
    explicit = set()
    for tok in argv:
        if tok.startswith("--"):
            key = tok[2:].split("=", 1)[0]
            if key in names:
                explicit.add(key)
            elif key.startswith("no") and key[2:] in names:
                explicit.add(key[2:])
    return Flags(vars(ns), explicit)


# --dataset presets (carpedm20/DCGAN-tensorflow naming, which the reference's flag help lists:
# "celebA, mnist, lsun"): image shape for the flags the command line did not set, and the
# ``data/<dataset>`` directory when --data_dir is left at its default and that directory exists.
DATASET_PRESETS: Dict[str, Dict[str, Any]] = {
    "celebA": {"output_size": 64, "c_dim": 3},
    "lsun": {"output_size": 64, "c_dim": 3},
    "mnist": {"output_size": 28, "c_dim": 1},
    "cifar10": {"output_size": 32, "c_dim": 3},
}


def apply_dataset_preset(flags: Flags) -> Dict[str, Any]:
    """Apply the --dataset preset in place; returns what it changed (name -> value). Unknown
    names are kept (they label checkpoints / logs) and change nothing."""
    changed: Dict[str, Any] = {}
    name = str(flags.dataset)
    preset = DATASET_PRESETS.get(name) or {k.lower(): v for k, v in DATASET_PRESETS.items()}.get(name.lower())
    for k, v in (preset or {}).items():
        if not flags.explicitly_set(k) and getattr(flags, k) != v:
            setattr(flags, k, v)
            changed[k] = v
    if not flags.explicitly_set("data_dir"):
        d = os.path.join("data", name)
        if not os.path.isdir(flags.data_dir) and os.path.isdir(d):
            flags.data_dir = d
            changed["data_dir"] = d
    return changed


def default_flags(**overrides: Any) -> Flags:
    values = {name: default for name, _, default, _ in ALL_FLAGS}
    for k, v in overrides.items():
        if k not in values:
            raise KeyError("unknown flag %r" % k)
        values[k] = v
    return Flags(values)


def cluster_from_flags(flags: Flags) -> Dict[str, Any]:
    """Map the reference's cluster flags onto a torch.distributed rendezvous.

    torchrun-style env vars (RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT) win. Without them,
    ``--worker_hosts=h0:p0,h1:p1,...`` + ``--task_index=i`` give world_size = #workers,
    rank = i and master = the first worker (the chief, reference ``image_train.py:123``).
    ``--job_name=ps`` has no meaning in synchronous DDP (there is no parameter server);
    the caller reports that and exits 0.
    """
    env = os.environ
    if "RANK" in env and "WORLD_SIZE" in env:
        return {
            "rank": int(env["RANK"]),
            "world_size": int(env["WORLD_SIZE"]),
            "local_rank": int(env.get("LOCAL_RANK", env["RANK"])),
            "master_addr": env.get("MASTER_ADDR", "127.0.0.1"),
            "master_port": int(env.get("MASTER_PORT", "29500")),
            "source": "env",
        }
    workers = [w.strip() for w in flags.worker_hosts.split(",") if w.strip()] if flags.worker_hosts else []
    if len(workers) > 1:
        host, _, port = workers[0].rpartition(":")
        if flags.task_index < 0 or flags.task_index >= len(workers):
            raise ValueError("--task_index=%d out of range for %d workers" % (flags.task_index, len(workers)))
        # one process per GPU: this worker's GPU is its index among the workers listed for the
        # same host (reference launches N workers on one box as N --worker_hosts entries)
        my_host = workers[flags.task_index].rpartition(":")[0]
        local = sum(1 for w in workers[:flags.task_index] if w.rpartition(":")[0] == my_host)
        return {
            "rank": flags.task_index,
            "world_size": len(workers),
            "local_rank": int(env.get("LOCAL_RANK", str(local))),
            "master_addr": host or "127.0.0.1",
            "master_port": int(port or 29500),
            "source": "worker_hosts",
        }
    return {"rank": 0, "world_size": 1, "local_rank": 0, "master_addr": "127.0.0.1",
            "master_port": 29500, "source": "single"}
