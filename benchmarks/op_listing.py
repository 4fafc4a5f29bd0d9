"""Dry-run listing of everything the HIP engine records, for comparing two trees (CPU only).

For a grid of configurations it builds ``HipEngine(..., dry_run=True)`` with every ``Program`` behind
a thin proxy and lists, per Program in creation order, each recording call (one that adds an op):
method name and all arguments. Pointers are written in a canonical form so that listings of two
processes compare equal when the recorded step is the same:

  * an integer that falls inside a tensor reachable from the engine (attributes, dicts, lists, the
    flat parameter sets, ...) becomes ``<attribute path>+<byte offset>``; of several tensors holding
    the address the largest wins, then the smallest path, so a view is named by its flat buffer;
  * a buffer with no stable path (the ``_keep`` entries) becomes ``#k+<byte offset>``, k counting such
    buffers in order of first appearance within the configuration.

The recorded positions (``_a_fwd``, ``_a_gd_end``, ``_b_split``, ``_b_top_dgrad``, ``_g_w``,
``_g_w_layer``, ``_c_split``, ``_c_split_a``) are appended. A configuration the engine rejects is
listed by its error text. Output: one sha256 per configuration and the totals; ``--dump DIR`` also
writes the JSON texts. Use: run it from the root of each tree, then diff the two outputs.

    python benchmarks/op_listing.py [--dump DIR] [--quick]
"""
import argparse
import bisect
import hashlib
import itertools
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine  # noqa: E402
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig  # noqa: E402
from distributed_tensorflow_for_dcgan_amd.ops.options import ENV_NAMES  # noqa: E402

POSITIONS = ("_a_fwd", "_a_gd_end", "_b_split", "_b_top_dgrad", "_g_w", "_g_w_layer", "_c_split", "_c_split_a")
ANONYMOUS = ("_keep", "_s_keep")  # engine attributes whose entries have no stable path
ENV = ("DCGAN_D_BATCH_NORM", "DCGAN_DDP_SHARD") + ENV_NAMES  # cleared: a listing does not depend on the caller's shell
MIN_PTR = 1 << 16  # smaller integers are sizes, counts and flags


class ProgramProxy:
    """Forwards everything to the real Program; calls that add an op are logged with their arguments."""

    def __init__(self, prog, log):
        self._prog, self.calls = prog, []
        log.append(self)

    def __getattr__(self, name):
        attr = getattr(self._prog, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            before = self._prog.size()
            out = attr(*args, **kwargs)
            if self._prog.size() != before:
                self.calls.append((name, args, kwargs))
            return out
        return call


class RecordingEngine(HipEngine):
    def _prog(self):
        if "_op_log" not in self.__dict__:
            self._op_log = []
        return ProgramProxy(super()._prog(), self._op_log)


def reachable_tensors(root):
    """[(path, tensor)] of every tensor reachable from root's attributes, and the anonymous ones."""
    named, anon, seen = [], [], set()

    def walk(obj, path, out, depth):
        if isinstance(obj, torch.Tensor):
            out.append((path, obj))
            return
        if depth > 6 or id(obj) in seen or isinstance(obj, (str, bytes, int, float, bool, type(None), ProgramProxy)):
            return
        seen.add(id(obj))
        if isinstance(obj, dict):
            for k in obj:
                walk(obj[k], "%s[%r]" % (path, k), out, depth + 1)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                walk(v, "%s[%d]" % (path, i), out, depth + 1)
        elif hasattr(obj, "__dict__") and not isinstance(obj, (type, types.ModuleType)):
            for k in sorted(vars(obj)):
                walk(vars(obj)[k], path + "." + k if path else k, anon if (not path and k in ANONYMOUS) else out,
                     depth + 1)

    walk(root, "", named, 0)
    return named, anon


class Namer:
    def __init__(self, eng):
        named, anon = reachable_tensors(eng)
        spans = {}
        for path, t in named:
            if t.numel():
                key = (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
                spans[key] = min(spans.get(key, path), path)
        for _, t in anon:
            if t.numel():
                spans.setdefault((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()), None)
        # widest span first at equal start; nested views are skipped by the containment scan below
        self.spans = sorted(spans.items(), key=lambda kv: (kv[0][0], -kv[0][1]))
        self.starts = [kv[0][0] for kv in self.spans]
        self.anon_ids = {}

    def name(self, v):
        i = bisect.bisect_right(self.starts, v)
        best = None
        for j in range(i - 1, -1, -1):  # all spans starting at or before v; keep the widest holding it
            (lo, hi), path = self.spans[j]
            if v < hi and (best is None or hi - lo > best[0][1] - best[0][0]
                           or (hi - lo == best[0][1] - best[0][0] and (path or "~") < (best[1] or "~"))):
                best = self.spans[j]
            if v - lo > (1 << 34):
                break
        if best is None:
            return None
        (lo, _), path = best
        if path is None:
            path = "#%d" % self.anon_ids.setdefault(lo, len(self.anon_ids))
        return "%s+%d" % (path, v - lo)

    def canon(self, v):
        if isinstance(v, bool) or v is None or isinstance(v, (str, float)):
            return v
        if isinstance(v, int):
            if v < MIN_PTR:
                return v
            n = self.name(v)
            return v if n is None else n
        if isinstance(v, (list, tuple)):
            return [self.canon(x) for x in v]
        if isinstance(v, dict):
            return {k: self.canon(v[k]) for k in sorted(v)}
        return repr(type(v))


def listing(cfg, B, env, **kw):
    """(JSON text, number of ops) of one configuration."""
    saved = {k: os.environ.get(k) for k in ENV}
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        try:
            eng = RecordingEngine(cfg, B, torch.device("cpu"), dry_run=True, graph=False, **kw)
        except (ValueError, RuntimeError) as e:
            return json.dumps({"rejected": "%s: %s" % (type(e).__name__, e)}), 0
        namer = Namer(eng)
        progs = [[[name, namer.canon(args), namer.canon(kwargs)] for name, args, kwargs in p.calls]
                 for p in eng._op_log]
        pos = {k: namer.canon(getattr(eng, k, None)) for k in POSITIONS}
        return json.dumps({"programs": progs, "positions": pos}, indent=0), sum(len(p) for p in progs)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def grid(quick=False):
    """(label, cfg kwargs, env, engine kwargs) of every configuration."""
    models = {"28x28x1": dict(output_size=28, c_dim=1), "64x64x3": {}, "128x128x3": dict(output_size=128)}
    for (mname, mkw), dtype, d_bn, sn, d_steps, noise, aug, color, topk, world, sched in itertools.product(
            models.items(), ("bf16", "fp16", "fp32"), (True, False), (False, True), (1, 3), (None, 0.1),
            ("", "translation,cutout"), ("", "brightness,saturation,contrast"), (None, 0.5), (1, 2), (None, "serial")):
        if quick and (mname == "128x128x3" or d_steps == 3 and (noise or aug or color or topk)):
            continue
        variants = [("", {}, {})]
        if mname == "64x64x3":
            variants.append((" force_ddp", {}, dict(ddp=True)) if world == 1
                            else (" shard", {"DCGAN_DDP_SHARD": "1"}, {}))
        # adaptive augmentation probability: a fixed p and the controller, beside the ungated listing, where
        # both augmentation switches are on and nothing else is
        adas = [("", {})]
        if aug and color and noise is None and not topk:
            adas += [(" ada=fixed", dict(d_augment_p=0.5)), (" ada=adaptive", dict(ada_target=0.6, ada_interval=2))]
        for (vname, env, vkw), (aname, akw) in itertools.product(variants, adas):
            # (DiffAugment / its color policy / top-k off keeps the label it had before the switch existed: those lines
            # compare one to one with a listing from an older tree)
            label = "%s %s d_bn=%d sn=%d d_steps=%d noise=%d world=%d sched=%s%s%s%s%s" % (
                mname, dtype, d_bn, sn, d_steps, noise is not None, world, sched or "default", vname,
                " aug=1" if aug else "", " color=1" if color else "", " topk=1" if topk else "") + aname
            kw = dict(dtype=dtype, d_spectral_norm=sn, d_steps=d_steps, instance_noise=noise or 0.0,
                      instance_noise_steps=1000, world=world, schedule=sched, **vkw, **akw)
            if aug:
                kw["d_augment"] = aug
            if color:
                kw["d_color_augment"] = color
            if topk:
                kw.update(g_topk=topk, g_topk_steps=1000)
            yield label, dict(mkw, d_bn=d_bn), env, kw


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dump", help="write each configuration's JSON text into this directory")
    ap.add_argument("--quick", action="store_true", help="a subset of the grid")
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    recorded = rejected = ops = 0
    total = hashlib.sha256()
    for label, ckw, env, kw in grid(a.quick):
        text, n = listing(DCGANConfig(**ckw), a.batch, env, **kw)
        h = hashlib.sha256(text.encode()).hexdigest()
        total.update(h.encode())
        recorded, rejected, ops = recorded + (n > 0), rejected + (n == 0), ops + n
        print("%s  %5d  %s" % (h[:16], n, label), flush=True)
        if a.dump:
            with open(os.path.join(a.dump, label.replace(" ", "_") + ".json"), "w") as f:
                f.write(text)
    print("configurations recorded %d, rejected %d, ops %d, sha256 of all %s"
          % (recorded, rejected, ops, total.hexdigest()))


if __name__ == "__main__":
    main()
