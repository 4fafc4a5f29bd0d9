"""Time of ``engine.swd`` on the HIP engine: the first evaluation (real side + fake side + both sorts) and a
cached one (fake side only), in HIP events around each call. Random-init weights after a few training steps.

    python benchmarks/bench_swd.py [--images 256] [--patches 128] [--output_size 64] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine  # noqa: E402
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--patches", type=int, default=128)
    ap.add_argument("--output_size", type=int, default=64)
    ap.add_argument("--c_dim", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_swd.py needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = DCGANConfig(output_size=a.output_size, c_dim=a.c_dim)
    eng = HipEngine(cfg, a.batch_size, dev, dtype=a.dtype, graph=False)
    g = torch.Generator().manual_seed(0)
    eng.set_synthetic_batch((torch.rand(a.batch_size, a.output_size, a.output_size, a.c_dim, generator=g) * 2 - 1).to(dev))
    for _ in range(3):
        eng.train_step()
    real = (torch.rand(a.images, a.output_size, a.output_size, a.c_dim, generator=g) * 2 - 1).to(dev)
    z = (torch.rand(a.images, cfg.z_dim, generator=g) * 2 - 1).to(dev)
    eng.sampler(z[:a.batch_size])  # (the sampler's program and code objects are not the metric's cost)

    def timed(refresh):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        vals = eng.swd(real, z, a.patches, 1, refresh=refresh)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), vals
    cold, vals = timed(True)  # builds the programs and loads the kernels: reported apart
    first = sorted(timed(True)[0] for _ in range(a.iters))
    cached = sorted(timed(False)[0] for _ in range(a.iters))
    res = {"metric": "swd_eval_ms", "images": a.images, "patches": a.patches, "shape": [a.output_size, a.output_size, a.c_dim],
           "dtype": a.dtype, "iters": a.iters, "cold_first_ms": round(cold, 3), "first_ms_median": round(first[len(first) // 2], 3),
           "first_ms_min_max": [round(first[0], 3), round(first[-1], 3)], "cached_ms_median": round(cached[len(cached) // 2], 3),
           "cached_ms_min_max": [round(cached[0], 3), round(cached[-1], 3)], "swd": [round(v, 4) for v in vals]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
