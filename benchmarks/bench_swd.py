"""Time of ``engine.swd`` on the HIP engine: the first evaluation (real side + fake side + both sorts) and a
cached one (fake side only), in HIP events around each call. Random-init weights after a few training steps.
Above 32768 descriptors per set (--images * --patches) give --swd_max_rows, as the trainer's flag; --sort_yardstick
also times torch.sort(dim=-1) of a float32 [512, images * patches] tensor, the sort alone, in the same process.

    python benchmarks/bench_swd.py [--images 256] [--patches 128] [--output_size 64] [--iters 10] [--out FILE]
                                   [--swd_max_rows 32768] [--sort_yardstick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine  # noqa: E402
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig  # noqa: E402


def _sort_times(sw, iters):
    """ms of the metric's own sort of one level's [J, N] columns (the cached evaluation's sort and distance)."""
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    J, N = sw.proj[0].shape
    prog, out = H.ext().Program(), []
    if N > 32768:
        prog.swd_sort_large("swd.sort_large_dist", sw.proj[0].data_ptr(), 0, sw.real_sorted[0].data_ptr(), sw.keys0.data_ptr(),
                            sw.keys1.data_ptr(), sw.tilepart.data_ptr(), sw.partial[0].data_ptr(), N, J, 0)
    else:
        prog.swd_sort_distance("swd.sort_dist", sw.proj[0].data_ptr(), 0, 0, 0, sw.real_sorted[0].data_ptr(),
                               sw.partial[0].data_ptr(), N, J, 0)
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        H.run(prog)
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--patches", type=int, default=128)
    ap.add_argument("--output_size", type=int, default=64)
    ap.add_argument("--c_dim", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--swd_max_rows", type=int, default=32768, help="largest images * patches accepted (up to 2^21)")
    ap.add_argument("--sort_yardstick", action="store_true", help="also time torch.sort of one level's columns")
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
        vals = eng.swd(real, z, a.patches, 1, refresh=refresh, max_rows=a.swd_max_rows)
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
    res["max_memory_allocated_gib"] = round(torch.cuda.max_memory_allocated() / 2.0 ** 30, 3)
    if a.sort_yardstick:  # after the peak is read: the yardstick's own buffers are not the metric's
        sw, ts = eng._swd, []
        for _ in range(min(a.iters, 3)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.sort(sw.proj[0], dim=-1)
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1))
        res["torch_sort_ms_median"] = round(sorted(ts)[len(ts) // 2], 3)
        res["sort_large_ms_median"] = round(sorted(_sort_times(sw, min(a.iters, 3)))[min(a.iters, 3) // 2], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
