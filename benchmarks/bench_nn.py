"""Time of ``engine.nn_metric`` on the HIP engine: the first evaluation (real side, its leave-one-out search, fake
side and the three blocks that involve it) and a cached one (fake side only), in HIP events around each call, and in
the same process ``torch.cdist`` + ``min`` over the same four blocks of the same feature matrices as the yardstick.
With ``--k`` the same for the metric with the k-NN manifold estimates next to the k = 0 numbers of the same run, the
nn_topk kernel against nn_top1 and nn_count on the (A, A) block alone, and ``torch.cdist`` + ``topk`` + the comparison
against the radii as the yardstick. With ``--mmd`` the metric with the kernel MMD, its triangular Gram kernel alone (full
and without the (A, A) pairs) against three nn_count launches over (A, A), (A, B), (B, B), and ``torch.cdist`` + ``exp``
+ ``sum`` over the same three blocks as the yardstick. With ``--fd`` the metric with the Frechet distance (``--fd_iters``
steps of the polar iteration), one launch of the cross-Gram, of P = X X^T and of the step alone, ``torch.linalg.svdvals``
of the same C where the build has it, and the distance of a second real draw against the first: the floor to compare with.

    python benchmarks/bench_nn.py [--images 1024] [--output_size 64] [--nn_size 0] [--k 0] [--mmd] [--fd] [--iters 10] [--out FILE]
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
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--output_size", type=int, default=64)
    ap.add_argument("--nn_size", type=int, default=0)
    ap.add_argument("--c_dim", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--k", type=int, default=0, help="also time the metric with precision / recall / density / coverage")
    ap.add_argument("--mmd", action="store_true", help="also time the metric with the kernel MMD and its Gram kernel alone")
    ap.add_argument("--fd", action="store_true", help="also time the metric with the Frechet distance and its GEMM launches alone")
    ap.add_argument("--fd_iters", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the result line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nn.py needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = DCGANConfig(output_size=a.output_size, c_dim=a.c_dim)
    eng = HipEngine(cfg, a.batch_size, dev, dtype=a.dtype, graph=False)
    g = torch.Generator().manual_seed(0)
    eng.set_synthetic_batch((torch.rand(a.batch_size, a.output_size, a.output_size, a.c_dim, generator=g) * 2 - 1).to(dev))
    for _ in range(3):
        eng.train_step()
    n = a.images
    real = (torch.rand(n, a.output_size, a.output_size, a.c_dim, generator=g) * 2 - 1).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=g) * 2 - 1).to(dev)
    eng.sampler(z[:a.batch_size])  # (the sampler's program and code objects are not the metric's cost)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        r = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), r
    cold, res = timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True))  # records the programs: reported apart
    first = sorted(timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True))[0] for _ in range(a.iters))
    cached = sorted(timed(lambda: eng.nn_metric(None, z, a.nn_size))[0] for _ in range(a.iters))
    nn = eng._nn
    FA, FB = nn._keep[2][1], nn._keep[3][1]  # the centred feature matrices the kernels searched

    def yard():
        out = []
        for X, Y, loo in ((FA, FA, True), (FA, FB, False), (FB, FA, False), (FB, FB, True)):
            D = torch.cdist(X, Y)
            if loo:
                D.fill_diagonal_(float("inf"))
            out.append(D.min(1))
        return out
    timed(yard)
    cd = sorted(timed(yard)[0] for _ in range(a.iters))
    K = nn.K
    med = lambda v: round(v[len(v) // 2], 3)  # noqa: E731
    out = {"metric": "nn_eval_ms", "images": n, "shape": [a.output_size, a.output_size, a.c_dim], "K": K, "dtype": a.dtype,
           "iters": a.iters, "cold_first_ms": round(cold, 3), "first_ms_median": med(first),
           "first_ms_min_max": [round(first[0], 3), round(first[-1], 3)], "cached_ms_median": med(cached),
           "cached_ms_min_max": [round(cached[0], 3), round(cached[-1], 3)], "cdist_min_4_blocks_ms_median": med(cd),
           "cdist_min_max": [round(cd[0], 3), round(cd[-1], 3)],
           "gemm_flop_first": 4 * 2.0 * n * n * nn._keep[2][1].shape[1],
           "result": {k: (round(v, 4) if isinstance(v, float) else None) for k, v in res.items() if k != "nearest"}}
    if a.k > 0:
        from distributed_tensorflow_for_dcgan_amd.ops import hip as H
        timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, k=a.k))
        first_k = sorted(timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, k=a.k))[0] for _ in range(a.iters))
        cached_k = sorted(timed(lambda: eng.nn_metric(None, z, a.nn_size, k=a.k))[0] for _ in range(a.iters))
        res_k = eng.nn_metric(None, z, a.nn_size, k=a.k)
        nk = eng._nn
        (_, FA, nA), (_, FB, nB) = nk._keep[2], nk._keep[3]
        Kp, sp, e, p = FA.shape[1], H.nn_splits(n, n), H.ext(), H._p
        part = torch.empty(sp, n, a.k, dtype=torch.int64, device=dev)
        cpart, cnt = torch.empty(sp, n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        progs = {"top1": e.Program(), "topk": e.Program(), "count": e.Program()}  # the (A, A) block's GEMM kernel alone
        progs["top1"].nn_top1("top1", p(FA), p(nA), p(FA), p(nA), p(part), n, n, Kp, 1, sp, 0)
        progs["topk"].nn_topk("topk", p(FA), p(nA), p(FA), p(nA), p(part), n, n, Kp, 1, sp, a.k, 0)
        progs["count"].nn_count("count", p(FA), p(nA), p(FA), p(nA), p(nk.rad[:n]), p(cpart), p(cnt), n, n, Kp, sp, 0)
        kern = {}
        for name, prog in progs.items():
            timed(lambda: H.run(prog))
            kern[name] = sorted(timed(lambda: H.run(prog))[0] for _ in range(a.iters))

        def yard_k():
            r, res = {}, []
            for X, Y, loo in ((FA, FA, True), (FB, FB, True), (FA, FB, False), (FB, FA, False)):
                D = torch.cdist(X, Y)
                if loo:
                    D.fill_diagonal_(float("inf"))
                    r[id(X)] = D.topk(a.k, dim=1, largest=False).values[:, -1]
                    res.append(r[id(X)])
                else:
                    res += [D.min(1), (D <= r[id(Y)][None, :]).sum(1)]
            return res
        timed(yard_k)
        cdk = sorted(timed(yard_k)[0] for _ in range(a.iters))
        out.update({"k": a.k, "first_k_ms_median": med(first_k), "first_k_ms_min_max": [round(first_k[0], 3), round(first_k[-1], 3)],
                    "cached_k_ms_median": med(cached_k), "cached_k_ms_min_max": [round(cached_k[0], 3), round(cached_k[-1], 3)],
                    "aa_kernel_ms_median": {m: med(v) for m, v in kern.items()},
                    "aa_kernel_ms_min_max": {m: [round(v[0], 3), round(v[-1], 3)] for m, v in kern.items()},
                    "cdist_topk_count_ms_median": med(cdk), "cdist_topk_count_min_max": [round(cdk[0], 3), round(cdk[-1], 3)],
                    "result_k": {m: round(v, 4) for m, v in res_k.items() if m in ("precision", "recall", "density", "coverage")}})
    if a.mmd:
        from distributed_tensorflow_for_dcgan_amd.ops import hip as H
        timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, mmd=True))
        first_m = sorted(timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, mmd=True))[0] for _ in range(a.iters))
        cached_m = sorted(timed(lambda: eng.nn_metric(None, z, a.nn_size, mmd=True))[0] for _ in range(a.iters))
        res_m = eng.nn_metric(None, z, a.nn_size, mmd=True)
        nm = eng._nn
        (_, FA, nA), (_, FB, nB) = nm._keep[2], nm._keep[3]
        Kp, sp, e, p = FA.shape[1], H.nn_splits(n, n), H.ext(), H._p
        part = torch.empty(e.nn_mmd_pairs(n, n, 0), 3, dtype=torch.float64, device=dev)
        rad, cpart, cnt = torch.zeros(n, device=dev), torch.empty(sp, n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        # the Gram kernel alone: the triangle of [A; B] (about 2 n^2 pairs) against nn_count over (A, A), (A, B), (B, B) (3 n^2)
        progs = {"triangle": e.Program(), "triangle_skip_aa": e.Program(), "count_3_blocks": e.Program()}
        progs["triangle"].nn_mmd("mmd", p(FA), p(nA), p(FB), p(nB), p(nm.bw), p(part), n, n, Kp, 0, 0)
        progs["triangle_skip_aa"].nn_mmd("mmd", p(FA), p(nA), p(FB), p(nB), p(nm.bw), p(part), n, n, Kp, 1, 0)
        for tag, (X, nX), (Y, nY) in (("aa", (FA, nA), (FA, nA)), ("ab", (FA, nA), (FB, nB)), ("bb", (FB, nB), (FB, nB))):
            progs["count_3_blocks"].nn_count("count." + tag, p(X), p(nX), p(Y), p(nY), p(rad), p(cpart), p(cnt), n, n, Kp, sp, 0)
        kern = {}
        for name, prog in progs.items():
            timed(lambda: H.run(prog))
            kern[name] = sorted(timed(lambda: H.run(prog))[0] for _ in range(a.iters))
        c4h = float(nm.bw[0]) * 4.0

        def yard_m():
            return [sum(torch.exp(-(2.0 ** m) * q) for m in range(5)).sum()
                    for q in (torch.cdist(X, Y).square_() / c4h for X, Y in ((FA, FA), (FA, FB), (FB, FB)))]
        timed(yard_m)
        cdm = sorted(timed(yard_m)[0] for _ in range(a.iters))
        mm = lambda v: [round(v[0], 3), round(v[-1], 3)]  # noqa: E731
        out.update({"first_mmd_ms_median": med(first_m), "first_mmd_ms_min_max": mm(first_m),
                    "cached_mmd_ms_median": med(cached_m), "cached_mmd_ms_min_max": mm(cached_m),
                    "mmd_workgroups": [e.nn_mmd_pairs(n, n, 0), e.nn_mmd_pairs(n, n, 1)],
                    "gram_kernel_ms_median": {m: med(v) for m, v in kern.items()},
                    "gram_kernel_ms_min_max": {m: mm(v) for m, v in kern.items()},
                    "cdist_exp_sum_3_blocks_ms_median": med(cdm), "cdist_exp_sum_min_max": mm(cdm),
                    "result_mmd": {m: round(res_m[m], 5) for m in ("mmd2", "k_rr", "k_ff", "k_rf", "h")}})
    if a.fd:
        from distributed_tensorflow_for_dcgan_amd.ops import hip as H
        timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, fd=a.fd_iters))
        first_f = sorted(timed(lambda: eng.nn_metric(real, z, a.nn_size, refresh=True, fd=a.fd_iters))[0] for _ in range(a.iters))
        cached_f = sorted(timed(lambda: eng.nn_metric(None, z, a.nn_size, fd=a.fd_iters))[0] for _ in range(a.iters))
        nf = eng._nn
        it, FA, FB, e, p = nf._keep[-1], nf._keep[2][1], nf._keep[3][1], H.ext(), H._p
        progs = {"gram": e.Program(), "ppt": e.Program(), "step": e.Program()}  # one launch each, on the metric's buffers
        progs["ppt"].nn_fd_ppt("ppt", p(it.X[0]), p(it.P), n, 0)
        progs["step"].nn_fd_step("step", p(it.P), p(it.X[0]), p(it.X[1]), n, 0)
        progs["gram"].nn_fd_gram("gram", p(FA), p(FB), p(nf.fd_c), n, FA.shape[1], 0)
        kern = {}
        for name, prog in progs.items():
            timed(lambda: H.run(prog))
            kern[name] = sorted(timed(lambda: H.run(prog))[0] for _ in range(a.iters))
        mm = lambda v: [round(v[0], 3), round(v[-1], 3)]  # noqa: E731
        res_f = eng.nn_metric(None, z, a.nn_size, fd=a.fd_iters)  # (fd_c is again this set's centred C)
        Cc = nf.fd_c[:, :n].contiguous()
        try:
            timed(lambda: torch.linalg.svdvals(Cc))
            sv = sorted(timed(lambda: torch.linalg.svdvals(Cc))[0] for _ in range(a.iters))
            svd = {"svdvals_ms_median": med(sv), "svdvals_ms_min_max": mm(sv),
                   "svdvals_nuc": float(torch.linalg.svdvals(Cc).double().sum())}
        except Exception as ex:  # (a build without a device SVD)
            svd = {"svdvals": "unavailable: %s" % type(ex).__name__}
        real2 = (torch.rand(n, a.output_size, a.output_size, a.c_dim, generator=g) * 2 - 1).to(dev)
        floor = H.nn_frechet(real, real2, a.nn_size or None, a.fd_iters)  # a second real draw: the floor of the distance
        out.update({"fd_iters": a.fd_iters, "first_fd_ms_median": med(first_f), "first_fd_ms_min_max": mm(first_f),
                    "cached_fd_ms_median": med(cached_f), "cached_fd_ms_min_max": mm(cached_f),
                    "fd_workgroups": {"ppt": e.nn_fd_ppt_groups(n), "step": e.nn_fd_step_groups(n)},
                    "fd_kernel_ms_median": {m: med(v) for m, v in kern.items()},
                    "fd_kernel_ms_min_max": {m: mm(v) for m, v in kern.items()},
                    "result_fd": {m: res_f[m] for m in ("fd", "fd_mean2", "fd_tr", "fd_nuc", "fd_tail")},
                    "real_real_floor": floor._asdict(),
                    "fp32_resolution": n * 2.0 ** -24 * (floor.tr_a + floor.tr_b)}, **svd)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
