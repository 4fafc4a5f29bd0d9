"""GPU tests of the Frechet distance (nn.hip: nn_fd_*) against the fp64 oracle of ops/reference.py.

Polar iteration. C = U diag(sigma) V^T with sigma geometric from 1 to 1e-3 and one exact zero: the smallest scaled
singular value is at least 1e-3 / sqrt(257) = 6.2e-5, about 24 growth steps and the quadratic phase, below the 40 run.
The device is held to the fp64 run of the same iteration on the same fp32 matrix. No tight tolerance follows from
first principles (errors in the singular values are damped, errors in the vectors add up over `iters` products of depth
n), so the bound is 4 x the largest relative deviation measured over these cases (profiles/r27/nn_fd_r27.txt:
1.3444e-8, at n = 130), and it stays below the linear worst case iters (n + 4) 2^-24 of the smallest case, 6.7e-5.

Images. mean2, tr_a and tr_b carry the fp32 mean and norms: 2^-20 relative, as the MMD's h. nuc adds the Gram form's
error gmax per element of F_A F_B^T (test_hip_nn.py), n gmax / (n - 1) on the nuclear norm."""
import functools

import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)
EPS, ITERS = 2.0 ** -24, 40
NUC_REL = 4 * 1.3444e-8
assert NUC_REL <= ITERS * (24 + 4) * EPS


@functools.lru_cache(maxsize=None)
def _spectrum(n):
    """(C as fp32 values in fp64, sum of sigma, the fp64 iteration on the exact and on the fp32 matrix)."""
    g = torch.Generator().manual_seed(n)
    U, V = (torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0] for _ in range(2))
    sigma = torch.cat([torch.logspace(0, -3, n - 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)])
    C = (U * sigma) @ V.T
    C32 = C.float().double()
    return C32, float(sigma.sum()), R.nn_polar_nuclear(C, ITERS), R.nn_polar_nuclear(C32, ITERS)


@pytest.mark.parametrize("n", [24, 100, 130, 257])  # one tile; ragged rows, k no multiple of 32; two and three tile rows
def test_polar_iteration_on_a_known_spectrum(n):
    C32, total, exact, want = _spectrum(n)
    assert abs(exact[0] - total) <= 1e-6 * total  # the oracle alone, in fp64, before the device is looked at
    Cd = C32.float().to(dev)
    buf, out = HH.slot(8, torch.float64)
    nuc, tail, alpha = H().nn_polar_nuclear(Cd, ITERS, out=out)
    assert HH.intact(buf)
    print("n %d: device nuc %.9f tail %.3e alpha %.7f  oracle %s  relative %.3e  (sum sigma %.9f)"
          % (n, nuc, tail, alpha, want, abs(nuc - want[0]) / want[0], total))
    assert abs(alpha - want[2]) <= 2 * EPS * want[2]
    assert abs(nuc - want[0]) <= NUC_REL * want[0]
    assert tail >= 0
    again = torch.empty_like(out)
    H().nn_polar_nuclear(Cd, ITERS, out=again)
    assert torch.equal(again, out) and out[7] == ITERS  # bitwise reproducible


@pytest.mark.parametrize("n", [130, 2049])  # 64 x 64 tiles, three tile rows; 128 x 128 tiles (from 2048 rows), 17, the last of one row
def test_one_step_element_by_element(n):
    """P = X X^T and X' = 1.5 X - 0.5 P X against fp64 products. A K-term fp32 dot product errs by at most
    K 2^-24 sum |a_k b_k| in any order (K + 4: headroom for the final roundings), for P bounded through
    Cauchy-Schwarz; the step adds one rounding of 1.5 x and one of the result, and is held to the device's own P."""
    e, ld = H().ext(), H().ext().nn_fd_ld(n)
    X = torch.zeros(n, ld, dtype=torch.float64)
    X[:, :n] = (torch.randn(n, n, generator=torch.Generator().manual_seed(n)) / (2 * n ** 0.5)).double()
    Xd = X.float().to(dev)
    Pd, Xn = (torch.full((n, ld), float("nan"), device=dev) for _ in range(2))  # every element, the pad columns too, is written
    prog = e.Program()
    prog.nn_fd_ppt("ppt", H()._p(Xd), H()._p(Pd), n, 0)
    prog.nn_fd_step("step", H()._p(Pd), H()._p(Xd), H()._p(Xn), n, 0)
    FA, FB = (torch.randn(n, 48, generator=torch.Generator().manual_seed(s)) for s in (1, 2))  # the cross-Gram, all tiles
    Fa, Fb, Cd = FA.to(dev), FB.to(dev), torch.full((n, ld), float("nan"), device=dev)
    prog.nn_fd_gram("gram", H()._p(Fa), H()._p(Fb), H()._p(Cd), n, 48, 0)
    H().run(prog)
    C, wantC = Cd.cpu().double(), FA.double() @ FB.double().T / (n - 1)
    errC = (C[:, :n] - wantC).abs() / (EPS * (52 * FA.double().norm(dim=1)[:, None] * FB.double().norm(dim=1)[None, :] / (n - 1)
                                              + 2 * wantC.abs()))  # the dot product, then 1 / (n - 1) in fp32 and the product by it
    assert float(errC.max()) <= 1 and not C[:, n:].any()
    P, Xn, norm = Pd.cpu().double(), Xn.cpu().double(), X.norm(dim=1)
    errP = (P[:, :n] - X @ X.T).abs() / ((n + 4) * EPS * norm[:, None] * norm[None, :])
    want = 1.5 * X - 0.5 * P[:, :n] @ X
    errX = (Xn - want).abs() / (EPS * (0.5 * (n + 4) * (P[:, :n].abs() @ X.abs()) + 1.5 * X.abs() + want.abs()) + 1e-300)
    print("n %d: largest error over its bound: P %.3f, step %.3f" % (n, float(errP.max()), float(errX.max())))
    assert float(errP.max()) <= 1 and float(errX.max()) <= 1
    assert torch.equal(P[:, :n], P[:, :n].T) and not P[:, n:].any() and not Xn[:, n:].any()  # the mirror stores; zero pads


@pytest.mark.parametrize("S,C,n,size", [(32, 3, 24, 16), (28, 1, 20, 28)])
def test_frechet_on_images_part_by_part(S, C, n, size):
    g = torch.Generator().manual_seed(21)
    rnd = lambda: torch.rand(n, S, S, C, generator=g) * 2 - 1  # noqa: E731
    A, B = rnd(), 0.5 * rnd()  # half the amplitude: the distributions differ
    FA, FB = R.nn_features(A, size), R.nn_features(B, size)
    want = R.nn_frechet(FA, FB)
    mu = FA.mean(0)  # the device centres both sets by the real mean
    gmax = (FA.shape[1] + 4) * EPS * (2 * float(torch.cat([FA - mu, FB - mu]).norm(dim=1).max())) ** 2
    bound = {m: 2.0 ** -20 * getattr(want, m) for m in ("mean2", "tr_a", "tr_b")}
    bound["nuc"] = NUC_REL * want.nuc + n * gmax / (n - 1)
    bound["fd"] = bound["mean2"] + bound["tr_a"] + bound["tr_b"] + 2 * bound["nuc"]
    print("%dx%dx%d at %d: gmax %.3e, oracle %s, bounds %s" % (S, S, C, size, gmax, want, bound))
    assert want.fd >= 100 * bound["fd"]  # in fp64, before the device is looked at

    got = H().nn_frechet(A.to(dev), B.to(dev), size, ITERS)
    print("device %s" % (got,))
    for m, b in bound.items():
        assert abs(getattr(got, m) - getattr(want, m)) <= b, m
    # converged: the last two iterates both lie within the iteration's bound of the limit, whichever way the last step went
    assert abs(got.tail) <= 2 * NUC_REL * want.nuc and got.iters == ITERS


def test_engine_nn_metric_with_fd_leaves_the_step_alone():
    cfg, n = small(), 16
    eng = HH.engine(cfg, B=8)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = (torch.rand(n, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    first = eng.nn_metric(real, z, fd=ITERS)
    again = eng.nn_metric(None, z, fd=ITERS)  # tr S_A from the cache
    fake = torch.cat([eng.sampler(z[i:i + 8]).float() for i in (0, 8)])
    plain = eng.nn_metric(real, z)
    assert plain == R.nn_report(H().nn_two_sample(real, fake))  # the parent's keys and values
    assert first == again == dict(plain, **R.nn_fd_report(H().nn_frechet(real, fake, iters=ITERS)))
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
