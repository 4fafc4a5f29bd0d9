"""GPU tests of the k-NN search, the ball counts and the precision / recall / density / coverage metric (nn.hip)
against the fp64 oracle of ops/reference.py.

Exact part. The inputs are integers in -3..3, so every product and every partial sum of the Gram form stays below
2^24 (9 K and 36 K at K <= 3072) and is exact in fp32 whatever the order: the device must equal the oracle bit by
bit, ties and their (distance, index) order included.

Images. There the Gram form errs by at most gmax = (K + 4) 2^-24 (2 max|f|)^2 per distance (test_hip_nn.py). A
device radius lies in [r, r + 2 gmax] and a compared distance within gmax, so a count lies between the oracle's
counts at r - 3 gmax and at r + 3 gmax, row by row."""
import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)
EPS = 2.0 ** -24


def _ints(m, k, seed):
    return torch.randint(-3, 4, (m, k), generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize("Mx,My,K,k,loo,splits", [
    (24, 40, 48, 1, False, 1),
    (130, 257, 80, 5, False, 3),    # ragged tiles, K no multiple of 32, a last chunk of 1 column
    (200, 200, 3072, 3, True, 2),   # the diagonal crosses a tile edge
    (140, 130, 48, 16, False, 2),   # k at its limit, a last chunk of 2 columns
])
def test_topk_radius_and_count_are_exact(Mx, My, K, k, loo, splits):
    X = _ints(Mx, K, 1)
    if loo:  # bitwise copies inside a tile and across the tile edge at 128
        X[5], X[Mx - 1], X[130] = X[2], X[2], X[127]
        Y = X
    else:    # two columns equal to row 0, and two equal columns: a tie in every row
        Y = _ints(My, K, 2)
        Y[3], Y[My - 1], Y[7] = X[0], X[0], Y[4]
    wd, wj = R.nn_topk(X, Y, k, loo)
    assert bool((wd[:, 1:] == wd[:, :-1]).any() or k == 1) and float(wd.min()) == 0.0  # the case has ties and zeros
    Xd, Yd = X.float().to(dev), Y.float().to(dev)
    (bi, idx), (bd, dist), (br, rad) = HH.slot((Mx, k), torch.int32, fill=7), HH.slot((Mx, k), torch.float64), HH.slot(Mx, torch.float32)
    H().nn_topk(Xd, Yd, k, loo=loo, splits=splits, out=(idx, dist, rad))
    assert HH.intact(bi, fill=7) and HH.intact(bd) and HH.intact(br)
    assert torch.equal(idx.cpu().long(), wj)
    assert torch.equal(dist.cpu(), wd)
    assert torch.equal(rad.cpu().double(), wd[:, -1])
    one = H().nn_topk(Xd, Yd, k, loo=loo, splits=1)
    assert torch.equal(one[0], idx) and torch.equal(one[1], dist)

    balls = R.nn_topk(Y, Y, k, True)[0][:, -1]  # the columns' own k-NN balls
    want = R.nn_count(X, Y, balls)
    print("counts from %d to %d" % (int(want.min()), int(want.max())))
    bc, cnt = HH.slot(Mx, torch.int32, fill=7)
    H().nn_count(Xd, Yd, balls.float().to(dev), splits=splits, out=cnt)
    assert HH.intact(bc, fill=7)
    assert torch.equal(cnt.cpu().long(), want)
    assert torch.equal(H().nn_count(Xd, Yd, balls.float().to(dev), splits=1), cnt)


def _between(D, r, g):
    """Per row of D the columns inside the balls r shrunk and grown by g: the ends of the device's bracket."""
    return (D <= r[None, :] - g).sum(1), (D <= r[None, :] + g).sum(1)


@pytest.mark.parametrize("S,C,n,size,k", [(32, 3, 24, 16, 3), (28, 1, 20, 28, 2)])
def test_prdc_on_images_within_the_gram_bracket(S, C, n, size, k):
    g = torch.Generator().manual_seed(21)
    rnd = lambda m: torch.rand(m, S, S, C, generator=g) * 2 - 1  # noqa: E731
    A, B = rnd(n), rnd(n)
    B[:n // 2] = A[:n // 2] + 0.3 * rnd(n // 2)
    FA, FB = R.nn_features(A, size), R.nn_features(B, size)
    K = FA.shape[1]
    want = R.nn_prdc(FA, FB, k)
    gmax = (K + 4) * EPS * (2 * float(torch.cat([FA, FB]).norm(dim=1).max())) ** 2
    DAB = R.nn_distances(FA, FB)
    loA, hiA = _between(DAB, want.rB, 3 * gmax)        # reals in the fakes' balls
    loB, hiB = _between(DAB.t(), want.rA, 3 * gmax)    # fakes in the reals' balls
    near = DAB.min(1).values
    loC, hiC = near <= want.rA - 3 * gmax, near <= want.rA + 3 * gmax
    loose = [int((lo != hi).sum()) for lo, hi in ((loA, hiA), (loB, hiB), (loC, hiC))]
    print("%dx%dx%d at %d, k = %d: 3 gmax %.4f; rows with an open bracket: hitsA %d, hitsB %d, coverage %d of %d; oracle %s"
          % (S, S, C, size, k, 3 * gmax, loose[0], loose[1], loose[2], n, R.nn_prdc_report(want)))
    assert max(loose) <= n // 8  # in fp64, before the device is looked at

    got = H().nn_prdc(A.to(dev), B.to(dev), size, k)
    for name, h, lo, hi, ref in (("hitsA", got.hitsA, loA, hiA, want.hitsA), ("hitsB", got.hitsB, loB, hiB, want.hitsB)):
        h = h.cpu().long()
        assert bool(((lo <= h) & (h <= hi)).all()), name
        assert torch.equal(h[lo == hi], ref[lo == hi]), name
    frac = lambda m: int(m.sum()) / float(n)  # noqa: E731
    for name, v, lo, hi in (("precision", got.precision, frac(loB > 0), frac(hiB > 0)),
                            ("recall", got.recall, frac(loA > 0), frac(hiA > 0)),
                            ("density", got.density, int(loB.sum()) / float(k * n), int(hiB.sum()) / float(k * n)),
                            ("coverage", got.coverage, frac(loC), frac(hiC))):
        print("%s %.4f in [%.4f, %.4f]" % (name, v, lo, hi))
        assert lo <= v <= hi, name
    assert got.k == k


def test_engine_nn_metric_with_k_leaves_the_step_alone():
    cfg, n = small(), 16
    eng = HH.engine(cfg, B=8)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = (torch.rand(n, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    first = eng.nn_metric(real, z, k=3)
    again = eng.nn_metric(None, z, k=3)  # the real side and its balls from the cache
    fake = torch.cat([eng.sampler(z[i:i + 8]).float() for i in (0, 8)])
    plain = eng.nn_metric(real, z)
    assert plain == R.nn_report(H().nn_two_sample(real, fake))  # the parent's keys and values
    assert first == again == dict(plain, **R.nn_prdc_report(H().nn_prdc(real, fake, None, 3)))
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
