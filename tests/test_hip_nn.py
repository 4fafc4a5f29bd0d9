"""GPU tests of the 1-NN search and two-sample metric (nn.hip) against the fp64 oracle of ops/reference.py.

Bound. nn_top1 chooses by the Gram form d = |x|^2 + |y|^2 - 2 x.y in fp32: three K-term sums of magnitudes
|x|^2, |y|^2, |x||y| and two final roundings put one distance within gamma(x, y) = (K + 4) 2^-24 (|x| + |y|)^2,
so a choice between two candidates is wrong by at most 2 gamma. The refined distance is (x_k - y_k)^2 in fp32
summed in fp64: 4 * 2^-24 relative. The planted margins are asserted in fp64 before the device is looked at."""
import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)
EPS = 2.0 ** -24


def _rows(m, k, seed):
    return torch.rand(m, k, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _f32(x):  # the inputs are fp32 values: the oracle sees exactly what the device sees
    return x.float().double()


@pytest.mark.parametrize("Mx,My,K,loo,splits", [(24, 40, 48, False, 1), (130, 257, 784, False, 3), (200, 200, 3072, True, 2)])
def test_top1_against_oracle(Mx, My, K, loo, splits):
    X = _f32(_rows(Mx, K, 1))
    noise = _rows(Mx, K, 2)
    if loo:  # rows 2t and 2t + 1 are partners
        pi = torch.arange(Mx) ^ 1
        X[1::2] = _f32(X[0::2] + 0.05 * noise[0::2])
        X[198:] = X[196]  # rows 198 and 199 copy row 196 bitwise; the four last rows are not planted
        Y = X
        dup = (196, 198)
    else:    # a fixed permutation-like map into the My columns; the two last columns copy row 3 bitwise
        pi = (torch.arange(Mx) * 7 + 3) % (My - 2)
        assert len(set(pi.tolist())) == Mx
        Y = _f32(_rows(My, K, 3))
        Y[pi] = _f32(X + 0.05 * noise)
        dup = (3, My - 2)
        Y[My - 2:] = X[3]
    D = R.nn_distances(X, Y)
    if loo:
        D.fill_diagonal_(float("inf"))
    nx, ny = X.norm(dim=1), Y.norm(dim=1)
    gamma = (K + 4) * EPS * (nx[:, None] + ny[None, :]) ** 2
    planted = torch.ones(Mx, dtype=torch.bool)
    planted[196 if loo else dup[0]:(200 if loo else dup[0] + 1)] = False
    rest = D.clone()
    rest[torch.arange(Mx), pi] = float("inf")
    margin = rest.min(1).values - D[torch.arange(Mx), pi]
    print("K = %d: least planted margin %.2f, 2 gamma at most %.3f" % (K, float(margin[planted].min()), 2 * float(gamma.max())))
    assert bool((margin[planted] > 2 * gamma.max()).all()) and 2 * float(gamma.max()) < 5

    (bi, idx), (bd, dist) = HH.slot(Mx, torch.int32, fill=7), HH.slot(Mx, torch.float64)
    H().nn_top1(X.float().to(dev), Y.float().to(dev), loo=loo, splits=splits, out=(idx, dist))
    assert HH.intact(bi, fill=7) and HH.intact(bd)
    idx, dist = idx.cpu().long(), dist.cpu()
    assert 0 <= int(idx.min()) and int(idx.max()) < My
    assert torch.equal(idx[planted], pi[planted])                                  # 1
    if dup:
        assert int(idx[dup[0]]) == dup[1] and float(dist[dup[0]]) == 0.0           # 2
    if loo:
        assert not bool((idx == torch.arange(Mx)).any())                            # 3
    rows = torch.arange(Mx)
    chosen = D[rows, idx]
    assert bool((chosen <= D.min(1).values + 2 * gamma[rows, idx]).all())           # 4
    err = (dist - chosen).abs()
    print("refined distance: max relative error %.3e" % float((err / chosen.clamp_min(1e-30)).max()))
    assert bool((err <= 4 * EPS * chosen).all())                                    # 5


def _planted_sets(n, S, C, seed):
    """Real and fake images in which every row's nearest real and nearest fake are planted at noise scales 0.05 and
    0.075, the nearer one alternating from pair to pair: reals come in pairs (x, x + b e), fake i sits at real i + a e',
    and (a, b) is (0.05, 0.075) for the even pairs and (0.075, 0.05) for the odd ones."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, S, S, C, generator=g) * 2 - 1  # noqa: E731
    near = torch.tensor([0.05, 0.05, 0.075, 0.075]).repeat(n)[:n].view(n, 1, 1, 1)  # a: fake i to real i
    pair = torch.tensor([0.075, 0.05]).repeat(n)[:n // 2].view(n // 2, 1, 1, 1)      # b: real 2t to real 2t + 1
    A = rnd(n)
    A[1::2] = A[0::2] + pair * rnd(n // 2)
    B = A + near * rnd(n)
    return A.contiguous(), B.contiguous()


@pytest.mark.parametrize("S,C,n,size", [(32, 3, 24, 16), (28, 1, 20, 28)])
def test_two_sample_against_oracle(S, C, n, size):
    A, B = _planted_sets(n, S, C, 21)
    FA, FB = R.nn_features(A, size), R.nn_features(B, size)
    K = FA.shape[1]
    want = R.nn_two_sample(FA, FB)
    # every choice and every label has a margin above 2 gamma, in fp64, before the device is looked at
    P = torch.cat([FA, FB])
    gmax = (K + 4) * EPS * (2 * float(P.norm(dim=1).max())) ** 2
    for X, Y, loo in ((FA, FA, True), (FA, FB, False), (FB, FA, False), (FB, FB, True)):
        D = R.nn_distances(X, Y)
        if loo:
            D.fill_diagonal_(float("inf"))
        two = D.topk(2, dim=1, largest=False).values
        assert bool((two[:, 1] - two[:, 0] > 2 * gmax).all())
    gap = (want.dA - want.dB).abs()
    print("%dx%dx%d at %d: label margins from %.3f, 2 gamma %.4f" % (S, S, C, size, float(gap.min()), 2 * gmax))
    assert bool((gap > 2 * gmax).all())

    got = H().nn_two_sample(A.to(dev), B.to(dev), size)
    for a, b in ((got.jA, want.jA), (got.jB, want.jB)):
        assert torch.equal(a.cpu(), b)
    assert got.counts == want.counts and (got.acc, got.acc_real, got.acc_fake) == (want.acc, want.acc_real, want.acc_fake)
    # dist = sqrt(d / K): 4 * 2^-24 relative on d is half that on dist; 1e-5 absolute on every feature moves an RMS
    # difference by at most 2e-5 (no pyramid when size is S)
    for g, w in ((got.dist_fr, want.dist_fr), (got.dist_rr, want.dist_rr)):
        print("dist %.8f against %.8f" % (g, w))
        assert abs(g - w) <= 2 * EPS * w + (2e-5 if size != S else 0.0)


def test_engine_nn_metric_leaves_the_step_alone():
    cfg, n = small(), 16
    eng = HH.engine(cfg, B=8)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = (torch.rand(n, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    first = eng.nn_metric(real, z)
    again = eng.nn_metric(None, z)  # the real side from the cache
    fake = torch.cat([eng.sampler(z[i:i + 8]).float() for i in (0, 8)])
    assert first == again == R.nn_report(H().nn_two_sample(real, fake))
    assert 0 < first["dist_fr"] and 0 < first["dist_rr"] and len(first["nearest"]) == n
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
