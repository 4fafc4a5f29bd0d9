"""GPU tests of the sliced Wasserstein distance (swd.hip) against the fp64 oracle of ops/reference.py: the
Laplacian pyramid, the patch centres, the MFMA projection with the normalisation folded in, the LDS sort
with its distance, the whole metric, and the engine's method beside an untouched training step.

Bounds. Laplacian: 1e-5 absolute (two cascaded 25-tap filters of weights summing to 1 on |x| <= 1: far
under 2 * 30 * 2^-24). Projection: per element K * 2^-23 * max_row |d|_2, d the normalised descriptors (the
dot product's bound for |theta| = 1, doubled for the folded normalisation). Sorted columns: bitwise.
Distance: N * 2^-24 * max |a - b|. End to end: 10 x the oracle's own |fp32 - fp64| on the test's inputs,
measured on the CPU as 3.03e-6 (32x32x3: levels 3.03e-6, 1.38e-6) and 1.91e-6 (28x28x1), capped at 1e-3
relative."""
import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)


def _images(n, S, C, seed):
    return torch.rand(n, S, S, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.mark.parametrize("S,C,n", [(32, 3, 2), (28, 1, 3), (64, 3, 1)])
def test_laplacian_matches_oracle(S, C, n):
    x = _images(n, S, C, 3)
    want = R.swd_laplacian(x)
    slots = [HH.slot((n, s, s, C), torch.float32) for s in R.swd_levels(S)]
    got = H().swd_laplacian(x.to(dev), out=[v for _, v in slots])
    for (buf, _), g, w in zip(slots, got, want):
        assert HH.intact(buf)
        err = float((g.double().cpu() - w).abs().max())
        print("laplacian %dx%dx%d level %d: max err %.3e" % (S, S, C, w.shape[1], err))
        assert err <= 1e-5


@pytest.mark.parametrize("n,P,s,level", [(8, 16, 32, 0), (64, 64, 16, 2), (3, 16, 28, 1)])
def test_patch_centres_match_oracle(n, P, s, level):
    if (n * P) & (n * P - 1):
        with pytest.raises(ValueError, match="power of two"):
            H().swd_patch_centres(n, P, s, level, 9, device=dev)
        return
    got = H().swd_patch_centres(n, P, s, level, 9, device=dev)
    assert torch.equal(got.cpu().long(), R.swd_patch_centres(n, P, s, level, 9))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", [16, 2048])
def test_projection_matches_oracle(C, N):
    n, s = 8, 20
    l = _images(n, s, C, 4)
    cen = R.swd_patch_centres(n, N // n, s, 1, 6)
    d = R.swd_descriptors(l.double(), cen)
    mu, sigma = R.swd_stats(d, C)
    theta = R.swd_directions(49 * C, 6, 1, 128)
    dn = ((d.reshape(N, 49, C) - mu) / sigma).reshape(N, -1)
    want = (dn @ theta.t()).t()
    got = H().swd_project(l.to(dev), cen.int().to(dev), mu.float(), sigma.float(), theta.float().to(dev))
    bound = 49 * C * 2.0 ** -23 * float(dn.norm(dim=1).max())
    err = float((got.double().cpu() - want).abs().max())
    print("projection K = %d, N = %d: max err %.3e, bound %.3e" % (49 * C, N, err, bound))
    assert got.shape == (128, N) and err <= bound


@pytest.mark.parametrize("N", [16, 64, 2048, 16384, 32768])
def test_sort_and_distance(N):
    g = torch.Generator().manual_seed(N)
    a, b = torch.randn(3, N, generator=g), torch.randn(3, N, generator=g)
    a[:, :5] = torch.tensor([0.0, -0.0, 0.0, -1.5, -1.5])   # both zeros, duplicates, negatives
    b[:, 3:9] = torch.tensor([-0.0, 0.0, 2.25, 2.25, -3.0, -0.0])
    sa, sb, dist = H().swd_sorted_distance(a.to(dev), b.to(dev))

    def by_key(x):  # the kernel's order: torch.sort of the monotone integer key (-0 < +0), mapped back
        i = x.view(torch.int32).long()
        k = torch.where(i < 0, -(i & 0x7FFFFFFF) - 1, i).sort(-1).values
        return torch.where(k < 0, -(k + 1) - 2 ** 31, k).int().view(torch.float32)
    for got, x in ((sa, a), (sb, b)):
        assert HH.same_bits(got.cpu(), by_key(x))
    want = R.swd_sorted_distance(a.double(), b.double())
    bound = N * 2.0 ** -24 * float((by_key(a) - by_key(b)).abs().max())
    err = float((dist.cpu() - want).abs().max())
    print("distance N = %d: max err %.3e, bound %.3e" % (N, err, bound))
    assert err <= bound


# (S, C, n, P) -> the oracle's largest |fp32 - fp64| over the levels, measured on the CPU on these inputs
END_TO_END = {(32, 3, 8, 16): 3.03e-6, (28, 1, 8, 8): 1.91e-6}


@pytest.mark.parametrize("S,C,n,P", list(END_TO_END))
def test_swd_matches_oracle(S, C, n, P):
    A = _images(n, S, C, 11)
    B = 0.8 * A + 0.2 * _images(n, S, C, 12)
    want = R.swd(A, B, P, 5)
    got = H().swd(A.to(dev), B.to(dev), P, 5)
    assert len(got) == len(want) == len(R.swd_levels(S))
    for s, g, w in zip(R.swd_levels(S), got, want):
        tol = min(10 * END_TO_END[S, C, n, P], 1e-3 * w)
        print("swd %dx%dx%d level %d: %.8f against %.8f, err %.3e, tolerance %.3e" % (S, S, C, s, g, w, abs(g - w), tol))
        assert w > 1.0 and abs(g - w) <= tol


def test_engine_swd_leaves_the_step_alone():
    cfg, n, P = small(), 16, 8
    eng = HH.engine(cfg, B=8)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = _images(n, cfg.output_size, cfg.c_dim, 13).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    first = eng.swd(real, z, P, 5)
    again = eng.swd(None, z, P, 5)  # the real side from the cache
    fake = torch.cat([eng.sampler(z[i:i + 8]) for i in (0, 8)])
    assert first == again == H().swd(real, fake, P, 5) and all(v > 0 for v in first)
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
