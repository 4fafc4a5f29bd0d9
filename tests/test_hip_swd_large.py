"""GPU tests of the sliced Wasserstein distance above 32768 descriptors per set: the global merge sort of
swd.hip (swd_sort_chunks, swd_merge, swd_tile_sum) against torch.sort of the integer key and the fp64 oracle.

Bounds, as tests/test_hip_swd.py: sorted columns bitwise; distance N * 2^-24 * max |sort(a) - sort(b)|; end to
end min(10 g, 1e-3 w), g the oracle's own largest |fp32 - fp64| over the levels on the test's inputs."""
import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)


def _images(n, S, C, seed):
    return torch.rand(n, S, S, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _columns(N, g, planted):
    """[5, N]: random with +-0, duplicates and negatives planted; sorted; reverse-sorted; the first half above
    the second (co-ranks at the ends of a run); constant across the border of two sorted runs (ties on the split)."""
    x = torch.randn(5, N, generator=g)
    x[0, 3:3 + len(planted)] = torch.tensor(planted)
    x[1] = x[1].sort().values
    x[2] = x[2].sort(descending=True).values
    x[3] = torch.cat([x[3, :N // 2].abs() + 1, -x[3, N // 2:].abs() - 1])
    x[4, 32768 - 5000:32768 + 5000] = 0.25
    return x


def _by_key(x):  # the kernel's order: torch.sort of the monotone integer key (-0 < +0), mapped back
    i = x.view(torch.int32).long()
    k = torch.where(i < 0, -(i & 0x7FFFFFFF) - 1, i).sort(-1).values
    return torch.where(k < 0, -(k + 1) - 2 ** 31, k).int().view(torch.float32)


@pytest.mark.parametrize("N", [65536, 131072, 262144])
def test_sort_and_distance_large(N):
    g = torch.Generator().manual_seed(N)
    a = _columns(N, g, [0.0, -0.0, 0.0, -1.5, -1.5])
    b = _columns(N, g, [-0.0, 0.0, 2.25, 2.25, -3.0, -0.0])
    sa, sb, dist = H().swd_sorted_distance(a.to(dev), b.to(dev))  # a: the pass that keeps dst; b: the one against ref
    for got, x in ((sa, a), (sb, b)):
        assert HH.same_bits(got.cpu(), _by_key(x))
    want = R.swd_sorted_distance(a.double(), b.double())
    bound = N * 2.0 ** -24 * float((_by_key(a) - _by_key(b)).abs().max())
    err = float((dist.cpu() - want).abs().max())
    print("distance N = %d: max err %.3e, bound %.3e" % (N, err, bound))
    assert err <= bound


# (S, C, n, P) -> the oracle's largest |fp32 - fp64| over the levels, measured on the CPU on these inputs
# (level 32: 3.3599, 8.4e-7; level 16: 4.8923, 2.8e-7)
END_TO_END = {(32, 1, 512, 128): 8.4e-7}


@pytest.mark.parametrize("S,C,n,P", list(END_TO_END))
def test_swd_large_matches_oracle(S, C, n, P):
    A = _images(n, S, C, 11)
    B = 0.8 * A + 0.2 * _images(n, S, C, 12)
    want = R.swd(A.to(dev), B.to(dev), P, 5, max_rows=n * P)  # (fp64, on the device: seconds instead of 11 s)
    got = H().swd(A.to(dev), B.to(dev), P, 5)
    assert len(got) == len(want) == len(R.swd_levels(S))
    for s, g, w in zip(R.swd_levels(S), got, want):
        tol = min(10 * END_TO_END[S, C, n, P], 1e-3 * w)
        print("swd %dx%dx%d level %d: %.8f against %.8f, err %.3e, tolerance %.3e" % (S, S, C, s, g, w, abs(g - w), tol))
        assert w > 1.0 and abs(g - w) <= tol


def test_engine_swd_large():
    cfg, n, P, B = small(), 512, 128, 64
    eng = HH.engine(cfg, B=B)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = _images(n, cfg.output_size, cfg.c_dim, 13).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    with pytest.raises(ValueError, match="power of two in \\[16, 32768\\]"):
        eng.swd(real, z, P, 5)  # not without the opt-in
    first = eng.swd(real, z, P, 5, max_rows=n * P)
    again = eng.swd(None, z, P, 5, max_rows=n * P)  # the real side from the cache
    fake = torch.cat([eng.sampler(z[i:i + B]) for i in range(0, n, B)])
    assert first == again == H().swd(real, fake, P, 5) and all(v > 0 for v in first)
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
