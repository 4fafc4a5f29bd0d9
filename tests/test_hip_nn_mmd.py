"""GPU tests of the kernel MMD (nn.hip: nn_mmd_bw, nn_mmd, nn_mmd_final) against the fp64 oracle of ops/reference.py.

Sums. The inputs are the integers -3..3 of test_hip_nn_prdc.py, so the Gram form is exact in fp32 and only the epilogue
is under test. Per class sum the budget is a relative 2^-14: 1 ulp of exp2 amplified 16 times by the four squarings
(2^-19), the fp32 roundings of c and of d c at |d c| <= 1.7 (2^-19 together), the worst-case linear bound of a lane's
fp32 partial over 64 x 5 positive terms (319 * 2^-24 = 2^-15.7), and a factor 2 of headroom; everything after the
lane's partial is fp64.

Images. The Gram form errs by at most gmax = (K + 4) 2^-24 (2 max|f|)^2 per distance (test_hip_nn.py) and
|dk/dd| <= 31 / (20 h), so a mean kernel value may differ from the oracle's by 2^-14 mean + 31 gmax / (20 h)."""
import pytest
import torch

import hip_harness as HH
from hip_harness import H, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu
_clean_env = HH.clean_env(HH.ENV)
EPS, REL = 2.0 ** -24, 2.0 ** -14


def _ints(m, k, seed):
    return torch.randint(-3, 4, (m, k), generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize("Mx,My,K,skip_aa", [
    (24, 24, 48, False), (24, 24, 48, True),     # one diagonal tile that holds all three classes
    (100, 100, 80, False), (100, 100, 80, True),  # row Mx inside tile 0, K no multiple of 32, a ragged last tile
    (130, 130, 48, True),                         # row Mx inside tile 1, three tile rows
    (128, 200, 3072, False), (128, 200, 3072, True),  # the boundary on a tile edge, unequal sets, long K
])
def test_class_sums_on_exact_grams(Mx, My, K, skip_aa):
    X, Y = _ints(Mx, K, 1), _ints(My, K, 2)
    X[5], Y[1], Y[My - 1] = X[2], X[0], Y[3]  # d = 0 inside A, across the A / B boundary and inside B
    h = float(torch.tensor(R.nn_mmd_bandwidth(X), dtype=torch.float32))
    want = R.nn_mmd_sums(X, Y, h, skip_aa)
    Xd, Yd = X.float().to(dev), Y.float().to(dev)
    buf, out = HH.slot(8, torch.float64)
    got = H().nn_mmd_sums(Xd, Yd, h, skip_aa, out=out).cpu().tolist()
    assert HH.intact(buf)
    print("h %.1f  S_AA, S_BB, S_AB: device %s  oracle %s  relative %s"
          % (h, got, list(want), [abs(g - w) / w if w else 0.0 for g, w in zip(got, want)]))
    for g, w in zip(got, want):
        assert abs(g - w) <= REL * w
    assert not skip_aa or got[0] == 0.0
    assert torch.equal(H().nn_mmd_sums(Xd, Yd, h, skip_aa), out[:3])  # bitwise reproducible


@pytest.mark.parametrize("S,C,n,size", [(32, 3, 24, 16), (28, 1, 20, 28)])
def test_mmd_on_images_within_the_gram_bound(S, C, n, size):
    g = torch.Generator().manual_seed(21)
    rnd = lambda: torch.rand(n, S, S, C, generator=g) * 2 - 1  # noqa: E731
    A, B = rnd(), 0.5 * rnd()  # half the amplitude: the distributions differ
    FA, FB = R.nn_features(A, size), R.nn_features(B, size)
    want = R.nn_mmd(FA, FB)
    gmax = (FA.shape[1] + 4) * EPS * (2 * float(torch.cat([FA, FB]).norm(dim=1).max())) ** 2
    bound = {m: REL * getattr(want, m) + 31 * gmax / (20 * want.h) for m in ("k_rr", "k_ff", "k_rf")}
    bound["mmd2"] = bound["k_rr"] + bound["k_ff"] + 2 * bound["k_rf"]
    print("%dx%dx%d at %d: gmax %.3e, oracle %s, bounds %s" % (S, S, C, size, gmax, R.nn_mmd_report(want), bound))
    assert bound["mmd2"] < 1e-3 and abs(want.mmd2) >= 100 * bound["mmd2"]  # in fp64, before the device is looked at

    got = H().nn_mmd(A.to(dev), B.to(dev), size)
    print("device %s" % (R.nn_mmd_report(got),))
    assert abs(got.h - want.h) <= 2.0 ** -20 * want.h  # centring by an fp32 mean, fp32 norms
    for m, b in bound.items():
        assert abs(getattr(got, m) - getattr(want, m)) <= b, m


def test_engine_nn_metric_with_mmd_leaves_the_step_alone():
    cfg, n = small(), 16
    eng = HH.engine(cfg, B=8)
    eng.train_step()
    before, names, count = HH.snap(eng), eng.op_names(), eng.kernel_count()
    real = (torch.rand(n, cfg.output_size, cfg.output_size, cfg.c_dim, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(dev)
    z = (torch.rand(n, cfg.z_dim, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    first = eng.nn_metric(real, z, mmd=True)
    again = eng.nn_metric(None, z, mmd=True)  # the bandwidth and S_AA from the cache
    fake = torch.cat([eng.sampler(z[i:i + 8]).float() for i in (0, 8)])
    plain = eng.nn_metric(real, z, mmd=False)
    assert plain == R.nn_report(H().nn_two_sample(real, fake))  # the parent's keys and values
    assert first == again == dict(plain, **R.nn_mmd_report(H().nn_mmd(real, fake)))
    assert eng.op_names() == names and eng.kernel_count() == count
    for x, y in zip(before, HH.snap(eng)):
        assert torch.equal(x, y)
