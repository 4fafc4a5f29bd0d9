"""CPU tests of the kernel MMD: the oracle of ops/reference.py against a case worked by hand and a plain double loop,
the validation of --nn_mmd, and the reference engine's [MMD] line through the trainer."""
import glob
import io
import math
import re

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


def _k(d, h):
    return sum(math.exp(-(2 ** m) * d / (4 * h)) for m in range(5)) / 5


def test_oracle_on_a_hand_made_case():
    """A = {0, 2}, B = {1, 3} on a line: h = D(a0, a1) = 4; the only (A, A) and (B, B) pairs lie 4 apart, and of the
    four (A, B) pairs three lie 1 apart and (a0, b1) 9."""
    A, B = torch.tensor([[0.0], [2.0]], dtype=torch.float64), torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    m = R.nn_mmd(A, B)
    want = (4.0, _k(4, 4), _k(4, 4), (3 * _k(1, 4) + _k(9, 4)) / 4)
    assert m[:4] == pytest.approx(want, rel=1e-14) and m.mmd2 == pytest.approx(want[1] + want[2] - 2 * want[3], rel=1e-12)
    assert m.mmd2 < 0  # the unbiased estimate of two interleaved sets: reported as it is
    assert R.nn_mmd_report(m) == {"mmd2": m.mmd2, "k_rr": m.k_rr, "k_ff": m.k_ff, "k_rf": m.k_rf, "h": 4.0}
    assert not math.isfinite(R.nn_mmd(torch.ones(3, 2, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64)).mmd2)  # h = 0
    with pytest.raises(ValueError):
        R.nn_mmd(A[:1], B[:1])
    with pytest.raises(ValueError):
        R.check_nn_mmd(True, 1)
    assert R.check_nn_mmd(False, 1) is False and R.check_nn_mmd(True, 2) is True


@pytest.mark.parametrize("Mx,My,skip_aa", [(5, 4, False), (3, 6, True), (4, 0, False)])
def test_sums_and_bandwidth_against_a_double_loop(Mx, My, skip_aa):
    g = torch.Generator().manual_seed(3)
    X, Y = torch.randn(Mx, 3, generator=g, dtype=torch.float64), torch.randn(My, 3, generator=g, dtype=torch.float64)
    D = lambda x, y: sum(float(a - b) ** 2 for a, b in zip(x, y))  # noqa: E731
    h = sum(D(X[i], X[j]) for i in range(Mx) for j in range(Mx) if i != j) / (Mx * (Mx - 1))
    assert R.nn_mmd_bandwidth(X) == pytest.approx(h, rel=1e-13)
    Z, want = torch.cat([X, Y]), [0.0, 0.0, 0.0]  # AA, BB, AB over the upper triangle of the stacked set
    for i in range(Mx + My):
        for j in range(i + 1, Mx + My):
            if not (skip_aa and j < Mx):
                want[(0, 2, 1)[(i >= Mx) + (j >= Mx)]] += _k(D(Z[i], Z[j]), h)
    assert R.nn_mmd_sums(X, Y, h, skip_aa) == pytest.approx(tuple(want), rel=1e-13, abs=0)


@pytest.mark.parametrize("argv,ok", [(["--nn_mmd"], True), (["--nn_mmd", "--nn_images=1"], False),
                                     (["--nn_every=2", "--nn_images=2", "--nn_mmd"], True), (["--nn_mmd=2"], False)])
def test_flag_validation(argv, ok):
    """As --nn_k: accepted without --nn_every, and the set's size is checked as soon as the flag is named."""
    if ok:
        assert F.parse_flags(argv).nn_mmd is True and F.parse_flags([]).nn_mmd is False
    else:
        with pytest.raises(SystemExit):
            F.parse_flags(argv)


def test_reference_engine_through_the_trainer(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    from distributed_tensorflow_for_dcgan_amd.obs.events import read_events
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=32", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--max_steps=3", "--nn_every=2", "--nn_images=6",
                        "--nn_size=16", "--nn_mmd", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    lines = re.findall(r"^\[MMD\] step (\d+)  mmd2 (\S+)  k_rr (\S+)  k_ff (\S+)  k_rf (\S+)  h (\S+)$", out.getvalue(), re.M)
    assert [l[0] for l in lines] == ["2", "3"] and len(re.findall(r"^\[NN\] step", out.getvalue(), re.M)) == 2
    assert "[PRDC]" not in out.getvalue()
    for l in lines:
        mmd2, rr, ff, rf, h = map(float, l[1:])
        assert 0 < rr <= 1 and 0 < ff <= 1 and 0 < rf <= 1 and h > 0 and abs(mmd2 - (rr + ff - 2 * rf)) < 2e-4
    files = glob.glob(str(tmp_path / "ck" / "events.out.tfevents.*"))
    assert len(files) == 1
    steps = {}
    for ev in read_events(files[0]):
        for v in ev["values"]:
            steps.setdefault(v.get("tag"), []).append(ev["step"])
    assert all(steps.get("nn/" + m) == [2, 3] for m in ("mmd2", "k_rr", "k_ff", "k_rf", "acc"))
