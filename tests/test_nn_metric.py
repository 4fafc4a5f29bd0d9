"""CPU tests of the 1-NN two-sample metric: the oracle of ops/reference.py on a case worked out by hand, the
flag validation, and the reference engine's nn_metric through the trainer."""
import io
import os
import re

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


def test_oracle_on_a_hand_made_case():
    """3 + 3 points in K = 2. B0 = (1, 0) lies at distance 1 from A0 and from A1 (a column tie: j = 0) and at 1 from
    B1 (dA == dB: called real); B1 lies at 2 from A0 and A1 (the other column tie)."""
    A = torch.tensor([[0.0, 0.0], [2.0, 0.0], [10.0, 10.0]], dtype=torch.float64)
    B = torch.tensor([[1.0, 0.0], [1.0, 1.0], [10.0, 12.0]], dtype=torch.float64)
    r = R.nn_two_sample(A, B)
    assert r.dA.tolist() == [4.0, 4.0, 164.0, 1.0, 2.0, 4.0] and r.jA.tolist() == [1, 0, 1, 0, 0, 2]
    assert r.dB.tolist() == [1.0, 1.0, 4.0, 1.0, 1.0, 202.0] and r.jB.tolist() == [0, 0, 2, 1, 0, 1]
    assert r.counts == (0, 1, 6)  # no real is called real; of the fakes only B1 is called fake
    assert (r.acc_real, r.acc_fake, r.acc) == (0.0, 1.0 / 3.0, 1.0 / 6.0)
    assert r.dist_fr == 1.0 and abs(r.dist_rr - 2.0 ** 0.5) <= 1e-15  # the lower medians of dA: 2 and 4, over K = 2
    assert R.nn_report(r)["nearest"] == [0, 0, 2]


@pytest.mark.parametrize("argv,msg", [
    (["--nn_every=2", "--nn_size=24"], "--nn_size must be one of the pyramid sizes"),
    (["--nn_size=8"], "--nn_size must be one of the pyramid sizes"),
    (["--nn_images=1"], "--nn_images must be at least 2"),
    (["--nn_every=-1"], "--nn_every and --nn_grid must be >= 0"),
])
def test_flag_validation(argv, msg, capsys):
    with pytest.raises(SystemExit):
        F.parse_flags(argv)
    assert re.search(msg, capsys.readouterr().err)


def test_reference_engine_through_the_trainer(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=32", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--max_steps=3", "--nn_every=2",
                        "--nn_images=6", "--nn_size=16", "--nn_grid=3", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    lines = re.findall(r"^\[NN\] step (\d+)  1nn: (\S+) \(real (\S+)  fake (\S+)\)  fake->real (\S+)  real->real (\S+)$",
                       out.getvalue(), re.M)
    assert [l[0] for l in lines] == ["2", "3"]  # every second step, and once at the end
    for l in lines:
        acc, ar, af, fr, rr = map(float, l[1:])
        assert abs(acc - (ar + af) / 2) <= 1e-3 and 0 <= ar <= 1 and 0 <= af <= 1 and fr > 0 and rr > 0
    assert os.path.exists(tmp_path / "s" / "nn_2.png") and os.path.exists(tmp_path / "s" / "nn_3.png")
