"""CPU tests of the k-NN manifold estimates (precision, recall, density, coverage): the oracle of ops/reference.py on
a case worked out by hand, the validation of --nn_k, and the reference engine's nn_metric through the trainer."""
import glob
import io
import re

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


def test_oracle_on_a_hand_made_case():
    """5 + 5 points in K = 2, k = 2. Squared radii: rA = 9, 4, 9 (a2 has a0 and a3 both at 9: j = 0 first), 25, 101 and
    rB = 5, 2, 5, 324, 361. b0 lies in the balls of a0, a1; b1 in those of a0, a1, a2; b2 in a0..a3; b3 and b4 in none.
    a0 lies in b0, b1 (2 <= 2: a tie is inside), b2; a1 in b0, b1, b2; a2 in b2, b3, b4; a3 in b3, b4; a4 in none, and
    its nearest fake (b2, at 104) is outside its own ball (101)."""
    A = torch.tensor([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0], [6.0, 0.0], [0.0, -10.0]], dtype=torch.float64)
    B = torch.tensor([[0.0, 1.0], [1.0, 1.0], [2.0, 0.0], [20.0, 0.0], [21.0, 0.0]], dtype=torch.float64)
    d, j = R.nn_topk(A, A, 2, loo=True)
    assert d.tolist() == [[1, 9], [1, 4], [4, 9], [9, 25], [100, 101]] and j.tolist() == [[1, 2], [0, 2], [1, 0], [2, 1], [0, 1]]
    p = R.nn_prdc(A, B, 2)
    assert p.rA.tolist() == [9, 4, 9, 25, 101] and p.rB.tolist() == [5, 2, 5, 324, 361]
    assert p.hitsB.tolist() == [2, 3, 4, 0, 0] and p.hitsA.tolist() == [3, 3, 3, 2, 0]
    assert (p.precision, p.recall, p.density, p.coverage, p.k) == (3 / 5, 4 / 5, 9 / 10, 4 / 5, 2)
    assert R.nn_prdc_report(p) == {"precision": 3 / 5, "recall": 4 / 5, "density": 9 / 10, "coverage": 4 / 5, "k": 2}
    for k in (0, 5, 17):  # 1 <= k <= min(16, n - 1)
        with pytest.raises(ValueError):
            R.nn_prdc(A, B, k)


@pytest.mark.parametrize("argv", [["--nn_k=-1"], ["--nn_k=17"], ["--nn_every=2", "--nn_images=4", "--nn_k=4"]])
def test_flag_validation(argv, capsys):
    with pytest.raises(SystemExit):
        F.parse_flags(argv)
    assert re.search(r"--nn_k must be in \[0, min\(16, --nn_images - 1\)\]", capsys.readouterr().err)


def test_reference_engine_through_the_trainer(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    from distributed_tensorflow_for_dcgan_amd.obs.events import read_events
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=32", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--max_steps=3", "--nn_every=2", "--nn_images=6",
                        "--nn_size=16", "--nn_k=2", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    lines = re.findall(r"^\[PRDC\] step (\d+)  k 2  precision (\S+)  recall (\S+)  density (\S+)  coverage (\S+)$",
                       out.getvalue(), re.M)
    assert [l[0] for l in lines] == ["2", "3"] and len(re.findall(r"^\[NN\] step", out.getvalue(), re.M)) == 2
    for l in lines:
        pr, rc, dn, cv = map(float, l[1:])
        assert 0 <= pr <= 1 and 0 <= rc <= 1 and 0 <= dn <= 6 / 2 and 0 <= cv <= 1
    files = glob.glob(str(tmp_path / "ck" / "events.out.tfevents.*"))
    assert len(files) == 1
    steps = {}
    for ev in read_events(files[0]):
        for v in ev["values"]:
            steps.setdefault(v.get("tag"), []).append(ev["step"])
    assert all(steps.get("nn/" + m) == [2, 3] for m in ("precision", "recall", "density", "coverage", "acc"))
