"""CPU tests of the sliced Wasserstein distance's oracle (ops/reference.py swd_*), its flags and the
trainer's ``[SWD]`` line."""
import io
import itertools
import re

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


def _images(n, S, C, seed):
    return torch.rand(n, S, S, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def test_sorted_distance_is_the_best_matching():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(6, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    best = min(float((a - b[list(p)]).abs().mean()) for p in itertools.permutations(range(6)))
    assert abs(float(R.swd_sorted_distance(a, b)) - best) <= 1e-15


def test_distance_of_a_set_to_itself_is_zero():
    X, Y = _images(8, 32, 3, 0), _images(8, 32, 3, 1)
    assert R.swd(X, X, 16, 3) == [0.0, 0.0]
    assert all(v > 0 for v in R.swd(X, Y, 16, 3))


@pytest.mark.parametrize("S,C", [(64, 3), (28, 1)])
def test_laplacian_reconstructs_the_image(S, C):
    x = _images(2, S, C, 2).double()
    lap = R.swd_laplacian(x)
    r = lap[-1]
    for l in lap[-2::-1]:
        r = l + R.swd_up(r)
    assert [l.shape[1] for l in lap] == R.swd_levels(S)
    assert float((r - x).abs().max()) <= 8 * 2.0 ** -52


def test_levels():
    assert [R.swd_levels(S) for S in (64, 128, 28, 32)] == [[64, 32, 16], [128, 64, 32, 16], [28], [32, 16]]


def test_patch_centres_stay_inside_and_reach_both_ends():
    c = R.swd_patch_centres(64, 64, 16, 0, 7)  # 4096 draws
    assert c.shape == (4096, 2) and int(c.min()) == 3 and int(c.max()) == 12


@pytest.mark.parametrize("argv,msg", [
    (["--swd_every=2", "--swd_images=100"], "--swd_images . --swd_patches must be a power of two"),
    (["--swd_every=2", "--swd_images=512"], "--swd_images . --swd_patches must be a power of two"),
    (["--swd_images=1", "--swd_patches=8"], "--swd_images . --swd_patches must be a power of two"),
    (["--swd_every=2", "--output_size=8"], "--output_size must be at least 16"),
    (["--swd_every=-1"], "--swd_every must be >= 0"),
])
def test_flag_validation(argv, msg, capsys):
    with pytest.raises(SystemExit):
        F.parse_flags(argv)
    assert re.search(msg, capsys.readouterr().err)


def test_trainer_prints_the_swd_line(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--max_steps=3", "--swd_every=2",
                        "--swd_images=8", "--swd_patches=8", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    lines = re.findall(r"^\[SWD\] step (\d+)  28: (\S+)  avg: (\S+)$", out.getvalue(), re.M)
    assert [l[0] for l in lines] == ["2", "3"]  # every second step, and once at the end
    assert all(float(l[1]) > 0 and l[1] == l[2] for l in lines)
