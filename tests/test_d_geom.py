"""ADA's geometric stage on D's input (``--d_geom_augment``), CPU side: the oracle of ops/reference.py
(pixel moves bitwise, the transpose identity in fp64, autograd, the draws), the option row and the
reference engine through the trainer."""
import io

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import options as O
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

ALL = R.DGeom(True, True, True, True)
BLIT = R.DGeom(True, True, False, False)
SHAPES = [(16, 3), (28, 1)]
SEED = 0x1234ABCD5678


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for name in O.ENV_NAMES:
        monkeypatch.delenv(name, raising=False)


def _rand(*shape, seed=0, dtype=torch.float64):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1).to(dtype)


def hand_rows():
    """Eight rows: six drawn, one zoomed out over several reflection periods, one zoomed in."""
    p = R.geom_params(8, SEED, 3)
    p[6, 4:6] = torch.tensor([0.45, 0.7], dtype=torch.float64)
    p[7, 4:6] = torch.tensor([2.2, 0.7], dtype=torch.float64)
    p[:, :4] = R.geom_matrix(p, ALL).reshape(-1, 4)
    return p


@pytest.mark.parametrize("S,C", SHAPES)
def test_flips_and_quarter_turns_move_pixels_bit_for_bit(S, C):
    """k quarter turns are torch.rot90(x, k, (H, W)) -- counter-clockwise as the image is displayed -- of the
    x-flipped image: all 8 (flip, k), one per sample."""
    p = torch.zeros(8, 8, dtype=torch.float64)
    p[:, 4], p[:, 5] = 1.7, 0.3  # (drawn, but scale and rotate are off)
    p[:, 6], p[:, 7] = torch.arange(8) // 4, torch.arange(8) % 4
    p[:, :4] = R.geom_matrix(p, BLIT).reshape(-1, 4)
    for dtype in (torch.float32, torch.bfloat16):
        x = _rand(8, S, S, C, dtype=dtype)
        y = R.geom_augment(x, p, BLIT)
        for n in range(8):
            want = torch.rot90(torch.flip(x[n], (1,)) if n // 4 else x[n], n % 4, (0, 1))
            assert torch.equal(y[n], want), (dtype, n)
        assert torch.equal(R.geom_augment(x, p, BLIT, gates=torch.zeros(8)), x)  # gated off: the identity


@pytest.mark.parametrize("S,C", SHAPES)
def test_transpose_identity_in_fp64_and_autograd(S, C):
    p = hand_rows()
    x, g = _rand(8, S, S, C, seed=1).requires_grad_(True), _rand(8, S, S, C, seed=2)
    y = R.geom_augment(x, p, ALL)
    gt = R.geom_augment_transpose(g, p, ALL)
    gap = abs(float(((y * g).sum() - (x * gt).sum()).detach()))
    assert gap <= 1e-12 * float(x.detach().norm()) * float(g.norm()), gap
    (auto,) = torch.autograd.grad(y, x, g)
    assert torch.allclose(auto, gt, rtol=0, atol=1e-13)
    assert float((y.detach()[6] - x.detach()[6]).abs().max()) > 0.1  # (the hand-set rows do resample)


def test_draws_reproduce_and_cover_their_ranges():
    p = R.geom_params(4096, SEED, 7)
    assert torch.equal(p, R.geom_params(4096, SEED, 7)) and torch.equal(p[:16], R.geom_params(16, SEED, 7))
    assert not torch.equal(p[:4], R.geom_params(4, SEED, 8))
    assert not torch.equal(p[:4], R.geom_params(4, R.substep_seed(SEED, 0), 7))
    assert sorted(p[:, 6].unique().tolist()) == [0.0, 1.0] and sorted(p[:, 7].unique().tolist()) == [0.0, 1.0, 2.0, 3.0]
    assert 0.449 <= float(p[:, 4].min()) < 0.7 and 1.5 < float(p[:, 4].max()) <= 2.226
    assert -3.1416 <= float(p[:, 5].min()) and float(p[:, 5].max()) < 3.1416
    M = p[:, :4].view(-1, 2, 2)  # a scaled rotation or reflection: M M^T = I / s^2
    eye = torch.eye(2, dtype=torch.float64) / (p[:, 4] ** 2)[:, None, None]
    assert torch.allclose(M @ M.transpose(1, 2), eye, atol=1e-12)
    gates = R.gate_masks(4096, SEED, 7, R.GEOM_GATE_STREAM, 1 << 23, ALL.mask)
    assert sorted(gates.unique().tolist()) == list(range(16))
    off = R.geom_matrix(p, ALL, gates=torch.zeros(4096)).reshape(-1, 4)
    assert torch.equal(off, torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(4096, 4))


def test_the_option_row_and_its_flag(capsys, monkeypatch):
    assert R.check_d_geom(" Rotate ,xflip") == R.DGeom(True, False, False, True) and R.check_d_geom("none") == R.DGeom()
    assert [R.check_d_geom(n).mask for n in R.GEOM_POLICIES] == [1, 2, 4, 8] and ALL.describe() == "xflip,rot90,scale,rotate"
    with pytest.raises(ValueError, match="unknown policy 'shear'"):
        R.check_d_geom("scale,shear")
    kw = dict(d_geom_augment="scale,rot90")
    o = O.resolve(8, env=False, **kw)
    assert o.geom == R.DGeom(False, True, True, False) and not O.resolve(8, env=False).geom.active
    assert O.resolve(8, env=False, **O.from_flags(F.parse_flags(["--d_geom_augment=scale,rot90"]))) == o
    assert O.resolve(8, env=False, d_geom_augment=o.geom) == o
    with pytest.raises(SystemExit):
        F.parse_flags(["--d_geom_augment=xflip,shear"])
    assert "unknown policy 'shear'" in capsys.readouterr().err
    # a gate needs a policy to gate; the geometric switch alone is one
    with pytest.raises(SystemExit):
        F.parse_flags(["--d_augment_p=0.5"])
    assert "need a policy to gate" in capsys.readouterr().err
    assert O.resolve(8, env=False, d_augment_p=0.5, **kw).ada.active
    assert F.parse_flags(["--ada_target=0.6", "--d_geom_augment=xflip"]).ada_target == 0.6
    monkeypatch.setenv("DCGAN_D_GEOM_AUGMENT", "rotate")  # the environment default; an explicit argument wins
    assert O.resolve(8).geom == R.resolve_d_geom(None) == R.DGeom(False, False, False, True)
    assert not O.resolve(8, d_geom_augment="").geom.active and not O.resolve(8, env=False).geom.active


def test_reference_trainer_runs_with_the_switch_and_keeps_sample_losses_clean(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine
    from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32", "--max_steps=3",
                        "--epoch=0", "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s"),
                        "--nolog_device_placement", "--d_geom_augment=xflip,rot90,scale,rotate", "--d_augment_p=0.7"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    assert "geometric augmentation of D's inputs: xflip,rot90,scale,rotate" in out.getvalue()
    cfg = DCGANConfig(output_size=28, c_dim=1)
    on = ReferenceEngine(cfg, 4, torch.device("cpu"), seed=2, d_geom_augment="scale,rotate")
    off = ReferenceEngine(cfg, 4, torch.device("cpu"), seed=2)
    real, z = _rand(4, 28, 28, 1, dtype=torch.float32), _rand(4, cfg.z_dim, seed=3, dtype=torch.float32)
    assert on.eval_losses(real, z) == off.eval_losses(real, z)
    on.set_synthetic_batch(real), off.set_synthetic_batch(real)
    on.train_step(), off.train_step()
    assert on.last_losses() != off.last_losses()
