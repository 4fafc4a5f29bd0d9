"""ADA's geometric stage on the GPU (csrc/hip/dgeom.hip): the draws, the pixel moves bitwise, the resampling
and its transpose against the fp64 oracle on the RECORDED matrices, the gates, and the stage in the engine."""
import pytest
import torch

import hip_harness as HH
from hip_harness import BUILDS, dev, small
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

ENV = HH.ENV + HH.env_of("aug", "color", "noise", "ada") + ("DCGAN_D_GEOM_AUGMENT",)
_clean_env = HH.clean_env(ENV)
ALL, BLIT = R.DGeom(True, True, True, True), R.DGeom(True, True, False, False)
SEED, STEP, N = 0xFEDCBA9876543210, (1 << 32) + 3, 8
CASES = [(b, S, C) for b in ("bf16", "fp32") for S, C in ((16, 3), (28, 1))]


def _x(build, S, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, S, S, C, generator=g) * 2 - 1).to(BUILDS[build]).to(dev)


def _bound(build, S):
    """4 delta + r: delta = 16 * 2^-24 * 3 S, the fp32 error of a folded source coordinate up to 3 S; 4 = the largest
    change of a bilinear surface of |x| <= 1 per pixel of displacement; r = the output's rounding."""
    return 4 * 16 * 2.0 ** -24 * 3 * S + (2.0 ** -9 if build == "bf16" else 2.0 ** -23)


def _warp_err(y, x, params, geom, gates=None):
    want = R.geom_augment(x.cpu().double(), params.cpu(), geom, gates=gates)
    return float((y.cpu().double() - want).abs().max())


def test_draws_match_the_oracle():
    """s and theta inside 4 * 2^-24 relative of the fp64 oracle rounded to fp32, every matrix entry inside
    2^-19 absolute of the fp64 product. Measured on the MI355X over 4096 draws: s 2 x 2^-24, theta 2 x 2^-24,
    matrix 0.1 x 2^-19 (the kernel takes sin / cos of the exact turn fraction, not of the rounded theta)."""
    for n in (N, 4096):
        got, want = HH.H().geom_params(n, SEED, STEP).cpu().double(), R.geom_params(n, SEED, STEP)
        assert torch.equal(got[:, 6:], want[:, 6:])
        w32 = want[:, 4:6].float().double()
        rel = ((got[:, 4:6] - w32).abs() / w32.abs().clamp_min(1e-30)).max(0).values
        m_err = float((got[:, :4] - want[:, :4]).abs().max())
        print("n=%d: s rel %.3g theta rel %.3g (x 2^-24), matrix abs %.3g (x 2^-19)"
              % (n, float(rel[0]) * 2 ** 24, float(rel[1]) * 2 ** 24, m_err * 2 ** 19))
        assert float(rel.max()) <= 4 * 2.0 ** -24 and m_err <= 2.0 ** -19
    for p24 in (0, 1 << 23, 1 << 24):
        assert torch.equal(HH.H().gate_masks(64, SEED, STEP, 8, p24, 15).cpu(), R.gate_masks(64, SEED, STEP, 8, p24, 15))


@pytest.mark.parametrize("build,S,C", CASES)
def test_flips_and_quarter_turns_are_bitwise_moves(build, S, C):
    h, x = HH.H(), _x(build, S, C)
    buf, y = HH.slot(x.shape, x.dtype)
    _, params = h.geom_draw(x, SEED, STEP, BLIT, out=y)
    assert len({tuple(r) for r in params[:, 6:].tolist()}) > 2  # (several different moves among the 8)
    assert HH.same_bits(y, R.geom_augment(x.cpu(), params.cpu(), BLIT).to(dev)) and HH.intact(buf)
    g = _x(build, S, C, seed=1)
    buf, gx = HH.slot(x.shape, x.dtype)
    h.geom_apply(g, params, BLIT, transpose=True, out=gx)
    assert HH.same_bits(gx, R.geom_augment_transpose(g.cpu(), params.cpu(), BLIT).to(dev)) and HH.intact(buf)
    assert HH.same_bits(h.geom_apply(gx, params, BLIT), g)  # the inverse permutation


@pytest.mark.parametrize("build,S,C", CASES)
def test_warp_matches_the_fp64_oracle_on_the_recorded_matrices(build, S, C):
    """The oracle alone, fp32 against fp64 on these inputs (CPU): 2.1e-6 at S = 16, 4.5e-6 at S = 28, under a
    quarter of the bounds (1.8e-4, 3.2e-4 for fp32 output). The kernel, measured on the MI355X: fp32 1.5e-6 /
    3.7e-6, bf16 1.95e-3 (its rounding) against 2.1e-3 / 2.3e-3."""
    h, x = HH.H(), _x(build, S, C)
    buf, y = HH.slot(x.shape, x.dtype)
    _, params = h.geom_draw(x, SEED, STEP, ALL, out=y)
    err, bound = _warp_err(y, x, params, ALL), _bound(build, S)
    own = float((R.geom_augment(x.cpu().float(), params.cpu(), ALL).double()
                 - R.geom_augment(x.cpu().double(), params.cpu(), ALL)).abs().max())
    print("%s S=%d C=%d: kernel err %.3e, fp32 oracle err %.3e, bound %.3e" % (build, S, C, err, own, bound))
    assert own <= bound / 4 and err <= bound and HH.intact(buf)
    assert HH.same_bits(h.geom_apply(x, params, ALL), y)  # the probe, from the recorded matrix


@pytest.mark.parametrize("S,C", [(16, 3), (28, 1)])
def test_transpose_is_the_adjoint_and_deterministic(S, C):
    h, x, g = HH.H(), _x("fp32", S, C), _x("fp32", S, C, seed=1)
    y, params = h.geom_draw(x, SEED, STEP, ALL)
    params[6, :4] = torch.tensor([1.0, -2.0, 2.0, 1.0]) / 1.1  # a strong zoom-out, several reflection periods per axis
    params[7, :4] = torch.tensor([1.0, 0.1, -0.1, 1.0]) * 0.45  # and a zoom-in
    y = h.geom_apply(x, params, ALL)
    buf, gx = HH.slot(x.shape, x.dtype)
    h.geom_apply(g, params, ALL, transpose=True, out=gx)
    gap = abs(float((y.double() * g.double()).sum() - (x.double() * gx.double()).sum()))
    bound = N * S * S * C * 2.0 ** -23 * float(x.abs().max()) * float(g.abs().max())
    want = R.geom_augment_transpose(g.cpu().double(), params.cpu(), ALL)
    print("S=%d C=%d: |<Wx, g> - <x, W^T g>| %.3e (bound %.3e), max |W^T g - oracle| %.3e"
          % (S, C, gap, bound, float((gx.cpu().double() - want).abs().max())))
    assert gap <= bound and HH.intact(buf)
    assert HH.same_bits(h.geom_apply(g, params, ALL, transpose=True), gx)


@pytest.mark.parametrize("build,S,C", CASES)
def test_gates(build, S, C):
    h, x = HH.H(), _x(build, S, C)
    y, params, gates = h.geom_draw(x, SEED, STEP, ALL, p24=0)
    assert HH.same_bits(y, x) and not bool(gates.any())
    assert torch.equal(params[:, 4:].cpu(), h.geom_params(N, SEED, STEP)[:, 4:].cpu())  # drawn whatever the gates say
    y, params, gates = h.geom_draw(x, SEED, STEP, ALL, p24=1 << 24)
    y0, p0 = h.geom_draw(x, SEED, STEP, ALL)
    assert HH.same_bits(y, y0) and torch.equal(params, p0) and bool((gates == 15).all())
    y, params, gates = h.geom_draw(x, SEED, STEP, ALL, p24=1 << 23)
    assert torch.equal(gates.cpu(), R.gate_masks(N, SEED, STEP, 8, 1 << 23, 15)) and len(gates.unique()) > 2
    want_m = R.geom_matrix(R.geom_params(N, SEED, STEP), ALL, gates=gates.cpu()).reshape(-1, 4)
    assert float((params[:, :4].cpu().double() - want_m).abs().max()) <= 2.0 ** -19
    assert _warp_err(y, x, params, ALL, gates.cpu()) <= _bound(build, S)
    g = _x(build, S, C, seed=1)
    gx = h.geom_apply(g, params, ALL, gates=gates, transpose=True)
    want = R.geom_augment_transpose(g.cpu().double(), params.cpu(), ALL, gates=gates.cpu())
    # an input pixel sums <= 4 s^2 <= 20 output pixels (the hat's support through M^-1, reflections included), each
    # weight off by <= 2 delta: 40 delta = 10 x (4 delta), and |gx| <= 5 max |g| under the output's rounding
    assert float((gx.cpu().double() - want).abs().max()) <= 10 * _bound(build, S)


class _WithGeom:
    """ReferenceStep behind the two calls ``check_piece`` makes, fed the matrices the engine recorded."""

    def __init__(self, ref, eng):
        self.ref, self.eng = ref, eng

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, geom=self.eng.geom_params.cpu())

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z, geom=self.eng.geom_params.cpu())


GEOM = dict(d_geom_augment="xflip,rot90,scale,rotate")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_engine_step_matches_the_reference_on_the_recorded_matrices(dtype, seed=3):
    cfg, B = small(), 8
    eng, off = HH.engine(cfg, B, 1, dtype=dtype, seed=seed, **GEOM), HH.engine(cfg, B, 1, dtype=dtype, seed=seed)
    aug = HH.engine(cfg, B, 1, dtype=dtype, seed=seed, d_augment="translation")  # (swaps in the unfused image gradient)
    extra = sorted(set(eng.op_names()) - set(off.op_names()))
    assert [n for n in extra if "geom" in n] == ["d_geom", "d_geom_bwd"]
    assert set(extra) - {"d_geom", "d_geom_bwd"} <= set(aug.op_names()) - set(off.op_names())
    assert off.d_warped is None and off.geom_params is None and "d_geom" not in off.op_names()
    assert tuple(eng.geom_params.shape) == (2 * B, 8) and eng.geom_gates is None and eng._d_input() is eng.d_warped
    ref_model, ref, rdev = HH.ref_for(cfg, dtype, seed, False, **GEOM)
    real = HH.reals(B, cfg, dtype, 1)[0].to(rdev)
    eng.train_step()  # (a warm-up step moves D's layer-0 biases off the LeakyReLU's kink)
    HH.check_piece(eng, _WithGeom(ref, eng), ref_model, cfg, real, dtype, False, True, eng.train_full_step, "geom")
    want = R.geom_params(2 * B, eng._zseed(None), 1)
    got = eng.geom_params.cpu().double()
    assert torch.equal(got[:, 6:], want[:, 6:]) and float((got[:, :4] - want[:, :4]).abs().max()) <= 2.0 ** -19
    assert _warp_err(eng.d_warped, eng.d_in, eng.geom_params, ALL) <= _bound(dtype, cfg.output_size)
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    before = eng.d_warped.clone()  # eval_losses stays clean: the plain engine's ops, the stage's copy untouched
    assert eng.eval_losses(real, z)["d_loss"] > 0 and HH.same_bits(eng.d_warped, before)
    assert off.eval_losses(real, z)["d_loss"] > 0
    assert [eng.progEval.name(i) for i in range(eng.progEval.size())] == [off.progEval.name(i) for i in range(off.progEval.size())]


def test_schedule_check_with_every_input_stage_on():
    from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
    kw = dict(GEOM, d_augment="translation,cutout", d_color_augment="brightness,saturation,contrast",
              instance_noise=0.1, instance_noise_steps=10, d_steps=2, d_augment_p=0.5)
    for extra in (GEOM, kw):
        _, hazards, ops = SC.check(small(), 8, "bf16", **extra)
        assert ops > 0 and hazards == []
