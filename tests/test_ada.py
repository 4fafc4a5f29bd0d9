"""Adaptive augmentation probability (ADA: --d_augment_p, --ada_target, --ada_interval, --ada_kimg), CPU
side: the gates by hand from the Philox block of each sample, the gated oracles against the ungated ones
under the smaller policy, their adjoint identities, the gate frequencies, the controller against a
hand-written table and fp64 closed forms, validation and precedence at every entry point,
``ReferenceStep`` with a fixed p against autograd on the gated input, the checkpoint round trip, the
dry-run HIP schedules (hazards, where ``ada_update`` sits and what it reads, a planted race), the switch
off, and the CLI.

The recorded gate mask of a sample is its effective policy: the policy bits whose gate is on."""
import io
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_d_color as TC
from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
from distributed_tensorflow_for_dcgan_amd.engine import schedule_check as SC
from distributed_tensorflow_for_dcgan_amd.engine.factory import ReferenceEngine, build_engine
from distributed_tensorflow_for_dcgan_amd.engine.reference_step import ReferenceStep
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.models.dcgan import DCGAN
from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F

CPU = torch.device("cpu")
ROOT = TC.ROOT
ADA_ENV = ("DCGAN_D_AUGMENT_P", "DCGAN_ADA_TARGET", "DCGAN_ADA_INTERVAL", "DCGAN_ADA_KIMG")
ENV = TC.ENV + ADA_ENV + ("DCGAN_G_TOPK", "DCGAN_G_TOPK_STEPS", "DCGAN_LABEL_SMOOTH")
SEED = TC.SEED
SEEDS, STEPS = TC.SEEDS, TC.STEPS
ONE = 1 << 24
AUG = R.DAugment(True, True)
COL = R.DColor(True, True, True)
ON = dict(d_color_augment="brightness,saturation,contrast", d_augment="translation,cutout")
FIXED = dict(ON, d_augment_p=0.5)
ADAPT = dict(ON, ada_target=0.6, ada_interval=2, ada_kimg=1.0)
_hip, small, _real, _z, _record, _name = TC._hip, TC.small, TC._real, TC._z, TC._record, TC._name


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------ 1. the gates
def test_gates_by_hand_from_the_philox_block_of_each_sample():
    """Sample n: words of the block at counter (lo32(n), hi32(n), lo32(t), hi32(t) ^ s) under the seed;
    bit i on iff (w_i >> 8) < p24. s = 4: translation, cutout; s = 5: brightness, saturation, contrast."""
    assert (R.AUG_GATE_STREAM, R.COLOR_GATE_STREAM) == (4, 5)
    assert len({0, R.NOISE_STREAM, R.AUG_STREAM, R.COLOR_STREAM, R.AUG_GATE_STREAM, R.COLOR_GATE_STREAM}) == 6
    for seed, t, p24 in itertools.product(SEEDS, STEPS, (1, 1 << 23, 5033165)):
        for stream, nbits in ((4, 2), (5, 3)):
            full = (1 << nbits) - 1
            got = R.gate_masks(5, seed, t, stream, p24, full)
            assert got.dtype == torch.int32 and tuple(got.shape) == (5,)
            for n in range(5):
                ctr = np.array([n & 0xFFFFFFFF, n >> 32, t & 0xFFFFFFFF, ((t >> 32) ^ stream) & 0xFFFFFFFF], dtype=np.uint64)
                key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
                w = [int(v) for v in R.philox4x32_10(ctr, key)]
                want = sum(int((w[i] >> 8) < p24) << i for i in range(nbits))
                assert int(got[n]) == want
            for policy in range(1, full + 1):  # bits outside the policy are cleared
                assert torch.equal(R.gate_masks(5, seed, t, stream, p24, policy), got & policy)
    # the ends: 2^24 gates nothing off, 0 everything; a sub-step's seed draws other gates
    for stream, full in ((4, 3), (5, 7)):
        assert bool((R.gate_masks(64, SEED, 3, stream, ONE, full) == full).all())
        assert not bool(R.gate_masks(64, SEED, 3, stream, 0, full).any())
        a = R.gate_masks(64, SEED, 3, stream, ONE // 2, full)
        assert not torch.equal(a, R.gate_masks(64, R.substep_seed(SEED, 0), 3, stream, ONE // 2, full))
        assert not torch.equal(a, R.gate_masks(64, SEED, 4, stream, ONE // 2, full))
    assert not torch.equal(R.gate_masks(64, SEED, 3, 4, ONE // 2, 3), R.gate_masks(64, SEED, 3, 5, ONE // 2, 3))


def test_gate_frequencies_are_binomial():
    """N = 4096 samples at p = 0.3: the count of on-gates of each policy within 5 binomial standard
    deviations of N p. Deterministic: the seed is fixed (the largest deviation is printed)."""
    N, p = 4096, 0.3
    bound = 5 * math.sqrt(N * p * (1 - p))
    assert 146 < bound < 148
    worst = 0.0
    for stream, nbits in ((4, 2), (5, 3)):
        g = R.gate_masks(N, SEED, 11, stream, R.ada_p24(p), (1 << nbits) - 1)
        for i in range(nbits):
            dev_ = abs(int(((g >> i) & 1).sum()) - N * p)
            worst = max(worst, dev_)
            assert dev_ <= bound, (stream, i, dev_)
    print("largest |count - N p| = %.1f of %.1f allowed" % (worst, bound))
    assert worst <= bound / 2  # the chosen seed passes with room


def test_p24_is_round_half_even():
    assert R.ADA_ONE == ONE and R.ada_p24(0.0) == 0 and R.ada_p24(1.0) == ONE and R.ada_p24(0.5) == ONE // 2
    assert R.ada_p24(0.3) == 5033165 and R.ada_p24(2.0 ** -25) == 0 and R.ada_p24(3 * 2.0 ** -25) == 2  # ties to even
    assert R.ada_p24(0.6) == int(np.rint(np.float64(0.6) * 2.0 ** 24))
    for bad in (-0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            R.ada_p24(bad)


# ------------------------------------------------------------------ 2. the gated oracles
def _inputs(N=6, S=9, C=3, dtype=torch.float32, seed=2):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, S, S, C, generator=gen, dtype=dtype), torch.randn(N, S, S, C, generator=gen, dtype=dtype))


def test_all_on_equals_ungated_and_all_off_is_the_identity_bitwise():
    x, g = _inputs()
    x[0, 0, 0, 0], x[1, 2, 3, 1] = -0.0, 0.0
    N, S = x.shape[0], x.shape[1]
    ap, cp = R.augment_params(N, S, SEED, 5), R.color_params(N, SEED, 5)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for aug in (AUG, R.DAugment(True, False), R.DAugment(False, True)):
        on, off = R.gate_masks(N, SEED, 5, 4, ONE, aug.mask), R.gate_masks(N, SEED, 5, 4, 0, aug.mask)
        assert torch.equal(bits(R.augment(x, ap, aug, gates=on)), bits(R.augment(x, ap, aug)))
        assert torch.equal(bits(R.augment_transpose(g, ap, aug, gates=on)), bits(R.augment_transpose(g, ap, aug)))
        assert torch.equal(bits(R.augment(x, ap, aug, gates=off)), bits(x))
        assert torch.equal(bits(R.augment_transpose(g, ap, aug, gates=off)), bits(g))
    for color in TC.SUBSETS:
        on, off = R.gate_masks(N, SEED, 5, 5, ONE, color.mask), R.gate_masks(N, SEED, 5, 5, 0, color.mask)
        assert torch.equal(bits(R.color_augment(x, cp, color, gates=on)), bits(R.color_augment(x, cp, color)))
        assert torch.equal(bits(R.color_augment_transpose(g, cp, color, gates=on)),
                           bits(R.color_augment_transpose(g, cp, color)))
        assert torch.equal(bits(R.color_augment(x, cp, color, gates=off)), bits(x))
        assert torch.equal(bits(R.color_augment_transpose(g, cp, color, gates=off)), bits(g))
    # gates=None keeps today's results (and today's code path)
    assert torch.equal(R.augment(x, ap, AUG, None), R.augment(x, ap, AUG))
    with pytest.raises(ValueError, match="one mask per sample"):
        R.augment(x, ap, AUG, gates=torch.zeros(N + 1))
    with pytest.raises(ValueError, match="one mask per sample"):
        R.color_augment(x, cp, COL, gates=torch.zeros(N - 1))


def test_each_gate_pattern_equals_the_ungated_oracle_under_the_smaller_policy():
    """Sample n under gates[n] == the same sample through the ungated oracle built for policy & gates[n],
    bitwise, forward and transpose (with the kernel's recorded Mx column too)."""
    x, g = _inputs(N=8)
    N, S = x.shape[0], x.shape[1]
    ap, cp = R.augment_params(N, S, SEED, 1), R.color_params(N, SEED, 1)
    cp4 = torch.cat([cp, R.color_mean(x)[:, None]], 1)
    for aug in (AUG, R.DAugment(True, False), R.DAugment(False, True)):
        gates = torch.arange(N) % 4
        y, t = R.augment(x, ap, aug, gates=gates), R.augment_transpose(g, ap, aug, gates=gates)
        for n in range(N):
            eff = int(gates[n]) & aug.mask
            sub = R.DAugment(bool(eff & 1), bool(eff & 2))
            want = R.augment(x[n:n + 1], ap[n:n + 1], sub) if eff else x[n:n + 1]
            want_t = R.augment_transpose(g[n:n + 1], ap[n:n + 1], sub) if eff else g[n:n + 1]
            assert torch.equal(y[n:n + 1], want) and torch.equal(t[n:n + 1], want_t), (aug, n)
    for color in TC.SUBSETS:
        gates = torch.arange(N) % 8
        for params in (cp, cp4):
            y = R.color_augment(x, params, color, gates=gates)
            t = R.color_augment_transpose(g, params, color, gates=gates)
            for n in range(N):
                eff = int(gates[n]) & color.mask
                sub = R.DColor(bool(eff & 1), bool(eff & 2), bool(eff & 4))
                want = R.color_augment(x[n:n + 1], params[n:n + 1], sub) if eff else x[n:n + 1]
                want_t = R.color_augment_transpose(g[n:n + 1], params[n:n + 1], sub) if eff else g[n:n + 1]
                assert torch.equal(y[n:n + 1], want) and torch.equal(t[n:n + 1], want_t), (color, n)


def test_gated_transposes_are_the_adjoints_in_fp64():
    """<A x, g> = <x, A^T g> with mixed gates: translation / cutout exactly (a gather; tests/test_d_augment.py
    compares its transpose bitwise), the color map's linear part to 1e-12 (tests/test_d_color.py)."""
    x, g = _inputs(N=8, dtype=torch.float64)
    N, S = x.shape[0], x.shape[1]
    ap, cp = R.augment_params(N, S, SEED, 9), R.color_params(N, SEED, 9)
    ag = R.gate_masks(N, SEED, 9, 4, ONE // 2, 3)
    cg = R.gate_masks(N, SEED, 9, 5, ONE // 2, 7)
    assert len(set(ag.tolist())) > 1 and len(set(cg.tolist())) > 2  # mixed
    lhs, rhs = float((R.augment(x, ap, AUG, gates=ag) * g).sum()), float((x * R.augment_transpose(g, ap, AUG, gates=ag)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    xr = x.clone().requires_grad_(True)
    auto, = torch.autograd.grad(R.augment(xr, ap, AUG, gates=ag), xr, g)
    assert torch.equal(auto, R.augment_transpose(g, ap, AUG, gates=ag))
    zero = torch.zeros_like(x)
    for color in TC.SUBSETS:
        Ax = R.color_augment(x, cp, color, gates=cg) - R.color_augment(zero, cp, color, gates=cg)
        Atg = R.color_augment_transpose(g, cp, color, gates=cg)
        lhs, rhs = float((Ax * g).sum()), float((x * Atg).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), color
        xr = x.clone().requires_grad_(True)
        auto, = torch.autograd.grad(R.color_augment(xr, cp, color, gates=cg), xr, g)
        assert float((auto - Atg).abs().max()) <= 1e-12, color


# ------------------------------------------------------------------ 3. the controller
# (state before, logits, thr, Tn, delta24, interval) -> state after; states are (p24, acc, cnt, r_acc, windows)
NAN, INF = float("nan"), float("inf")
TABLE = [
    # interval = 1: every step is a window. rising, falling, equal to the target
    ((100, 0, 0, 0, 0), [1.0, 2.0, 3.0, -1.0], 0.0, 1, 50, 1, (150, 0, 0, 2, 1)),
    ((100, 0, 0, 0, 0), [1.0, -2.0, -3.0, -1.0], 0.0, 1, 50, 1, (50, 0, 0, -2, 1)),
    ((100, 0, 0, 7, 3), [1.0, 2.0, -3.0, 0.0], 0.0, 1, 50, 1, (100, 0, 0, 1, 4)),
    # clamps at 0 and 2^24
    ((30, 0, 0, 0, 0), [-1.0] * 4, 0.0, 0, 50, 1, (0, 0, 0, -4, 1)),
    ((ONE - 10, 0, 0, 0, 0), [1.0] * 4, 0.0, 0, 50, 1, (ONE, 0, 0, 4, 1)),
    ((0, 0, 0, 0, 0), [-1.0] * 4, 0.0, 0, ONE, 1, (0, 0, 0, -4, 1)),
    ((0, 0, 0, 0, 0), [1.0] * 4, 0.0, 0, ONE, 1, (ONE, 0, 0, 4, 1)),
    # interval = 4: three steps accumulate, the fourth decides on the window's sum
    ((100, 0, 0, 0, 0), [1.0, 1.0, 1.0, -1.0], 0.0, 10, 7, 4, (100, 2, 1, 0, 0)),
    ((100, 2, 1, 0, 0), [1.0, 1.0, 1.0, 1.0], 0.0, 10, 7, 4, (100, 6, 2, 0, 0)),
    ((100, 6, 2, 0, 0), [1.0, 1.0, 1.0, -1.0], 0.0, 10, 7, 4, (100, 8, 3, 0, 0)),
    ((100, 8, 3, 0, 0), [1.0, 1.0, 1.0, 1.0], 0.0, 10, 7, 4, (107, 0, 0, 12, 1)),
    ((100, 8, 3, 5, 9), [1.0, 1.0, -1.0, -1.0], 0.0, 10, 7, 4, (93, 0, 0, 8, 10)),
    ((100, 8, 3, 5, 9), [1.0, 1.0, 1.0, -1.0], 0.0, 10, 7, 4, (100, 0, 0, 10, 10)),
    # NaN counts 0, +-inf count +-1, +-0 count 0 at thr = 0
    ((100, 0, 0, 0, 0), [NAN, INF, -INF, INF, 0.0, -0.0], 0.0, 0, 5, 1, (105, 0, 0, 1, 1)),
    ((100, 0, 0, 0, 0), [NAN, NAN], 0.0, 0, 5, 1, (100, 0, 0, 0, 1)),
    # the lsgan threshold: 0.5, and 0.45 with label_smooth = 0.1
    ((100, 0, 0, 0, 0), [0.6, 0.5, 0.4, 0.7], 0.5, 0, 5, 1, (105, 0, 0, 1, 1)),
    ((100, 0, 0, 0, 0), [0.46, 0.5, 0.44, 0.2], float(np.float32(0.45)), 0, 5, 1, (100, 0, 0, 0, 1)),
]


def test_controller_against_a_hand_written_table():
    for before, logits, thr, Tn, d24, iv, after in TABLE:
        got = R.ada_update(list(before), torch.tensor(logits), thr, Tn, d24, iv)
        assert len(got) == R.ADA_STATE_WORDS == 8 and got[5:] == [0, 0, 0]
        assert tuple(got[:5]) == after, (before, logits, got)
        assert tuple(R.ada_update(list(before) + [0, 0, 0], torch.tensor(logits[::-1]), thr, Tn, d24, iv)[:5]) == after  # any order
    assert R.ada_state(7) == [7, 0, 0, 0, 0, 0, 0, 0] and R.ADA_KEYS == ("p24", "acc", "cnt", "r_acc", "windows")
    assert R.ada_threshold("bce") == R.ada_threshold("hinge") == R.ada_threshold("bce", 0.2) == 0.0
    assert R.ada_threshold("lsgan") == 0.5 and R.ada_threshold("lsgan", 0.1) == float(np.float32(0.45))
    assert R.ada_sign_sum(torch.tensor([0.6, 0.4, NAN]), 0.5) == 0


def test_delta24_and_target_n_against_fp64_closed_forms():
    for W, B, iv, kimg in ((1, 64, 4, 500.0), (8, 64, 4, 500.0), (1, 8, 2, 1.0), (2, 7, 3, 0.37), (1, 1, 1, 1e9), (8, 4096, 65536, 1e-3)):
        want = int(np.clip(np.rint(np.float64(2.0 ** 24) * W * B * iv / (1000.0 * kimg)), 1, 2 ** 24))
        assert R.ada_delta24(W, B, iv, kimg) == want
    assert R.ada_delta24(1, 64, 4, 500.0) == 8590 and R.ada_delta24(1, 1, 1, 1e9) == 1 and R.ada_delta24(8, 4096, 65536, 1e-3) == ONE
    for target, B, iv in ((0.6, 64, 4), (0.6, 8, 2), (0.5, 7, 3), (0.25, 2, 1), (0.75, 2, 1), (0.999, 300, 7)):
        assert R.ada_target_n(target, B, iv) == int(np.rint(np.float64(target) * B * iv))
    assert R.ada_target_n(0.6, 64, 4) == 154 and R.ada_target_n(0.6, 8, 2) == 10
    assert R.ada_target_n(0.25, 2, 1) == 0 and R.ada_target_n(0.75, 2, 1) == 2  # halves go to the even integer


# ------------------------------------------------------------------ 4. validation and precedence
def test_check_ada_validates_and_minus_one_resolves_both_ways(monkeypatch):
    off = R.check_ada()
    assert off == R.DAda(1.0, 0.0, 4, 500.0) and not off.active and not off.adaptive and off.describe() == "off"
    assert R.check_ada(-1, 0.6) == R.DAda(0.0, 0.6, 4, 500.0) and R.check_ada(-1, 0.6).adaptive
    assert R.check_ada(-1, 0.0).p == 1.0 and R.check_ada(0.25).active and not R.check_ada(0.25).adaptive
    assert R.check_ada(1.0) == off and R.check_ada(0.3, 0.6, 1, 2.5) == R.DAda(0.3, 0.6, 1, 2.5)
    assert R.check_ada(R.DAda(0.5, 0.0, 4, 500.0)) == R.DAda(0.5, 0.0, 4, 500.0)
    assert "fixed p = 0.5" in R.check_ada(0.5).describe() and "target r_t = 0.6" in R.check_ada(-1, 0.6).describe()
    for kw, flag in ((dict(p=-0.5), "d_augment_p"), (dict(p=1.5), "d_augment_p"), (dict(p=float("nan")), "d_augment_p"),
                     (dict(target=1.0), "ada_target"), (dict(target=-0.1), "ada_target"),
                     (dict(interval=0), "ada_interval"), (dict(interval=(1 << 16) + 1), "ada_interval"),
                     (dict(interval=2.5), "ada_interval"), (dict(kimg=0.0), "ada_kimg"), (dict(kimg=float("inf")), "ada_kimg"),
                     (dict(p="x"), "d_augment_p")):
        with pytest.raises(ValueError, match=flag):
            R.check_ada(**kw)
    with pytest.raises(ValueError, match="below 2\\^31"):
        R.check_ada(0.5, interval=1 << 16, batch_size=1 << 15)
    R.check_ada(0.5, interval=1 << 16, batch_size=(1 << 15) - 1)
    # a gate or the controller with no policy to gate: an error; off never is
    for kw in (dict(p=0.5), dict(target=0.6)):
        with pytest.raises(ValueError, match="need a policy to gate"):
            R.check_ada(augmented=False, **kw)
        R.check_ada(augmented=True, **kw)
    R.check_ada(augmented=False)
    # the environment, and the arguments beating it
    monkeypatch.setenv("DCGAN_D_AUGMENT_P", "0.25")
    monkeypatch.setenv("DCGAN_ADA_TARGET", "0.7")
    monkeypatch.setenv("DCGAN_ADA_INTERVAL", "8")
    monkeypatch.setenv("DCGAN_ADA_KIMG", "20")
    assert R.resolve_ada() == R.DAda(0.25, 0.7, 8, 20.0)
    assert R.resolve_ada(0.5, 0.0, 2, 3.0) == R.DAda(0.5, 0.0, 2, 3.0) and R.resolve_ada(-1, 0.0) == R.DAda(1.0, 0.0, 8, 20.0)
    assert _hip(small(), **ON).ada == R.DAda(0.25, 0.7, 8, 20.0)
    assert _hip(small(), d_augment_p=1.0, ada_target=0.0, **ON).ada.active is False
    assert ReferenceEngine(small(), 4, CPU, **ON).ada == R.DAda(0.25, 0.7, 8, 20.0)
    with pytest.raises(ValueError, match="need a policy to gate"):
        _hip(small())
    with pytest.raises(ValueError, match="need a policy to gate"):
        ReferenceEngine(small(), 4, CPU)
    monkeypatch.setenv("DCGAN_ADA_INTERVAL", "x")
    with pytest.raises(ValueError, match="DCGAN_ADA_INTERVAL"):
        R.resolve_ada()


def test_every_entry_point_rejects_a_gate_without_a_policy(capsys):
    for kw in (dict(d_augment_p=0.5), dict(ada_target=0.6)):
        with pytest.raises(ValueError, match="need a policy to gate"):
            _hip(small(), **kw)
        with pytest.raises(ValueError, match="need a policy to gate"):
            ReferenceEngine(small(), 4, CPU, **kw)
        with pytest.raises(ValueError, match="need a policy to gate"):
            build_engine(small(), 4, CPU, engine="reference", **kw)
    with pytest.raises(ValueError, match="need a policy to gate"):
        ReferenceStep(DCGAN(small(), seed=1), d_ada=R.DAda(0.5, 0.0, 4, 500.0))
    for argv in (["--d_augment_p=0.5"], ["--ada_target=0.6"], ["--d_augment=cutout", "--ada_target=1.0"],
                 ["--d_augment=cutout", "--d_augment_p=2"], ["--d_augment=cutout", "--ada_target=0.6", "--ada_interval=0"],
                 ["--d_augment=cutout", "--ada_target=0.6", "--ada_kimg=0"]):
        with pytest.raises(SystemExit):
            F.parse_flags(argv)
        assert "--d_augment_p / --ada_target" in capsys.readouterr().err
    fl = F.parse_flags([])
    assert (fl.d_augment_p, fl.ada_target, fl.ada_interval, fl.ada_kimg) == (-1.0, 0.0, 4, 500.0)
    fl = F.parse_flags(["--d_color_augment=contrast", "--ada_target=0.6", "--ada_interval=2", "--ada_kimg=1.5", "--d_augment_p=0.1"])
    assert (fl.d_augment_p, fl.ada_target, fl.ada_interval, fl.ada_kimg) == (0.1, 0.6, 2, 1.5)
    # the bindings: a state without a gate buffer, a drawing launch without the state, aliased buffers
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    x, y, p, st, g, a = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
    for op in (prog.d_augment, prog.d_color):
        with pytest.raises(RuntimeError, match="without a gates buffer"):
            op("a", x, y, p, 2, 8, 3, 3, 5, st, 0, 0, a)
        with pytest.raises(RuntimeError, match="need ada_state"):
            op("a", x, y, p, 2, 8, 3, 3, 5, st, 0, g, 0)
        for alias in (x, y, p):
            with pytest.raises(RuntimeError, match="gates must be a buffer of its own"):
                op("a", x, y, p, 2, 8, 3, 3, 5, st, 0, alias, a)
        with pytest.raises(RuntimeError, match="ada_state must be a buffer of its own"):
            op("a", x, y, p, 2, 8, 3, 3, 5, st, 0, g, g + 4)
    for op in (prog.d_augment_bwd, prog.d_color_bwd):
        with pytest.raises(RuntimeError, match="gates must be a buffer of its own"):
            op("a", x, y, p, 2, 8, 3, 3, 0, y + 8)
    lg = 7 << 20
    for bad in (dict(logits=0), dict(state=0), dict(B=0), dict(interval=0), dict(interval=(1 << 16) + 1), dict(delta24=0),
                dict(delta24=ONE + 1), dict(target_n=17), dict(target_n=-17), dict(thr=float("nan")),
                dict(B=1 << 20, interval=1 << 12), dict(state=lg + 4)):
        kw = dict(dict(logits=lg, B=8, state=a, thr=0.0, target_n=10, delta24=5, interval=2), **bad)
        with pytest.raises(RuntimeError, match="ada_update"):
            prog.ada_update("u", **kw)
    assert prog.size() == 0


def test_bindings_record_the_byte_ranges():
    from distributed_tensorflow_for_dcgan_amd.ops import hip as H
    prog = H.ext().Program(0, True)
    x, y, p, st, g, a, lg = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 7 << 20
    nb = 2 * 8 * 8 * 3 * 2
    base = [(x, nb, False), (y, nb, True)]
    for k, (fwd, bwd) in enumerate(((prog.d_augment, prog.d_augment_bwd), (prog.d_color, prog.d_color_bwd))):
        i = prog.size()
        fwd("f", x, y, p, 2, 8, 3, 3, 5, st, 0, g, a)            # gated, drawing
        fwd("p", x, y, p, 2, 8, 3, 3, 0, 0, 0, gates=g)         # gated probe
        bwd("b", x, y, p, 2, 8, 3, 3, 0, gates=g + 4)           # gated transpose over later rows
        fwd("u", x, y, p, 2, 8, 3, 3, 5, st, 0)                 # ungated: today's ranges
        bwd("v", x, y, p, 2, 8, 3, 3, 0)
        probe_p = [(p, 32, False)] + ([(p, 32, True)] if k else [])
        assert sorted(prog.op_info(i)[4]) == sorted(base + [(st, 8, False), (p, 32, True), (a, 4, False), (g, 8, True)])
        assert sorted(prog.op_info(i + 1)[4]) == sorted(base + probe_p + [(g, 8, False)])
        assert sorted(prog.op_info(i + 2)[4]) == sorted(base + [(p, 32, False), (g + 4, 8, False)])
        assert sorted(prog.op_info(i + 3)[4]) == sorted(base + [(st, 8, False), (p, 32, True)])
        assert sorted(prog.op_info(i + 4)[4]) == sorted(base + [(p, 32, False)])
    i = prog.size()
    prog.ada_update("ada_update", lg, 8, a, 0.5, 10, 5, 2)
    assert sorted(prog.op_info(i)[4]) == sorted([(lg, 32, False), (a, 32, False), (a, 32, True)])
    for dt in (1, 2):  # every build has the entries
        q = H.ext().Program(dt, True)
        q.d_color("f", x, y, p, 2, 8, 3, 7, 5, st, 0, g, a)
        q.ada_update("u", lg, 300, a, 0.0, -4, ONE, 1)
        assert q.size() == 2


# ------------------------------------------------------------------ 5. ReferenceStep / ReferenceEngine
def test_reference_step_with_fixed_p_equals_autograd_on_the_gated_input():
    cfg, B = small(), 4
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    ada = R.check_ada(0.5)
    st = ReferenceStep(DCGAN(cfg, seed=3), d_ada=ada, noise_seed=SEED, d_steps=2, **ON)
    assert st.ada == ada and st.ada_state == R.ada_state(ONE // 2)
    st.global_step = 2
    seen = {}
    orig = st.model.discriminator

    def spy(x, **k):
        seen["x"] = x.detach().clone()
        return orig(x, **k)
    st.model.discriminator = spy
    out = st.forward_losses(real, z, update_ema=False)
    both = torch.cat([real, out["fake"].detach()], 0)
    cg, ag = R.gate_masks(2 * B, SEED, 2, 5, ONE // 2, 7), R.gate_masks(2 * B, SEED, 2, 4, ONE // 2, 3)
    assert all(torch.equal(a, b) for a, b in zip(st.draw_gates(2 * B), (cg, ag)))
    cp, ap = R.color_params(2 * B, SEED, 2), R.augment_params(2 * B, 28, SEED, 2)
    want = R.augment(R.color_augment(both, cp, COL, gates=cg), ap, AUG, gates=ag)
    assert torch.equal(seen["x"], want) and not torch.equal(want, R.augment(R.color_augment(both, cp, COL), ap, AUG))
    sub = st.draw_gates(2 * B, 0)  # a sub-step gates with its own seed and the same p24
    assert torch.equal(sub[0], R.gate_masks(2 * B, R.substep_seed(SEED, 0), 2, 5, ONE // 2, 7)) and not torch.equal(sub[0], cg)
    st.forward_losses(real, z, update_ema=False, gates=False)
    assert torch.equal(seen["x"], R.augment(R.color_augment(both, cp, COL), ap, AUG))
    # the step's gradients == autograd by hand through the gated augmentation
    st.model.discriminator = orig
    o, fd, fg = st.compute_grads(real, z, update_ema=False)
    o1, fd1, fg1 = st.compute_grads(real, z, update_ema=False, gates=(cg, ag), color=cp, augment=ap)
    assert torch.equal(fd, fd1) and torch.equal(fg, fg1)
    m = st.model
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in m.g.tensors.items()}
    fake = m.generator(z, train=True, P=Pg, update_ema=False)
    x = R.augment(R.color_augment(torch.cat([real, fake], 0), cp, COL, gates=cg), ap, AUG, gates=ag)
    _, logits = m.discriminator(x, groups=2, slots=(0, 1), train=True, update_ema=False)
    g_loss = R.gan_losses(logits[:B], logits[B:])[2]
    gg = torch.autograd.grad(g_loss, [Pg[n] for n in m.g.names()], allow_unused=True)
    ref = m.g.like()
    for n, t in zip(m.g.names(), gg):
        if t is not None:
            ref[n].copy_(t)
    assert torch.allclose(fg, ref.flat, rtol=1e-5, atol=1e-7) and float(fg.abs().max()) > 0
    # a fixed p never moves; p = 1 and no target is today's step, bitwise
    st.step(real, z)
    assert st.ada_state == R.ada_state(ONE // 2)
    a, b = ReferenceStep(DCGAN(cfg, seed=3), d_ada=R.check_ada(), **ON), ReferenceStep(DCGAN(cfg, seed=3), **ON)
    for _ in range(2):
        assert a.step(real, z) == b.step(real, z)
    assert torch.equal(a.model.d.flat, b.model.d.flat) and torch.equal(a.model.g.flat, b.model.g.flat)


def test_reference_step_carries_the_state_machine_from_its_own_logits():
    cfg, B = small(), 4
    real, z = _real(B, cfg, 1), _z(B, cfg, 2)
    ada = R.check_ada(-1, 0.6, 2, 0.01)
    st = ReferenceStep(DCGAN(cfg, seed=3), d_ada=ada, noise_seed=SEED, d_steps=2, world=2, **ON)
    d24, Tn = R.ada_delta24(2, B, 2, 0.01), R.ada_target_n(0.6, B, 2)
    assert st.ada_state == R.ada_state(0) and d24 > 1000 and Tn == 5
    want = R.ada_state(0)
    for t in range(5):
        st.d_step(real, z)
        assert st.ada_state == want  # the sub-step leaves the state alone
        st.step(real, z)
        want = R.ada_update(want, st.last["logits_real"].detach(), 0.0, Tn, d24, 2)
        assert st.ada_state == want and want[2] == (t + 1) % 2 and want[4] == (t + 1) // 2
    assert want[0] != 0 or want[3] <= Tn  # p moved unless every window fell at or below the target
    eng = ReferenceEngine(cfg, B, CPU, seed=3, ada_target=0.6, ada_interval=2, ada_kimg=0.01, **ON)
    eng.set_synthetic_batch(real)
    for _ in range(2):
        eng.train_step()
    s = eng.ada_status()
    assert s["windows"] == 1 and s["cnt"] == 0 and s["p"] == s["p24"] / ONE and s["r_t"] == s["r_acc"] / (B * 2)
    assert ReferenceEngine(cfg, B, CPU, **ON).ada_status() is None


# ------------------------------------------------------------------ 6. checkpoints
def test_checkpoint_round_trip_is_exact_and_missing_keys_start_from_the_initial_p(tmp_path):
    cfg, B = small(), 4
    kw = dict(seed=3, ada_target=0.6, ada_interval=4, ada_kimg=0.01, d_augment_p=0.25, **ON)
    eng = ReferenceEngine(cfg, B, CPU, **kw)
    eng.set_synthetic_batch(_real(B, cfg, 1))
    for _ in range(6):  # one finished window and two steps into the next
        eng.train_step()
    state = list(eng.step_impl.ada_state)
    assert state[2] == 2 and state[4] == 1
    sd = CK.collect_state(eng)
    keys = ["ada/" + k for k in R.ADA_KEYS]
    assert [k for k in sd if k.startswith("ada/")] == keys
    assert all(sd[k].dtype == np.int32 and sd[k].shape == () for k in keys)
    assert [int(sd[k]) for k in keys] == state[:5]
    mgr = CK.CheckpointManager(str(tmp_path / "ck"))
    mgr.save(eng)
    other = ReferenceEngine(cfg, B, CPU, **dict(kw, seed=9))
    info = mgr.restore_latest(other)
    assert other.step_impl.ada_state == state and info["ada"].startswith("loaded")
    other.set_synthetic_batch(_real(B, cfg, 1))
    eng.train_step()
    other.train_step()
    assert other.step_impl.ada_state == eng.step_impl.ada_state
    # a fixed p and the switch off write no key; loading such a checkpoint starts from the initial p, and says so
    for off_kw in (dict(seed=3, d_augment_p=0.5, **ON), dict(seed=3, **ON), dict(seed=3)):
        off = ReferenceEngine(cfg, B, CPU, **off_kw)
        assert not any(k.startswith("ada/") for k in CK.collect_state(off))
    mgr2 = CK.CheckpointManager(str(tmp_path / "ck2"))
    mgr2.save(ReferenceEngine(cfg, B, CPU, seed=3, **ON))
    other.step_impl.ada_state = [5, 4, 3, 2, 1, 0, 0, 0]
    info = mgr2.restore_latest(other)
    assert other.step_impl.ada_state == R.ada_state(R.ada_p24(0.25)) and "starts from p = 0.25" in info["ada"]
    plain = ReferenceEngine(cfg, B, CPU, seed=3, **ON)
    assert "ada" not in mgr.restore_latest(plain)  # keys a run without the controller ignores
    # resumed under a shorter interval than the window the checkpoint is in (cnt = 2): cnt == interval could never
    # fire again, so the open window is dropped and p, r_acc and the window count are kept
    assert CK.ADA_KEYS is R.ADA_KEYS
    short = ReferenceEngine(cfg, B, CPU, **dict(kw, ada_interval=2))
    info = mgr.restore_latest(short)
    assert short.step_impl.ada_state == [state[0], 0, 0, state[3], state[4], 0, 0, 0] and "is dropped" in info["ada"]
    short.set_synthetic_batch(_real(B, cfg, 1))
    for _ in range(2):
        short.train_step()
    assert short.step_impl.ada_state[4] == state[4] + 1 and short.step_impl.ada_state[2] == 0
    same = ReferenceEngine(cfg, B, CPU, **dict(kw, ada_interval=3))  # cnt = 2 < 3 still fits: kept as it is
    assert "dropped" not in mgr.restore_latest(same)["ada"] and same.step_impl.ada_state[:5] == state[:5]


# ------------------------------------------------------------------ 7. schedules (dry-run HIP engines)
def _check_ada_ops(eng, d_steps, adaptive):
    """Every d_color / d_aug is gated: reads the 4 bytes of p24 and writes its gate buffer; the two
    transposes read the fake half's gate rows; one ada_update per full step on the D chain's stream behind the
    head launch (the fused step: behind the chain; the DDP schedules: ahead of it), reading logits[:B] and reading
    and writing the 32 bytes of state."""
    ex = _record(eng, steps=2)
    B = eng.B
    names = [_name(o) for o in ex.ops]
    p24 = (eng.ada_state.data_ptr(), 4, False)
    for nm, gates in (("d_color", eng.color_gates), ("d_aug", eng.aug_gates)):
        ops = [o for o in ex.ops if _name(o) == nm]
        assert len(ops) == 2 * d_steps
        for o in ops:
            assert p24 in o.acc and (gates.data_ptr(), 8 * B, True) in o.acc and o.stream == "main"
        bwd = [o for o in ex.ops if _name(o) == nm + "_bwd"]
        assert len(bwd) == 2 and all((gates.data_ptr() + 4 * B, 4 * B, False) in o.acc for o in bwd)
        assert not any(a == eng.ada_state.data_ptr() for o in bwd for a, _, _ in o.acc)  # no p24, no counter
        assert not any(a == eng.step_counter.data_ptr() for o in bwd for a, _, _ in o.acc)
    upd = [i for i, n in enumerate(names) if n == "ada_update"]
    assert len(upd) == (2 if adaptive else 0)
    assert "ada_update" not in [n for k in range(d_steps - 1) for n in eng.sub_op_names(k)]
    for i in upd:
        o = ex.ops[i]
        assert sorted(o.acc) == sorted([(eng.logits.data_ptr(), 4 * B, False), (eng.ada_state.data_ptr(), 32, False),
                                        (eng.ada_state.data_ptr(), 32, True)])
        head = max(j for j in range(i) if names[j].startswith("d_head") and "loss" in names[j])
        assert any(a == eng.logits.data_ptr() and w for a, _, w in ex.ops[head].acc)
        if eng._schedule() == "fused":  # behind the D chain's last op on its stream, ahead of the update
            assert o.stream == "alt0" and eng._ada_at_tail()
            prev = [j for j in range(head + 1, i) if ex.ops[j].stream == "alt0"]
            assert names[prev[0]].startswith("d_head.bwd") and names[prev[-1]] == eng.progB.name(eng.progB.size() - 1)
            assert not any(n.startswith(("adam", "ls.check", "step_end")) for n in names[head:i])
            continue
        nxt = [j for j in range(i + 1, len(names)) if ex.ops[j].stream == o.stream]
        assert names[nxt[0]].startswith("d_head.bwd")  # the D chain's first op follows it on its stream
        if eng._schedule() != "serial":
            assert o.stream == "alt0"
            assert [j for j in range(head + 1, i) if ex.ops[j].stream == "alt0"] == []


@pytest.mark.parametrize("mode", [FIXED, ADAPT], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("world,schedule,wire,d_steps", TC.CASES,
                         ids=["W%d-%s-%s-d%d" % (w, s or "default", a, d) for w, s, a, d in TC.CASES])
def test_schedules_are_hazard_free_with_the_gates_and_the_controller(world, schedule, wire, d_steps, mode):
    eng = _hip(world=world, schedule=schedule, allreduce_dtype=wire, d_steps=d_steps, **mode)
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_ada_ops(eng, d_steps, eng.ada.adaptive)


@pytest.mark.parametrize("extra", [dict(d_augment=""), dict(d_color_augment=""), TC.NOISE, dict(g_topk=0.5, g_topk_steps=10),
                                   dict(dtype="fp16", graph=False), dict(dtype="fp32"), dict(d_spectral_norm=True, d_steps=2),
                                   dict(gan_loss="lsgan", label_smooth=0.1)],
                         ids=["color-only", "geo-only", "noise", "topk", "fp16", "fp32", "sn-d2", "lsgan"])
def test_other_configurations_are_hazard_free(extra):
    for world, timing in ((1, False), (1, True), (2, False)):
        eng = _hip(small(), world=world, **dict(ADAPT, **extra))
        if timing:
            eng._timing = True
            eng._build_updates()
        hz, _ = SC.check_engine(eng)
        assert hz == [], "\n".join(map(str, hz[:10]))
        assert (eng.aug_gates is None) == (not eng.aug.active) and (eng.color_gates is None) == (not eng.color.active)
        ex = _record(eng)
        upd = [o for o in ex.ops if _name(o) == "ada_update"]
        assert len(upd) == 1
    lsgan = _hip(small(), gan_loss="lsgan", label_smooth=0.1, **ADAPT)
    assert lsgan.progAda.size() == 1 and lsgan.progAda.name(0) == "ada_update"


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_update_is_hazard_free(world, monkeypatch):
    monkeypatch.setenv("DCGAN_DDP_SHARD", "1")
    eng = _hip(world=world, **ADAPT)
    assert eng._sharded()
    hz, n = SC.check_engine(eng)
    assert n > 100 and hz == [], "\n".join(map(str, hz[:10]))
    _check_ada_ops(eng, 1, True)


def test_the_fused_step_takes_the_head_of_the_d_chain_on_request(monkeypatch):
    monkeypatch.setenv("DCGAN_ADA_PLACE", "head")
    for d_steps in (1, 2):
        eng = _hip(d_steps=d_steps, **ADAPT)
        assert not eng._ada_at_tail() and SC.check_engine(eng)[0] == []
        ex = _record(eng)
        names = [_name(o) for o in ex.ops]
        i = names.index("ada_update")
        nxt = [j for j in range(i + 1, len(names)) if ex.ops[j].stream == "alt0"]
        assert ex.ops[i].stream == "alt0" and names[nxt[0]].startswith("d_head.bwd")


def test_checker_finds_ada_update_moved_ahead_of_a_gated_forward():
    """ada_update of step 0 on a stream nothing waits for: its write of p24 races step 0's gated forwards
    (issued before it) and step 1's (issued after it). Only the accesses to the state are kept."""
    eng = _hip(**ADAPT)
    assert SC.check_engine(eng)[0] == []
    ex = _record(eng, steps=2)
    names = [_name(o) for o in ex.ops]
    i = names.index("ada_update")
    j = names.index("d_color")
    assert j < i
    op = ex.ops.pop(i)
    op.stream = "planted"
    op.vc = {"planted": 1}
    ex.ops.insert(j, op)
    lo, hi = eng.ada_state.data_ptr(), eng.ada_state.data_ptr() + 32
    for o in ex.ops:
        o.acc = [a for a in o.acc if lo <= a[0] < hi]
    hz = SC.find_hazards(ex.ops)
    pairs = {(h.a.split("@")[0], h.b.split("@")[0]) for h in hz}
    for other in ("step0:d_color", "step0:d_aug", "step1:d_color", "step1:d_aug"):
        assert any({"step0:ada_update", other} == set(p) for p in pairs), (other, pairs)
    assert any({"step0:ada_update", "step1:ada_update"} == set(p) for p in pairs)


def test_with_the_switch_off_the_recorded_ops_are_todays():
    for kw in (dict(), dict(d_steps=2), dict(world=2), dict(world=2, schedule="ddp"), dict(dtype="fp16"), dict(dtype="fp32")):
        off, bare = _hip(d_augment_p=-1.0, ada_target=0.0, **ON, **kw), _hip(**ON, **kw)
        for e in (off, bare):
            assert not e.ada.active and e.ada_state is None and e.aug_gates is None and e.color_gates is None
            assert e.progAda is None and e.ada_status() is None
        assert off.op_names() == bare.op_names() and "ada_update" not in bare.op_names()
        a, b = _record(off), _record(bare)
        assert [(_name(x), x.stream, len(x.acc)) for x in a.ops] == [(_name(x), x.stream, len(x.acc)) for x in b.ops]
        fixed, adapt = _hip(**FIXED, **kw), _hip(**ADAPT, **kw)
        assert fixed.op_names() == bare.op_names() and fixed.progAda is None and fixed.ada_state is not None
        assert [n for n in adapt.op_names() if n != "ada_update"] == bare.op_names()
        assert adapt.op_names().count("ada_update") == 1 and adapt.kernel_count() == bare.kernel_count() + 1
        c = _record(adapt)
        assert [_name(x) for x in c.ops if _name(x) != "ada_update"] == [_name(x) for x in b.ops]  # one more launch
        assert len(c.ops) == len(b.ops) + 1
        for x, y in zip(_record(fixed).ops, b.ops):  # gated: two more ranges in each forward, one in each transpose
            extra = {"d_color": 2, "d_aug": 2, "d_color_bwd": 1, "d_aug_bwd": 1}.get(_name(x), 0)
            assert len(x.acc) == len(y.acc) + extra and x.stream == y.stream


# ------------------------------------------------------------------ 8. trainer / CLI
def test_cli_runs_with_the_controller_and_writes_the_two_scalars(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") + ENV:
        env.pop(k, None)
    args = ["--synthetic", "--engine", "reference", "--max_steps=4", "--device=cpu", "--output_size=28", "--c_dim=1",
            "--batch_size=4", "--sample_every=0", "--save_summaries_secs=0", "--epoch=0", "--d_color_augment=contrast",
            "--d_augment=cutout", "--ada_target=0.6", "--ada_interval=2", "--ada_kimg=0.01",
            "--checkpoint_dir=%s" % (tmp_path / "ck"), "--sample_dir=%s" % (tmp_path / "s")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args, env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "augmentation probability of D's inputs: adaptive p from 0, target r_t = 0.6, every 2 steps" in p.stdout
    blob = b"".join(open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(str(tmp_path)) for f in fs if "tfevents" in f)
    assert b"ada/p" in blob and b"ada/r_t" in blob
    # resumed: the state is found
    p = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py")] + args[:4] + ["--max_steps=5"] + args[5:],
                       env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "adaptive augmentation state: loaded" in p.stdout, p.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "image_train.py"), "--ada_target=0.6"], env=env,
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert bad.returncode != 0 and "need a policy to gate" in bad.stdout


def test_trainer_prints_nothing_with_the_switch_off(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32", "--max_steps=1",
                        "--epoch=0", "--d_augment=cutout", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    assert "augmentation probability" not in out.getvalue() and "adaptive augmentation" not in out.getvalue()
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=28", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--nosummaries", "--train_size=32", "--max_steps=1",
                        "--epoch=0", "--d_augment=cutout", "--d_augment_p=0.25", "--checkpoint_dir=%s" % (tmp_path / "ck2"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    assert "augmentation probability of D's inputs: fixed p = 0.25" in out.getvalue()
