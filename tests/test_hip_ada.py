"""GPU tests of the adaptive augmentation probability (ADA) of D's augmentations: the gated instances of
``d_augment_kernel`` / ``d_color_kernel`` against the gated oracles (every build, the 16-byte and the
element paths, canaries around every output, params and gate buffer), ``ada_update_kernel`` against
``ops.reference.ada_update``, and the engine: gated buffers and gate rows per step and sub-step, steps
against ``ReferenceStep`` with the oracle's draws and gates passed in (the comparison and tolerances of
test_hip_d_steps.py, as test_hip_d_color.py uses them), the controller's state after each of 9 steps, graph
replay on the live state, an fp16 overflow step, the switch off, clean sample-time losses, one-rank RCCL
DDP and a resume through the trainer in the middle of a window.

Color inputs are the exact-sum ones of test_hip_d_color.py (bitwise, the mean included); on general inputs
the forward is compared at the recorded Mx, as there."""
import io
import itertools
import os

import pytest
import torch
import torch.multiprocessing as mp

import test_ada as TA
import test_hip_d_color as HC
import test_hip_d_spectral_norm as SNT
import test_hip_d_steps as TD
from distributed_tensorflow_for_dcgan_amd.models.config import DCGANConfig
from distributed_tensorflow_for_dcgan_amd.ops import reference as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
BUILDS = SNT.BUILDS
PAD = SNT.PAD
ENV = HC.ENV + TA.ADA_ENV
ONE = 1 << 24
P24S = [0, 1, 1 << 23, ONE - 1, ONE]
N = 5
KSHAPES = [(S, C) for S in (8, 9, 16) for C in (1, 3)]  # S = 9: the element paths; 8, 16: the 16-byte paths
SEED, T = 0xFEDCBA9876543210, (1 << 32) + 3
AUG, COL = TA.AUG, TA.COL
ON = TA.ON
FIXED = TA.FIXED
_slot, _intact, _same_bits, _exact = HC._slot, HC._intact, HC._same_bits, HC._exact


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def H():
    from distributed_tensorflow_for_dcgan_amd.ops import hip
    return hip


def small():
    return DCGANConfig(output_size=28, c_dim=1)


def _islot(n, fill=-3):
    """int32 [n] between PAD canaries: (buffer, view)."""
    buf = torch.full((n + 2 * PAD,), fill, dtype=torch.int32, device=dev)
    return buf, buf[PAD:PAD + n]


def _iintact(buf, fill=-3):
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


# ------------------------------------------------------------------ 1. the gates
def test_gate_mask_probes_equal_the_oracle():
    h = H()
    for p24 in P24S:
        for seed, t in ((SEED, T), (1000020, 0), (1000020, 1)):
            for stream, full in ((4, 3), (5, 7)):
                got = h.gate_masks(64, seed, t, stream, p24, full)
                assert got.dtype == torch.int32 and torch.equal(got.cpu(), R.gate_masks(64, seed, t, stream, p24, full))
        assert torch.equal(h.gate_masks(64, SEED, T, 5, p24, 5).cpu(), R.gate_masks(64, SEED, T, 5, p24, 5))
        assert torch.equal(h.gate_masks(64, SEED, T, 4, p24, 2).cpu(), R.gate_masks(64, SEED, T, 4, p24, 2))
    # a device state and a device counter
    state = torch.tensor([1 << 23, 9, 9, 9, 9, 0, 0, 0], dtype=torch.int32, device=dev)
    step = torch.tensor([7], dtype=torch.int64, device=dev)
    assert torch.equal(h.gate_masks(4096, SEED, step, 5, state, 7).cpu(), R.gate_masks(4096, SEED, 7, 5, 1 << 23, 7))
    assert state.tolist() == [1 << 23, 9, 9, 9, 9, 0, 0, 0]  # only read
    with pytest.raises(ValueError):
        h.gate_masks(4, SEED, 0, 3, 0, 7)
    with pytest.raises(ValueError):
        h.gate_masks(4, SEED, 0, 4, ONE + 1, 3)


# ------------------------------------------------------------------ 2. the gated kernels
@pytest.mark.parametrize("S,C", KSHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("build", list(BUILDS))
def test_gated_kernels_are_bitwise_the_gated_oracle(build, S, C):
    h = H()
    dtype = BUILDS[build]
    full = (N, S, S, C)
    x0, g0 = _exact(N, S, C, 7).to(dtype), _exact(N, S, C, 8).to(dtype)
    xb, x = _slot(full, dtype)
    x.copy_(x0)
    gb, g = _slot(full, dtype)
    g.copy_(g0)
    ap, cp = R.augment_params(N, S, SEED, T), R.color_params(N, SEED, T)
    Mx = R.color_mean(x0.float())
    seen = set()
    for p24 in P24S:
        # ---- translation / cutout
        for aug in (AUG, R.DAugment(True, False), R.DAugment(False, True)):
            gates = R.gate_masks(N, SEED, T, 4, p24, aug.mask)
            seen.update(gates.tolist())
            yb, y = _slot(full, dtype)
            pb, p = _islot(4 * N)
            qb, q = _islot(N)
            out, pout, gout = h.augment_draw(x, SEED, T, aug, out=y, params_out=p.view(N, 4), p24=p24, gates_out=q)
            assert out.data_ptr() == y.data_ptr() and gout.data_ptr() == q.data_ptr()
            assert torch.equal(q.cpu(), gates) and torch.equal(p.view(N, 4).cpu().long(), ap)  # all four drawn whatever the gates
            assert _same_bits(y, R.augment(x0, ap, aug, gates=gates)), (p24, aug)
            assert _intact(yb) and _iintact(pb) and _iintact(qb)
            y2b, y2 = _slot(full, dtype)  # the probe and the transpose under the recorded rows
            h.augment_apply(x, ap, aug, out=y2, gates=q)
            assert _same_bits(y2, y) and _intact(y2b)
            tb, tg = _slot(full, dtype)
            h.augment_apply(g, ap, aug, transpose=True, out=tg, gates=q)
            assert _same_bits(tg, R.augment_transpose(g0, ap, aug, gates=gates)) and _intact(tb)
            if p24 == ONE:  # bitwise the ungated launch, params included
                y3, p3 = h.augment_draw(x, SEED, T, aug)
                assert _same_bits(y3, y) and torch.equal(p3, p.view(N, 4)) and bool((q == aug.mask).all())
                assert _same_bits(h.augment_apply(g, ap, aug, transpose=True), tg)
            if p24 == 0:  # a bitwise copy
                assert _same_bits(y, x0) and _same_bits(tg, g0) and not bool(q.any())
        # ---- color
        for color in HC.SUBSETS:
            gates = R.gate_masks(N, SEED, T, 5, p24, color.mask)
            yb, y = _slot(full, dtype)
            pb = torch.full((4 * N + 2 * PAD,), -3.0, dtype=torch.float32, device=dev)
            p = pb[PAD:PAD + 4 * N].view(N, 4)
            qb, q = _islot(N)
            h.color_draw(x, SEED, T, color, out=y, params_out=p, p24=p24, gates_out=q)
            assert torch.equal(q.cpu(), gates) and torch.equal(p[:, :3].cpu(), cp)
            con = ((gates >> 2) & 1).bool()
            assert torch.equal(p[:, 3].cpu(), torch.where(con, Mx, torch.zeros(N))), (p24, color)  # gated off: Mx = 0
            assert _same_bits(y, R.color_augment(x0, cp, color, gates=gates)), (p24, color)
            assert _intact(yb) and bool((pb[:PAD] == -3).all()) and bool((pb[-PAD:] == -3).all()) and _iintact(qb)
            y2b, y2 = _slot(full, dtype)
            p2 = torch.full((N, 4), -3.0, device=dev)
            h.color_apply(x, cp, color, out=y2, params_out=p2, gates=q)
            assert _same_bits(y2, y) and torch.equal(p2, p) and _intact(y2b)
            tb, tg = _slot(full, dtype)
            h.color_apply(g, cp, color, transpose=True, out=tg, gates=q)
            assert _same_bits(tg, R.color_augment_transpose(g0, cp, color, gates=gates)) and _intact(tb)
            if p24 == ONE:
                y3, p3 = h.color_draw(x, SEED, T, color)
                assert _same_bits(y3, y) and torch.equal(p3, p) and bool((q == color.mask).all())
                assert _same_bits(h.color_apply(g, cp, color, transpose=True), tg)
            if p24 == 0:
                assert _same_bits(y, x0) and _same_bits(tg, g0) and not bool(q.any()) and not bool(p[:, 3].any())
    assert seen == {0, 1, 2, 3}  # the five p24 reach every geometric pattern
    assert _same_bits(x, x0) and _intact(xb) and _same_bits(g, g0) and _intact(gb)  # only read


@pytest.mark.parametrize("build", list(BUILDS))
def test_general_inputs_forward_is_bitwise_at_the_recorded_mean(build):
    """As tests/test_hip_d_color.py: the recorded Mx within Higham's bound where contrast is on, the forward
    bitwise the gated oracle at it; mixed gates from the recorded rows."""
    h = H()
    dtype = BUILDS[build]
    for S, C in ((9, 3), (16, 3), (28, 1)):
        x0 = torch.tanh(torch.randn(N, S, S, C, generator=torch.Generator().manual_seed(12))).to(dtype)
        y, p, q = h.color_draw(x0.to(dev), SEED, 3, COL, p24=1 << 23)
        p, q = p.cpu(), q.cpu()
        assert torch.equal(q, R.gate_masks(N, SEED, 3, 5, 1 << 23, 7)) and torch.equal(p[:, :3], R.color_params(N, SEED, 3))
        con = ((q >> 2) & 1).bool()
        x64 = x0.double()
        dM = (p[:, 3].double() - x64.reshape(N, -1).mean(1)).abs()
        assert bool((dM[con] <= HC._mean_bound(x64)[con]).all()) and not bool(p[:, 3][~con].any())
        assert _same_bits(y, R.color_augment(x0, p, COL, gates=q).to(dev))


def test_a_garbage_gate_row_never_widens_the_policy():
    """The probe and the transposes AND the recorded row with the policy: bits outside it do nothing."""
    h = H()
    x0 = _exact(N, 9, 3, 3).to(torch.bfloat16)
    ap, cp = R.augment_params(N, 9, SEED, 1), R.color_params(N, SEED, 1)
    wild = torch.tensor([-1, 0x7FFFFFFF, 8, 0xF0, 3], dtype=torch.int32)
    for aug in (R.DAugment(True, False), R.DAugment(False, True)):
        assert _same_bits(h.augment_apply(x0.to(dev), ap, aug, gates=wild), R.augment(x0, ap, aug, gates=wild).to(dev))
        assert _same_bits(h.augment_apply(x0.to(dev), ap, aug, transpose=True, gates=wild),
                          R.augment_transpose(x0, ap, aug, gates=wild).to(dev))
    sat = R.DColor(False, True, False)
    assert _same_bits(h.color_apply(x0.to(dev), cp, sat, gates=wild), R.color_augment(x0, cp, sat, gates=wild).to(dev))


# ------------------------------------------------------------------ 3. the controller kernel
def test_ada_update_equals_the_oracle_over_the_table():
    h = H()
    for before, logits, thr, Tn, d24, iv, after in TA.TABLE:
        sb, st = _islot(8)
        st.copy_(torch.tensor(list(before) + [0, 0, 0], dtype=torch.int32))
        h.ada_update(st, torch.tensor(logits, device=dev), thr, Tn, d24, iv)
        assert tuple(st.tolist()[:5]) == after and st.tolist()[5:] == [0, 0, 0] and _iintact(sb), (before, logits)


@pytest.mark.parametrize("B", [1, 7, 256, 300])
def test_ada_update_tracks_the_oracle_over_windows(B):
    """Random logits with NaN and infinities mixed in, interval 1 and 4, a step size that reaches both clamps;
    lsgan's smoothed threshold; the logits a view into a longer buffer (the engine passes logits[:B])."""
    h = H()
    gen = torch.Generator().manual_seed(B)
    for iv, thr, target in ((1, 0.0, 0.6), (4, float(R.ada_threshold("lsgan", 0.1)), 0.5)):
        Tn, d24 = R.ada_target_n(target, B, iv), ONE // 3
        sb, st = _islot(8)
        st.copy_(torch.tensor(R.ada_state(ONE // 2), dtype=torch.int32))
        want = R.ada_state(ONE // 2)
        for t in range(12):
            both = torch.randn(2 * B, generator=gen) + (0.9 if (t // iv) % 3 else -0.9) + thr
            if B > 4:
                both[1], both[2], both[3] = float("nan"), float("inf"), float("-inf")
            both[B:] = 1e9  # the fake half must not count
            lg = both.to(dev)
            h.ada_update(st, lg[:B], thr, Tn, d24, iv)
            want = R.ada_update(want, both[:B], thr, Tn, d24, iv)
            assert st.tolist() == want and _iintact(sb), (iv, t)
        assert want[4] == 12 // iv


def test_bindings_reject_bad_calls_and_record_nothing():
    h = H()
    x = torch.zeros(2, 8, 8, 3, device=dev, dtype=torch.bfloat16)
    y = torch.full_like(x, 7.0)
    st = torch.zeros(8, dtype=torch.int32, device=dev)
    lg = torch.zeros(8, device=dev)
    with pytest.raises(TypeError):
        h.augment_draw(x, 1, 0, 3, out=y, p24=st[:4])
    with pytest.raises(TypeError):
        h.color_draw(x, 1, 0, 7, out=y, p24=st.long())
    with pytest.raises(ValueError):
        h.color_draw(x, 1, 0, 7, out=y, p24=-1)
    with pytest.raises(TypeError):
        h.augment_draw(x, 1, 0, 3, out=y, p24=0, gates_out=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        h.augment_apply(x, torch.zeros(2, 4, dtype=torch.int32), 3, out=y, gates=torch.zeros(2))
    with pytest.raises(TypeError):
        h.color_apply(x, torch.zeros(2, 3), 7, out=y, gates=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        h.ada_update(st.long(), lg, 0.0, 0, 1, 1)
    with pytest.raises(TypeError):
        h.ada_update(st, lg.double(), 0.0, 0, 1, 1)
    for bad in (dict(interval=0), dict(delta24=0), dict(delta24=ONE + 1), dict(target_n=9), dict(thr=float("nan"))):
        with pytest.raises(RuntimeError, match="ada_update"):
            h.ada_update(st, lg, **dict(dict(thr=0.0, target_n=0, delta24=1, interval=1), **bad))
    with pytest.raises(RuntimeError, match="ada_update"):
        h.ada_update(st, torch.zeros(0, device=dev), 0.0, 0, 1, 1)
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and not bool(st.any())


# ------------------------------------------------------------------ 4. the engine's buffers under a fixed p
def _check_gated(eng, d_in, k, t, tag):
    """Both recorded gate rows == the oracle's at (the piece's seed, step t, the live p24); the colored and
    the augmented copy == the gated oracles at the recorded params, bitwise."""
    B2 = 2 * eng.B
    p24 = int(eng.ada_state[0])
    cg, ag = eng.color_gates.cpu(), eng.aug_gates.cpu()
    assert torch.equal(cg, R.gate_masks(B2, eng._zseed(k), t, 5, p24, eng.color.mask)), tag
    assert torch.equal(ag, R.gate_masks(B2, eng._zseed(k), t, 4, p24, eng.aug.mask)), tag
    cp, ap = eng.color_params.cpu(), eng.aug_params.cpu().long()
    assert torch.equal(cp[:, :3], R.color_params(B2, eng._zseed(k), t)), tag
    assert torch.equal(ap, R.augment_params(B2, eng.cfg.output_size, eng._zseed(k), t)), tag
    assert not bool(cp[:, 3][((cg >> 2) & 1) == 0].any()), tag
    colored = R.color_augment(d_in.cpu(), cp, eng.color, gates=cg)
    assert _same_bits(eng.d_colored, colored.to(dev)), tag
    assert _same_bits(eng.d_auged, R.augment(colored, ap, eng.aug, gates=ag).to(dev)), tag
    return cg, ag


@pytest.mark.parametrize("dtype,size,c_dim", [("bf16", 28, 1), ("fp16", 28, 1), ("fp32", 28, 1), ("bf16", 64, 3)])
def test_engine_gated_buffers_and_gate_rows_are_the_oracles_and_z_is_untouched(dtype, size, c_dim):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    eng = TD._engine(cfg, 8, 2, dtype=dtype, seed=3, **FIXED)
    off = TD._engine(cfg, 8, 2, dtype=dtype, seed=3, **ON)
    assert eng.ada == R.DAda(0.5, 0.0, 4, 500.0) and eng.progAda is None and off.ada_state is None
    assert eng.ada_state.tolist() == R.ada_state(ONE // 2) and eng.op_names() == off.op_names()
    assert eng.color_gates.dtype == eng.aug_gates.dtype == torch.int32 and tuple(eng.aug_gates.shape) == (16,)
    seen = []
    for t in range(3):
        for k, run in ((0, lambda: eng.train_d_step(0)), (None, eng.train_full_step)):
            run()
            torch.cuda.synchronize()
            seen.append(_check_gated(eng, eng.d_in if k is None else eng.d_ins[k], k, t, "step %d piece %s" % (t, k)))
        off.train_step()
        torch.cuda.synchronize()
        assert torch.equal(eng.z, off.z)  # z keeps stream 0
        # the transposes replayed the fake half's rows: img_grad_t is the oracle's gated transposed gather
        ag = seen[-1][1]
        assert _same_bits(eng.img_grad_t, R.augment_transpose(eng.img_grad.cpu(), eng.aug_params[8:].cpu().long(), eng.aug,
                                                              gates=ag[8:]).to(dev))
    assert eng.ada_state.tolist() == R.ada_state(ONE // 2)  # a fixed p stays
    assert len({tuple(c.tolist()) for c, _ in seen}) == len(seen)  # fresh gates per step and per sub-step
    assert any(0 < int(c.ne(0).sum()) < 16 for c, _ in seen) and eng.ada_status()["p"] == 0.5


# ------------------------------------------------------------------ 5. against ReferenceStep (fixed p)
class _WithGates(HC._WithColor):
    gates = None

    def compute_grads(self, real, z, update_ema=True):
        return self.ref.compute_grads(real, z, update_ema=update_ema, color=self.color, augment=self.params, noise=self.noise,
                                      gates=self.gates)

    def compute_d_grads(self, real, z):
        return self.ref.compute_d_grads(real, z, color=self.color, augment=self.params, noise=self.noise, gates=self.gates)


def _gated_piece(eng, ref, ref_model, cfg, real, dtype, sn, k, run, tag, rdev):
    B2, p24, t = 2 * eng.B, int(eng.ada_state[0]), eng.global_step
    ref.gates = (R.gate_masks(B2, eng._zseed(k), t, 5, p24, eng.color.mask), R.gate_masks(B2, eng._zseed(k), t, 4, p24, eng.aug.mask))
    HC._color_piece(eng, ref, ref_model, cfg, real, dtype, sn, k, run, tag, rdev)
    assert torch.equal(eng.color_gates.cpu(), ref.gates[0]) and torch.equal(eng.aug_gates.cpu(), ref.gates[1]), tag


@pytest.mark.parametrize("dtype,size,c_dim", [("fp32", 28, 1), ("bf16", 28, 1), ("bf16", 64, 3)])
def test_four_gated_steps_track_the_reference(dtype, size, c_dim, seed=3):
    """Four steps after one warm-up step, as test_hip_d_color.py's colored and augmented steps (step 0 sits on
    the LeakyReLU kink over the zero-filled pixels)."""
    cfg, B = DCGANConfig(output_size=size, c_dim=c_dim), 8
    eng = TD._engine(cfg, B, 1, dtype=dtype, seed=seed, **FIXED)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, False, d_ada=R.check_ada(0.5), **ON)
    ref = _WithGates(ref)
    real = TD._reals(B, cfg, dtype, 1)[0].to(rdev)
    eng.train_step()
    for s in range(1, 5):
        _gated_piece(eng, ref, ref_model, cfg, real, dtype, False, None, eng.train_full_step, "step %d" % s, rdev)
    assert eng.global_step == 5


@pytest.mark.parametrize("size,c_dim", [(28, 1), (64, 3)])
def test_gated_cycle_with_sub_steps_and_spectral_norm_tracks_the_reference(size, c_dim, seed=4):
    cfg, B, dtype = DCGANConfig(output_size=size, c_dim=c_dim, d_bn=False), 8, "bf16"
    eng = TD._engine(cfg, B, 2, dtype=dtype, seed=seed, d_spectral_norm=True, beta2=0.9, **FIXED)
    ref_model, ref, rdev = TD._ref_for(cfg, dtype, seed, True, beta2=0.9, d_steps=2, d_ada=R.check_ada(0.5), **ON)
    ref = _WithGates(ref)
    reals = [x.to(rdev) for x in TD._reals(B, cfg, dtype, 2)]
    eng.train_step()  # (warm-up, as above)
    _gated_piece(eng, ref, ref_model, cfg, reals[0], dtype, True, 0, lambda: eng.train_d_step(0), "sub-step", rdev)
    _gated_piece(eng, ref, ref_model, cfg, reals[1], dtype, True, None, eng.train_full_step, "full", rdev)
    assert eng.global_step == 2


# ------------------------------------------------------------------ 6. the controller in the step
ADAPT = dict(ON, ada_target=0.6, ada_interval=2, ada_kimg=0.02)  # delta24 = 2^24 * 16 / 20: p moves and clamps


def _ada_consts(eng):
    a = eng.ada
    return (R.ada_threshold(eng.gan_loss, eng.label_smooth), R.ada_target_n(a.target, eng.B, a.interval),
            R.ada_delta24(eng.world, eng.B, a.interval, a.kimg), a.interval)


@pytest.mark.parametrize("dtype,size,c_dim,extra", [("bf16", 28, 1, {}), ("fp32", 28, 1, dict(gan_loss="lsgan", label_smooth=0.1)),
                                                    ("bf16", 64, 3, dict(d_steps=2))])
def test_adaptive_state_follows_the_oracle_fed_the_engines_own_logits(dtype, size, c_dim, extra):
    cfg = DCGANConfig(output_size=size, c_dim=c_dim)
    d_steps = extra.pop("d_steps", 1)
    eng = TD._engine(cfg, 8, d_steps, dtype=dtype, seed=3, **ADAPT, **extra)
    assert eng.op_names().count("ada_update") == 1 and eng.ada_state.tolist() == R.ada_state(0)
    assert all("ada_update" not in eng.sub_op_names(k) for k in range(d_steps - 1))
    want, ps = R.ada_state(0), []
    for t in range(9):
        for k in range(d_steps - 1):
            eng.train_d_step(k)
            torch.cuda.synchronize()
            assert eng.ada_state.tolist() == want  # a sub-step gates with the live p24 and leaves the state alone
            assert torch.equal(eng.aug_gates.cpu(), R.gate_masks(16, eng._zseed(k), t, 4, want[0], 3))
        eng.train_full_step()
        torch.cuda.synchronize()
        assert torch.equal(eng.color_gates.cpu(), R.gate_masks(16, eng._zseed(None), t, 5, want[0], 7)), t  # the p24 before the step
        want = R.ada_update(want, eng.logits[:8].cpu(), *_ada_consts(eng))
        assert eng.ada_state.tolist() == want, (t, eng.ada_state.tolist(), want)
        ps.append(want[0])
    assert want[4] == 4 and want[2] == 1 and len(set(ps)) > 1 and (0 in ps[1:] or ONE in ps)  # it moved, and clamped
    s = eng.ada_status()
    assert s["p"] == want[0] / ONE and s["r_t"] == want[3] / 16.0 and s["windows"] == 4


@pytest.mark.parametrize("dtype,d_steps", [("bf16", 2), ("fp16", 1)])
def test_graph_replay_equals_eager_on_the_live_state(dtype, d_steps):
    """A p24 baked in at capture time would keep the gates of the first replay's probability."""
    kw = dict(dtype=dtype, seed=1, **ADAPT)
    e1 = TD._engine(small(), 8, d_steps, **kw)
    e2 = TD._engine(small(), 8, d_steps, graph=True, **kw)
    ps = []
    for t in range(6):
        e1.train_step()
        e2.train_step()
        for x, y in zip(TD._snap(e1), TD._snap(e2)):
            assert torch.equal(x, y)
        assert torch.equal(e1.ada_state, e2.ada_state) and torch.equal(e1.color_gates, e2.color_gates)
        assert torch.equal(e1.aug_gates, e2.aug_gates) and _same_bits(e1.d_auged, e2.d_auged)
        assert _same_bits(e1.img_grad_c, e2.img_grad_c)
        ps.append(int(e2.ada_state[0]))
    assert e2.graph_enabled and not e1.graph_enabled and len(set(ps)) > 1
    assert e2.ada_state.tolist()[4] == 3 and e2.global_step == 6


def test_an_fp16_overflow_step_still_advances_the_controller():
    eng = TD._engine(small(), 8, 1, dtype="fp16", seed=1, **dict(ADAPT, ada_interval=1))
    eng.train_step()
    torch.cuda.synchronize()
    before, w0 = eng.ada_state.tolist(), eng.model.d.flat.clone()
    eng.loss_scale[0] = 1e38
    eng.train_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.model.d.flat, w0) and eng.loss_scale.tolist()[0] == pytest.approx(0.5e38, rel=1e-6)  # skipped
    want = R.ada_update(before, eng.logits[:8].cpu(), *_ada_consts(eng))
    assert eng.ada_state.tolist() == want and want[4] == before[4] + 1 and eng.global_step == 2


def test_the_switch_off_is_todays_engine():
    cfg = small()
    a = TD._engine(cfg, 8, 2, seed=2, d_augment_p=-1.0, ada_target=0.0, **ON)
    b = TD._engine(cfg, 8, 2, seed=2, **ON)
    c = TD._engine(cfg, 8, 2, seed=2, d_augment_p=1.0, **ON)
    for e in (a, b, c):
        assert not e.ada.active and e.ada_state is None and e.aug_gates is None and e.color_gates is None and e.progAda is None
    assert a.op_names() == b.op_names() == c.op_names() and a.kernel_count() == b.kernel_count()
    for _ in range(3):
        for e in (a, b, c):
            e.train_step()
    for x, y, w in zip(TD._snap(a), TD._snap(b), TD._snap(c)):
        assert torch.equal(x, y) and torch.equal(x, w)
    assert _same_bits(a.d_auged, b.d_auged) and torch.equal(a.color_params, b.color_params)
    # and p24 = 2^24 through the gated kernels is the same model, bitwise
    d = TD._engine(cfg, 8, 2, seed=2, d_augment_p=0.5, **ON)
    d.ada_state[0] = ONE
    for _ in range(3):
        d.train_step()
    for x, y in zip(TD._snap(d), TD._snap(b)):
        assert torch.equal(x, y)
    assert bool((d.aug_gates == 3).all()) and bool((d.color_gates == 7).all())


def test_eval_losses_stay_clean_and_leave_the_state_alone():
    cfg, B = small(), 8
    on = TD._engine(cfg, B, 1, seed=2, **ADAPT)
    off = TD._engine(cfg, B, 1, seed=7)
    on.train_step()
    torch.cuda.synchronize()
    for name in ("g", "d"):
        getattr(off.model, name).flat.copy_(getattr(on.model, name).flat)
    off.after_state_load()
    real = TD._reals(B, cfg, "bf16", 3)[2]
    z = torch.rand(B, cfg.z_dim, generator=torch.Generator().manual_seed(11)) * 2 - 1
    before = (on.ada_state.clone(), on.aug_gates.clone(), on.color_gates.clone(), on.d_auged.clone())
    a, b = on.eval_losses(real, z), off.eval_losses(real, z)
    assert a == b and a["d_loss"] > 0
    assert torch.equal(on.ada_state, before[0]) and torch.equal(on.aug_gates, before[1])
    assert torch.equal(on.color_gates, before[2]) and _same_bits(on.d_auged, before[3])
    names = [on.progEval.name(i) for i in range(on.progEval.size())]
    assert not {"d_color", "d_aug", "ada_update"} & set(names)
    assert names == [off.progEval.name(i) for i in range(off.progEval.size())]


# ------------------------------------------------------------------ 7. one-rank RCCL DDP
STEPS = 5


def _ddp_engine(graph):
    return TD._engine(small(), 8, 1, seed=3, graph=graph, rank_seeded_z=False, **ADAPT)


def _result(eng):
    torch.cuda.synchronize()
    return {"g": eng.model.g.flat.cpu(), "d": eng.model.d.flat.cpu(), "mg": eng.wbf_g.flat.cpu(),
            "md": eng.wbf_d.flat.cpu(), "losses": eng.losses.cpu(), "auged": eng.d_auged.cpu(),
            "state": eng.ada_state.cpu(), "cg": eng.color_gates.cpu(), "ag": eng.aug_gates.cpu(),
            "img_grad_c": eng.img_grad_c.cpu()}


def _rccl_worker(out_dir, schedule, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["DCGAN_FORCE_DDP"] = "1"
    os.environ["DCGAN_DDP_SCHEDULE"] = schedule
    os.environ["DCGAN_DDP_SHARD"] = "0"
    os.environ.pop("DCGAN_DIST_BACKEND", None)
    torch.cuda.set_device(0)
    from distributed_tensorflow_for_dcgan_amd.parallel import dist as D
    import torch.distributed as tdist
    D.init_distributed(1, 0, torch.device("cuda", 0))
    eng = _ddp_engine(True)
    assert eng.ddp and eng._schedule() == schedule and eng.ada.adaptive
    for _ in range(STEPS):
        eng.train_step()
    out = _result(eng)
    out.update({"step": eng.global_step, "backend": tdist.get_backend(), "graph": eng.graph_enabled, "ops": eng.op_names()})
    torch.save(out, os.path.join(out_dir, "rccl.pt"))
    D.barrier()
    D.shutdown()


@pytest.fixture(scope="module")
def fused_run():
    old = {k: os.environ.pop(k, None) for k in ENV}
    try:
        eng = _ddp_engine(True)
        assert not eng.ddp and eng._schedule() == "fused"
        for _ in range(STEPS):
            eng.train_step()
        return _result(eng)
    finally:
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("schedule", ["concurrent", "ddp"])
def test_rccl_single_rank_ddp_matches_fused_state_included(tmp_path, schedule, fused_run):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(str(tmp_path), schedule, SNT._free_port()))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0, "RCCL rank exited with %s" % p.exitcode
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r["backend"] == "nccl" and r["step"] == STEPS and r["graph"]
    assert r["ops"].count("ada_update") == 1
    for k, v in fused_run.items():
        assert torch.equal(r[k], v), k
    assert fused_run["state"].tolist()[4] == 2 and fused_run["state"].tolist()[2] == 1


# ------------------------------------------------------------------ 8. resume through the trainer
def test_trainer_resume_is_exact_in_the_middle_of_a_window(tmp_path, monkeypatch):
    """bf16, interval 4: 6 steps in one run == 2 steps (cnt = 2), a restart from the checkpoint, 4 more (the test's
    source alternates two batches, so an even split keeps them aligned) -- every saved tensor bitwise, the five
    ada/ keys among them; a run with a fixed p writes none of them."""
    from distributed_tensorflow_for_dcgan_amd.ckpt import checkpoint as CK
    from distributed_tensorflow_for_dcgan_amd.data import pipeline as P
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    from distributed_tensorflow_for_dcgan_amd.utils import flags as F

    def source(flags, batch, shape, device, **kw):
        class Two:
            num_examples = 1 << 20

            def __init__(self):
                self.i = 0
                self.x = [P.SyntheticSource(batch, shape, device, seed=s).next().to(torch.bfloat16) for s in (1, 2)]

            def next(self):
                self.i += 1
                return self.x[self.i % 2]

            def stats(self):
                return {"source": "test"}

            def close(self):
                pass
        return Two()
    monkeypatch.setattr(T, "make_source", source)
    AF = ["--d_color_augment=contrast,saturation,brightness", "--d_augment=translation,cutout", "--ada_target=0.6",
          "--ada_interval=4", "--ada_kimg=0.05", "--d_augment_p=0.5"]

    def run(ck, steps, af=AF):
        fl = F.parse_flags(["--synthetic", "--engine=hip", "--device=cuda", "--dtype=bf16", "--output_size=28",
                            "--c_dim=1", "--batch_size=8", "--max_steps=%d" % steps, "--sample_every=0", "--nosummaries",
                            "--save_model_secs=1e9", "--checkpoint_dir=%s" % ck, "--sample_dir=%s" % (tmp_path / "s"),
                            "--nolog_device_placement", "--seed=5"] + af)
        out = io.StringIO()
        assert T.run(fl, out=out) == 0, out.getvalue()
        return out.getvalue()

    def load(ck):
        from distributed_tensorflow_for_dcgan_amd.engine.hip_engine import HipEngine
        eng = HipEngine(small(), 8, dev, seed=99, graph=False, d_augment_p=0.5, ada_target=0.6, ada_interval=4,
                        ada_kimg=0.05, **ON)
        info = CK.CheckpointManager(str(ck)).restore_latest(eng)
        torch.cuda.synchronize()
        return info, CK.collect_state(eng), eng.ada_state.tolist()
    text = run(tmp_path / "a", 6)
    assert "augmentation probability of D's inputs: adaptive p from 0.5, target r_t = 0.6, every 4 steps" in text
    text = run(tmp_path / "b", 2)
    assert "load failed" in text
    text = run(tmp_path / "b", 6)
    assert "load success!" in text and "global_step 2" in text and "adaptive augmentation state: loaded" in text
    (ia, sa, ta), (ib, sb, tb) = load(tmp_path / "a"), load(tmp_path / "b")
    assert ia["global_step"] == ib["global_step"] == 6 and list(sa) == list(sb) and ta == tb
    assert [k for k in sa if k.startswith("ada/")] == ["ada/" + k for k in R.ADA_KEYS]
    assert int(sa["ada/cnt"]) == 2 and int(sa["ada/windows"]) == 1 and ta[:5] == [int(sa["ada/" + k]) for k in R.ADA_KEYS]
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    text = run(tmp_path / "c", 2, af=AF[:2] + ["--d_augment_p=0.5"])  # a fixed p: no key, and the controller's load says so
    assert "fixed p = 0.5" in text
    ic, sc, tc = load(tmp_path / "c")
    assert "starts from p = 0.5" in ic["ada"] and tc == R.ada_state(ONE // 2)
    from distributed_tensorflow_for_dcgan_amd.ckpt import tf_bundle
    ckc = CK.latest_checkpoint(str(tmp_path / "c"))
    assert ckc is not None and not any(k.startswith("ada/") for k in tf_bundle.read_bundle(ckc))
