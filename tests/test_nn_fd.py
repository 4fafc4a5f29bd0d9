"""CPU tests of the Frechet distance's oracle (ops/reference.py): the dual form against the textbook formula, the fp64
polar iteration against svdvals, the validation of --nn_fd, and the reference engine's [FD] line through the trainer."""
import io
import math
import re

import pytest
import torch

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


def _sqrtm(S):  # of a symmetric positive semi-definite matrix
    w, V = torch.linalg.eigh(S)
    return (V * w.clamp_min(0).sqrt()) @ V.T


@pytest.mark.parametrize("n,K", [(12, 5), (9, 9), (8, 40)])
def test_dual_form_equals_the_textbook_formula(n, K):
    g = torch.Generator().manual_seed(n)
    A = torch.randn(n, K, generator=g, dtype=torch.float64) @ torch.randn(K, K, generator=g, dtype=torch.float64)
    B = 0.5 * torch.randn(n, K, generator=g, dtype=torch.float64) + 0.3
    SA, SB, ra = torch.cov(A.T), torch.cov(B.T), _sqrtm(torch.cov(A.T))
    ev = torch.linalg.eigvalsh(ra @ SB @ ra).clamp_min(0)
    cross = ev.sqrt().sum()  # tr (S_A S_B)^(1/2), symmetrised
    want = float(((A.mean(0) - B.mean(0)) ** 2).sum() + SA.trace() + SB.trace() - 2 * cross)
    got = R.nn_frechet(A, B)
    # the textbook's own error: eigh leaves eps * max on each of the K - n + 1 zero eigenvalues, and the root takes its root
    tol = 1e-9 * want + 2 * K * math.sqrt(2.0 ** -52 * float(ev.max()))
    assert got.fd == pytest.approx(want, abs=2 * tol) and got.nuc == pytest.approx(float(cross), abs=tol)
    assert (got.tail, got.alpha, got.iters) == (0.0, 0.0, 0)
    assert R.nn_frechet(A, A).fd == pytest.approx(0.0, abs=1e-9 * got.tr_a)
    shifted = R.nn_frechet(A, A + 2.0)  # the fakes' own mean is taken out of C: only mean2 moves
    assert shifted.mean2 == pytest.approx(4.0 * K, rel=1e-12) and shifted.fd == pytest.approx(4.0 * K, rel=1e-9)
    assert R.nn_fd_report(got) == {"fd": got.fd, "fd_mean2": got.mean2, "fd_tr": got.tr_a + got.tr_b, "fd_nuc": got.nuc,
                                   "fd_tail": 0.0}


@pytest.mark.parametrize("n,cond", [(16, 1e2), (40, 1e4)])
def test_polar_iteration_reaches_svdvals_from_below(n, cond):
    g = torch.Generator().manual_seed(7)
    U, V = (torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0] for _ in range(2))
    sigma = torch.logspace(0, -math.log10(cond), n, dtype=torch.float64)
    C = (U * sigma) @ V.T
    want = float(torch.linalg.svdvals(C).sum())
    # alpha <= sqrt(n) sigma_max, and a singular value below 1 / 2 grows by at least 1.25 per step: the count below
    # brings the smallest one up to order 1, and ten more steps square the rest of the error away
    need = math.ceil(math.log(math.sqrt(n) * cond) / math.log(1.25)) + 10
    nuc, tail, alpha = R.nn_polar_nuclear(C, need)
    assert alpha >= float(sigma[0]) and nuc == pytest.approx(want, rel=1e-12) and abs(tail) <= 1e-12 * want
    early = math.floor(math.log(cond) / math.log(1.5)) - 2  # 1.5^k sigma_min / alpha < 0.45: its share is still missing
    values = [R.nn_polar_nuclear(C, k)[0] for k in (1, early // 2, early)]
    assert values[0] < values[1] < values[2] < want - 0.25 * float(sigma[-1])
    assert R.nn_polar_nuclear(torch.zeros(3, 3, dtype=torch.float64), 2) == (0.0, 0.0, 0.0)
    assert R.nn_frechet(C, C.flip(0), need).fd == pytest.approx(R.nn_frechet(C, C.flip(0)).fd, rel=1e-9)


@pytest.mark.parametrize("argv,ok", [(["--nn_fd"], True), (["--nn_fd", "--nn_images=1"], False), (["--nn_fd_iters=0"], False),
                                     (["--nn_fd", "--nn_fd_iters=12", "--nn_images=8"], True), (["--nn_fd_iters=257"], False)])
def test_flag_validation(argv, ok):
    if ok:
        fl = F.parse_flags(argv)
        assert fl.nn_fd is True and fl.nn_fd_iters == (12 if len(argv) > 1 else R.NN_FD_ITERS) and R.NN_FD_ITERS == 40
        assert F.parse_flags([]).nn_fd is False
    else:
        with pytest.raises(SystemExit):
            F.parse_flags(argv)
    with pytest.raises(ValueError):
        R.check_nn_fd(True, 8)
    assert R.check_nn_fd(0, 1) == 0 and R.check_nn_fd(40, 2) == 40


def test_reference_engine_through_the_trainer(tmp_path):
    from distributed_tensorflow_for_dcgan_amd.train import trainer as T
    fl = F.parse_flags(["--synthetic", "--engine=reference", "--device=cpu", "--output_size=32", "--c_dim=1",
                        "--batch_size=4", "--sample_every=0", "--max_steps=2", "--nn_every=2", "--nn_images=6",
                        "--nn_size=16", "--nn_fd", "--checkpoint_dir=%s" % (tmp_path / "ck"),
                        "--sample_dir=%s" % (tmp_path / "s"), "--nolog_device_placement"])
    out = io.StringIO()
    assert T.run(fl, out=out) == 0
    lines = re.findall(r"^\[FD\] step 2  fd (\S+)  mean2 (\S+)  tr (\S+)  nuc (\S+)  tail (\S+)$", out.getvalue(), re.M)
    assert len(lines) == 1 and "[MMD]" not in out.getvalue()
    fd, mean2, tr, nuc, tail = map(float, lines[0])
    assert fd > 0 and tr > 2 * nuc > 0 and abs(fd - (mean2 + tr - 2 * nuc)) < 1e-3 and abs(tail) < 1e-3 * nuc  # (fp32 here)
