"""CPU tests of --swd_max_rows, the opt-in to sets of more than 32768 descriptors, and of check_swd's bound."""
import re

import pytest

from distributed_tensorflow_for_dcgan_amd.ops import reference as R
from distributed_tensorflow_for_dcgan_amd.utils import flags as F


@pytest.mark.parametrize("argv,msg", [
    (["--swd_max_rows=65536", "--swd_images=512"], None),
    (["--swd_max_rows=65536", "--swd_images=1024"], r"--swd_images . --swd_patches must be a power of two in \[16, 65536\]"),
    (["--swd_max_rows=49152"], r"--swd_max_rows must be a power of two in \[32768, 2097152\]"),
    (["--swd_max_rows=16384"], r"--swd_max_rows must be a power of two in \[32768, 2097152\]"),
    (["--swd_max_rows=%d" % 2 ** 22], r"--swd_max_rows must be a power of two in \[32768, 2097152\]"),
])
def test_flag_validation(argv, msg, capsys):
    if msg is None:
        fl = F.parse_flags(argv)
        assert (int(fl.swd_max_rows), int(fl.swd_images)) == (65536, 512)
        return
    with pytest.raises(SystemExit):
        F.parse_flags(argv)
    assert re.search(msg, capsys.readouterr().err)


def test_check_swd_bound_follows_max_rows():
    with pytest.raises(ValueError, match=r"\[16, 32768\] \(larger sets need a global merge sort\)"):
        R.check_swd(512, 128, 32)
    assert R.check_swd(512, 128, 32, max_rows=65536) == 65536
    with pytest.raises(ValueError, match=r"\[16, 65536\]"):
        R.check_swd(1024, 128, 32, max_rows=65536)
