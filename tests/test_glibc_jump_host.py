"""The tables the device generator starts from, on the host (glibc_rand.hpp):
glibc_jump_table's words, glibc_pow_table's squares M^(2^k) and the products
glibc_starts_pow_kernel forms from them, and GlibcRand's window / set_window /
commit, each against plainly stepping GlibcRand::next_raw
(tests/native/glibc_check.cpp).

Every level k <= 15 is stepped (4096 * 2^15 = 1.3e8 words, under a second a
seed): all the levels a 16M-sample epoch uses.  Levels 16 to 23 of the 24 the
engine builds are not checked here: stepping to them costs more than 1e10
words.  The composite block numbers are the last block of a 4.5M-word epoch
(1,099), of the 16M-sample epoch (19,531), small ones and an alternating bit
pattern."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def glibc_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("glibc") / "glibc_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "glibc_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("seed", [1, 7, 2 ** 31 - 1])
def test_jump_and_power_tables_match_stepping(glibc_check, seed):
    out = subprocess.run([glibc_check, str(seed)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    word, checks = out.stdout.split()
    # the jump table, 16 squares + 4 further block numbers (1 and 2 are squares), 2 x 6 round trips of 3 checks
    assert word == "ok" and int(checks) == 1 + 20 + 36
