"""The turbo decoder's sub-block schedule (ltesniffer_amd/csrc/kernels/lsn_turbo_core.h) on the CPU: the short sub-block of a window comes first, so that
the forward sweep skips a full one.  tests/native/test_turbo_subblocks.cc checks, for all 188 block sizes, that the sub-blocks tile the window with a full last
one and that a pass runs W - 16 forward-sweep steps; that every half-word of the interleaver address table the decoder reads is the transposed address of the
QPP permutation computed by brute force (and every unused half-word an address inside the block); and runs the decoder text the way the second block of a
paired workgroup gets it (index biases non-zero) against the oracle's decoder, with every packed add range-checked.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("TURBO_CXX", "/opt/rocm/lib/llvm/bin/clang++")   # as tests/native/Makefile
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def report():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("needs clang (ext_vector_type)")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    exe = os.path.join(NATIVE, "_build", "test_turbo_subblocks.%d" % os.getpid())   # (a program of this process: pytest workers may each build one)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(NATIVE, "test_turbo_subblocks.cc"),
                           "-L" + os.path.join(ROOT, "oracle", "_build"), "-llsn_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_build")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    os.remove(exe)
    lines = {l.split(":")[0]: l for l in out.stdout.splitlines() if ":" in l}
    return out, lines


def test_forward_sweep_skips_a_full_sub_block_at_every_block_size(report):
    out, lines = report
    w = lines["geometry"].split()
    assert int(w[1]) == 188 and int(w[3]) == 103 and int(w[-2]) == 0, out.stdout[-2000:] + out.stderr[-2000:]


def test_interleaver_table_holds_the_qpp_addresses_the_decoder_reads(report):
    out, lines = report
    w = lines["table"].split()
    assert int(w[1]) > 0 and int(w[-3]) == 0, out.stdout[-2000:] + out.stderr[-2000:]


def test_second_block_of_a_pair_decodes_as_the_oracle(report):
    out, lines = report
    w = lines["second half"].split()
    # 4 sizes (W mod 16 = 0, 1, 8, 15) x 6 x {marginal code word, saturated noise}, 12 iterations at most; the noise cases alone run 4 x 6 x 12 iterations,
    # and some of the code words must have needed several
    assert int(w[2]) == 48 and int(w[4]) >= 288 and int(w[6]) >= 4 and int(w[-2]) == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
