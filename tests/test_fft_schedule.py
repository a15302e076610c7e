"""The symbol transform's schedule (ltesniffer_amd/csrc/kernels/lsn_fft_map.h) on the CPU.  tests/native/test_fft_schedule.cc replays what k_ofdm and k_ul_fft
do - 256 threads, pass by pass, a plain array for LDS, every index from the header the kernels use - and holds it word for word to the oracle's o_fft (128,
256, 512, 1024, 2048, 1536) and, at 384 and 768, to the three-way formula restated on o_fft(M) (which it first shows to be o_fft(1536) at M = 512).  It
counts the LDS bank conflicts of every pass under the per-instruction lane groups (8-byte reads: 32 lanes on 64 banks, 8-byte writes: 16 lanes on 32 banks)
and checks that the last pass covers every kept carrier once inside the declared LDS size.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
ROWS = 8                                   # random, zeros, negative zeros, four impulses, denormals


@pytest.fixture(scope="module")
def report():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = os.path.join(NATIVE, "_build", "test_fft_schedule.%d" % os.getpid())   # (a program of this process: pytest workers may each build one)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    odir = os.path.join(ROOT, "oracle", "_build")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(NATIVE, "test_fft_schedule.cc"), "-L" + odir, "-llsn_oracle", "-Wl,-rpath," + odir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    os.remove(exe)
    lines, bank = {}, {}
    for l in out.stdout.splitlines():
        name, _, rest = l.partition(":")
        if name.startswith("bank "):
            bank[int(name.split()[1])] = [int(x) for x in re.findall(r"-?\d+", rest)]
            continue
        w = rest.split()
        lines[name] = {"cases": int(w[0]), "words": int(w[2]), "errors": int(w[4])}
    return out, lines, bank


def _tail(out):
    return out.stdout[-3000:] + out.stderr[-3000:]


def test_schedule_equals_o_fft_word_for_word(report):
    out, lines, _ = report
    n = 128 + 256 + 512 + 1024 + 2048 + 1536
    assert lines["exact"] == {"cases": 6 * ROWS, "words": 2 * n * ROWS, "errors": 0}, _tail(out)


def test_three_way_sizes_equal_the_formula_restated_on_o_fft(report):
    """the restatement at M = 512 is o_fft(1536) bit for bit; the schedule at 384 and 768 is the restatement"""
    out, lines, _ = report
    assert lines["three"] == {"cases": 3 * ROWS, "words": 2 * (384 + 768 + 1536) * ROWS, "errors": 0}, _tail(out)


def test_lds_reads_are_conflict_free_and_writes_at_most_two_way(report):
    out, lines, bank = report
    assert sorted(bank) == [128, 256, 384, 512, 768, 1024, 1536, 2048], _tail(out)
    for n, (rc, rx, rw, wc, wx, ww, oc, ox, ow) in bank.items():
        print("N = %4d: %5d LDS cycles, %4d of them conflicts (reads %d-way, writes %d-way); before %5d, %5d, %d-way" % (n, rc + wc, rx + wx, rw, ww, oc, ox, ow))
        assert rx == 0 and rw == 1 and ww <= 2, (n, _tail(out))
    assert lines["conflicts"]["errors"] == 0, _tail(out)
    assert bank[2048][1] + bank[2048][4] == 0 and bank[1024][4] == 0 and bank[512][4] == 0, _tail(out)   # the power-of-two sizes from 512 up: none at all


def test_last_pass_covers_every_kept_carrier_once_inside_the_lds_image(report):
    out, lines, _ = report
    assert lines["cover"] == {"cases": 16, "words": 2 * (72 + 180 + 300 + 600 + 1200 + 300 + 600 + 900), "errors": 0}, _tail(out)
    assert out.returncode == 0, _tail(out)
