"""The PDSCH demodulator's row geometry (ltesniffer_amd/csrc/kernels/lsn_rows.h) on the CPU: a row is one (symbol, allocated PRB) of a decode job in mapping
order and a demodulator workgroup takes 16 consecutive rows.  tests/native/test_demod_rows.cc checks the header - the one copy of the rule that the host's
work-item count, the prep kernel's PRB lists and the demodulator's row lookup share - against a brute-force enumeration: nof_prb in {6, 15, 25, 50, 75, 100,
110} x nslot in {7, 6} x l0 in 1 .. 4, every contiguous run, seeded RBG bitmaps with gaps, masks that differ between the slots (a slot without PRBs among
them) and the empty allocation.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CONFIGS = 7 * 2 * 4                                                    # (nof_prb, nslot, l0)
RUNS = 8 * sum(n * (n + 1) // 2 for n in (6, 15, 25, 50, 75, 100, 110))  # contiguous (start, length) runs over all of them


@pytest.fixture(scope="module")
def report():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = os.path.join(NATIVE, "_build", "test_demod_rows.%d" % os.getpid())   # (a program of this process: pytest workers may each build one)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(NATIVE, "test_demod_rows.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    os.remove(exe)
    lines = {}
    for l in out.stdout.splitlines():
        name, _, rest = l.partition(":")
        w = rest.split()
        lines[name] = {"cases": int(w[0]), "rows": int(w[2]), "errors": int(w[4])}
    return out, lines


def _tail(out):
    return out.stdout[-2000:] + out.stderr[-2000:]


def test_rows_are_the_allocated_symbol_prb_pairs_in_mapping_order(report):
    """every contiguous run and the seeded RBG bitmaps: the rows are the allocated (symbol, PRB) pairs, each once, symbol-major and PRBs ascending; the work
    items cover rows 0 .. R-1 once with fewer than 16 rows of padding; row -> (symbol, ordinal) holds at every row"""
    out, lines = report
    assert lines["runs"]["cases"] == RUNS and lines["runs"]["rows"] > 0 and lines["runs"]["errors"] == 0, _tail(out)
    assert lines["rbg"]["cases"] == 40 * CONFIGS and lines["rbg"]["rows"] > 0 and lines["rbg"]["errors"] == 0, _tail(out)


def test_slots_with_different_prb_sets_and_a_slot_without_prbs(report):
    out, lines = report
    assert lines["differ"]["cases"] == 160 * CONFIGS and lines["differ"]["rows"] > 0 and lines["differ"]["errors"] == 0, _tail(out)


def test_empty_allocation_has_no_rows_and_no_work_items(report):
    out, lines = report
    assert lines["empty"] == {"cases": CONFIGS, "rows": 0, "errors": 0}, _tail(out)


def test_division_constant_is_exact_for_every_row_index_and_prb_count(report):
    out, lines = report
    assert lines["division"] == {"cases": 110, "rows": 110 * 14 * 110, "errors": 0}, _tail(out)


def test_eight_prbs_at_prb_12_of_100_take_the_dense_item_count(report):
    """PRBs 12-19 of a 100-PRB cell: ceil(8 (14 - l0) / 16) work items for l0 = 1 .. 4 (the mapping by absolute groups of 16 PRBs took 2 x 14 workgroups)"""
    out, lines = report
    assert lines["example"] == {"cases": 4, "rows": 8 * (13 + 12 + 11 + 10), "errors": 0}, _tail(out)
    assert out.returncode == 0, _tail(out)
