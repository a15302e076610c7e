"""Several cells of one recording in one pass (k_resample_cells; lsn_resample_cells, lsn_file_process_cells): the kernel against k_resample cell by cell, bit for
bit, and the replay against the oracle's records and against the single-cell replay of every cell - two 100-PRB cells of the 61.44 MS/s recording, a 75-PRB next
to a 25-PRB cell in a 30.72 MS/s one, the chain from the carrier scan, per-cell LSN_TTI_FROM_MIB and max_subframes, and the refusals that need a device.
Nothing here is a tolerance: every comparison is bit identity or record equality."""
import contextlib
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from cells_cases import MIXED_NSF, MIXED_RATE, mixed_recording
from ddc_cases import quantise, recording
from parity import gpu_records
from resample_cases import FAR, LEAD
from resample_model import passband_hz

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
RATE = 30.72e6
# three cells of one 30.72 MS/s input: one at the centre (the plain branch) between two translated ones of opposite sign; three rate pairs (D = 4, 4/3 and 1,
# each with its own number of taps), the third with a fractional start; 511, 512 and 1300 outputs = one partial run, one full run and three runs, so the grid's x extent (3)
# leaves workgroups without work in the first two cells; the starts spread the cells over the input
THREE = (dict(rate_out=7.68e6, passband_hz=passband_hz(25), center_offset_hz=0.0, n_out=511, first_sample=12345, first_frac=0.0),
         dict(rate_out=23.04e6, passband_hz=passband_hz(75), center_offset_hz=4.5e6, n_out=512, first_sample=5000, first_frac=0.5),
         dict(rate_out=30.72e6, passband_hz=passband_hz(100), center_offset_hz=-3.3e6, n_out=1300, first_sample=0, first_frac=0.4375))
EIGHT = tuple(dict(rate_out=r, passband_hz=passband_hz(p), center_offset_hz=f0, n_out=100, first_sample=2000 * i, first_frac=i / 8.0)
              for i, (r, p, f0) in enumerate(((7.68e6, 25, 7.5e6), (15.36e6, 50, -5e6), (23.04e6, 75, 0.0), (30.72e6, 100, 1e6), (7.68e6, 25, -12e6), (15.36e6, 50, 0.0),
                                              (23.04e6, 75, -8e6), (30.72e6, 100, 6e6))))


def _noise(n, nant, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == la.FILE_CF32:
        return (rng.standard_normal((n, nant)) + 1j * rng.standard_normal((n, nant))).astype(np.complex64), 0.0
    full, dt, scale = ((32767, np.int16, 1.0 / 9000.0), (127, np.int8, 1.0 / 30.0))[fmt - 1]     # not powers of two: the conversion rounds
    return rng.integers(-full, full + 1, (n, nant, 2)).astype(dt), scale


def _shift(cells, first):
    return [dict(c, first_sample=c["first_sample"] + first) for c in cells]


@pytest.mark.parametrize("first", [0, FAR])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_kernel_is_k_resample_cell_by_cell_bit_for_bit(fmt, first):
    n_in, nant = 20000, 2
    x, scale = _noise(n_in, nant, fmt, 3 + fmt)
    base = max(first - 100, 0)     # first = 0: the third cell reads zeros in front of the recording
    for cells in (_shift(THREE, first), _shift(EIGHT, first)):
        got = la.resample_cells(x, RATE, cells, in_base=base, sample_format=fmt, sample_scale=scale)
        assert len(got) == len(cells)
        for c, y in zip(cells, got):
            kw = {k: v for k, v in c.items() if k != "rate_out"}
            one = la.resample(x, RATE, c["rate_out"], in_base=base, sample_format=fmt, sample_scale=scale, **kw)
            assert y.shape == one.shape == (nant, c["n_out"]) and float(np.abs(one).max()) > 0
            assert np.array_equal(y.view(np.uint32), one.view(np.uint32)), c


def test_kernel_call_refuses_nine_cells_and_unequal_antennas_with_the_outputs_untouched():
    L = la.lib()
    x, _ = _noise(20000, 2, la.FILE_CF32, 1)

    def call(cells, edit=None):
        n = len(cells)
        cfgs = (la.ResampleCfg * n)(*[la._resample_cfg(2, RATE, c["rate_out"], c["first_sample"], c["first_frac"], 0, 0, c["passband_hz"], la.FILE_CF32, 0.0, c["center_offset_hz"])
                                      for c in cells])
        if edit:
            edit(cfgs)
        outs = [np.full((2, c["n_out"]), 7 + 7j, dtype=np.complex64) for c in cells]
        rc = L.lsn_resample_cells(0, x.ctypes.data, 0, len(x), cfgs, n, (C.c_void_p * n)(*[o.ctypes.data for o in outs]), 0, (C.c_uint64 * n)(*[c["n_out"] for c in cells]))
        return rc, all(np.all(o == 7 + 7j) for o in outs)

    assert call(list(EIGHT)) == (0, False)
    assert call(list(EIGHT) + [EIGHT[0]]) == (INVALID, True)

    def one_antenna(cfgs):
        cfgs[1].nof_antennas = 1
    assert call(list(THREE), one_antenna) == (INVALID, True)

    def other_format(cfgs):
        cfgs[2].sample_format = la.FILE_SC16
    assert call(list(THREE), other_format) == (INVALID, True)
    assert call(list(THREE)) == (0, False)


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


@contextlib.contextmanager
def _block(n):
    """LSN_FILE_BLOCK = n for the replays inside (every Phy of a multi-cell replay holds its block buffers: small blocks, as test_gpu_ddc.py)"""
    old = os.environ.get("LSN_FILE_BLOCK")
    os.environ["LSN_FILE_BLOCK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LSN_FILE_BLOCK", None)
        else:
            os.environ["LSN_FILE_BLOCK"] = old


def _write(td, f, fmt, name="c"):
    raw, scale, _ = quantise(f, fmt)
    p = os.path.join(td, name + (".cf32", ".sc16")[fmt])
    raw.tofile(p)
    return p, scale


def _cells_replay(path, rate_in, cells, fmt, scale):
    """cells: [(sc, options, per-cell arguments)] -> (subframes done per cell, records per cell); the Phys live only as long as the call"""
    phys = [_phy(sc, **opt) for sc, opt, _ in cells]
    try:
        done = la.process_file_cells(path, rate_in, [(p, kw) for p, (_, _, kw) in zip(phys, cells)], sample_format=fmt, sample_scale=scale)
        return done, [gpu_records(p) for p in phys]
    finally:
        for p in phys:
            p.close()


def _single_replay(path, rate_in, sc, opt, kw, fmt, scale):
    phy = _phy(sc, **opt)
    try:
        n = phy.process_file_rate(path, rate_in, sample_format=fmt, sample_scale=scale, **kw)
        return n, gpu_records(phy)
    finally:
        phy.close()


def _two_cells():
    a, b = recording("two_cells_a"), recording("two_cells_b")
    assert np.array_equal(a[-1], b[-1]) and a[5] == b[5] == 61.44e6 and a[2] != b[2] and min(len(a[2]), len(b[2])) >= 10
    return [(r[0], r[4], dict(center_offset_hz=r[7], start_tti=r[1], offset_time=LEAD)) for r in (a, b)], [r[2] for r in (a, b)], a[5], a[-1]


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_two_cells_of_one_wideband_file_in_one_pass(fmt):
    """the 61.44 MS/s recording with two 100-PRB cells at +-9.9 MHz: one process_file_cells call with two Phys returns 12 and 12 subframes and each Phy's records are
    its cell's oracle records and those of its single-cell process_file_rate replay; two block sizes (5 divides neither 12 nor the shrunk block), the cells also
    in the other order"""
    cells, orecs, rate_in, f = _two_cells()
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, fmt)
        with _block(16):
            single = [_single_replay(path, rate_in, sc, opt, kw, fmt, scale) for sc, opt, kw in cells]
            assert [n for n, _ in single] == [12, 12] and [g for _, g in single] == orecs
            done, got = _cells_replay(path, rate_in, cells[::-1], fmt, scale)
            assert done == [12, 12] and got == orecs[::-1], (done, [len(g) for g in got])
        with _block(5):
            done, got = _cells_replay(path, rate_in, cells, fmt, scale)
            assert done == [12, 12] and got == orecs and got == [g for _, g in single], (done, [len(g) for g in got], [len(o) for o in orecs])


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_cells_of_different_bandwidth_in_one_pass(fmt):
    """cells_cases.mixed_recording: a 75-PRB cell at -4.5 MHz and a 25-PRB cell at +7.5 MHz (whole Hz, each confined to its 15 / 5 MHz channel, equal amplitude)
    in one 30.72 MS/s file - the offsets at which the CPU round trip (test_cells_plan.py) returns every record of both.  The 25-PRB capture is longer than the
    file: its cell is cut by max_subframes, the 75-PRB cell's count is what lies inside the file.  Both record lists equal the oracle's."""
    cells, f = mixed_recording()
    jobs = [(sc, opt, dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, max_subframes=MIXED_NSF if sc["nof_prb"] == 25 else 0)) for sc, tti0, _, opt, f0, _ in cells]
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, fmt)
        with _block(8):     # 8 subframes of the 75-PRB cell's buffer: the block shrinks to 5 (cf32) so that the 30.72 MS/s input fits
            done, got = _cells_replay(path, MIXED_RATE, jobs, fmt, scale)
    assert done == [MIXED_NSF, MIXED_NSF], done
    for (sc, _, orecs, _, _, _), g in zip(cells, got):
        assert len(orecs) >= 10 and g == orecs, "%d PRB: %d records vs %d" % (sc["nof_prb"], len(g), len(orecs))


def test_chain_from_the_carrier_scan_into_one_pass():
    """file_carrier_scan on the two-cell file; the carriers it returns go, unchanged, into process_file_cells (a Carrier is taken for center_offset_hz), each with a
    Phy of the bandwidth and ports carrier_mib reports and the cell id and CP of the scan's search: the records of test_two_cells_of_one_wideband_file_in_one_pass"""
    cells, orecs, rate_in, f = _two_cells()
    by_offset = {kw["center_offset_hz"]: (sc, opt, kw, o) for (sc, opt, kw), o in zip(cells, orecs)}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "two.cf32")
        cap = f.astype(np.complex64)
        cap.tofile(path)
        found = la.file_carrier_scan(path, rate_in, nof_antennas=cap.shape[1], nof_periods=1)
        assert sorted(c.center_offset_hz for c in found) == sorted(by_offset)
        jobs, want = [], []
        for c in found:
            sc, opt, kw, o = by_offset[c.center_offset_hz]
            mib = la.carrier_mib(la.carrier_channel(cap, rate_in, c.center_offset_hz), c.search)
            assert mib is not None and c.search.cell_id == sc["cell_id"]
            found_cell = dict(sc, nof_prb=mib["nof_prb"], nof_ports=mib["nof_ports"], cell_id=int(c.search.cell_id), cp=int(c.search.cp))
            jobs.append((found_cell, opt, dict(kw, center_offset_hz=c)))
            want.append(o)
        with _block(16):
            done, got = _cells_replay(path, rate_in, jobs, la.FILE_CF32, 0.0)
    assert done == [12, 12] and got == want, (done, [len(g) for g in got])


def test_start_tti_from_the_mib_and_max_subframes_are_per_cell():
    """the two-cell recording behind ten subframes of faint noise.  Cell A is started IN the noise: no MIB at its subframe 0, the one at its subframe 10 decodes, so
    its replay drops ten subframes (first_sf = 10) and is then limited to 7.  Cell B is started ten subframes further in, where the cells begin: MIB at once, to
    the end.  As handed in, the starts lie ten subframes apart; behind the MIB scans both cells read the same samples and the block is fitted again.  Counts and
    records equal the single-cell calls', and the cells' oracle records: all 12 subframes of B, the records of A's first 7."""
    from ddc_cases import cell
    from parity import oracle_records, run_oracle
    cells, orecs, rate_in, f = _two_cells()
    (sa, oa, ka), (sb, ob, kb) = cells
    rng = np.random.default_rng(12)
    pad = 10 * 61440
    noise = 1e-3 * (rng.standard_normal((pad, f.shape[1])) + 1j * rng.standard_normal((pad, f.shape[1])))
    jobs = [(sa, oa, dict(ka, start_tti=la.TTI_FROM_MIB, max_subframes=7)), (sb, ob, dict(kb, start_tti=la.TTI_FROM_MIB, offset_time=LEAD + pad))]
    _, tti0, iq, _, _, _ = cell("A")
    _, _, want_a = run_oracle(sa, tti0, iq[:7], taps=False, **oa)
    want = [oracle_records(want_a), orecs[1]]
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, np.concatenate([noise, f]), la.FILE_CF32)
        with _block(32):     # 32 subframes of cf32 output = 16 of 61.44 MS/s input: starts 10 subframes apart fit with 5 subframes per block, behind the MIBs with 15
            single = [_single_replay(path, rate_in, sc, opt, kw, la.FILE_CF32, scale) for sc, opt, kw in jobs]
            done, got = _cells_replay(path, rate_in, jobs, la.FILE_CF32, scale)
        with _block(16):     # 8 subframes of input: one subframe of each cell, 10 apart as handed in, does not fit one block
            with pytest.raises(ValueError):
                _cells_replay(path, rate_in, jobs, la.FILE_CF32, scale)
    assert [n for n, _ in single] == [7, 12] and done == [7, 12], (single[0][0], single[1][0], done)
    assert got == [g for _, g in single] and min(len(g) for g in got) > 0
    assert got == want, ([len(g) for g in got], [len(w) for w in want])


def test_refusals_decode_nothing_and_leave_every_phy_usable():
    cells, orecs, rate_in, f = _two_cells()
    (sa, oa, ka), (sb, ob, kb) = cells
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, la.FILE_CF32)
        with _block(16):
            pa, pb = _phy(sa, **oa), _phy(sb, **ob)
            multi = la.Phy(nof_rx_antennas=2, max_batch=4, pcapwriter=la.PcapWriter(None), devices=[0, 0])
            assert multi.setCell(sb["nof_prb"], sb["nof_ports"], sb["cell_id"], PHICH[sb["phich_ng_x6"]])
            bare = la.Phy(nof_rx_antennas=2, max_batch=4, pcapwriter=la.PcapWriter(None))
            one = la.Phy(nof_rx_antennas=1, max_batch=4, pcapwriter=la.PcapWriter(None))
            assert one.setCell(100, 2, 9)
            try:
                for bad in ([(pa, ka), (pa, kb)],                      # a Phy twice
                            [(pa, ka), (multi, kb)],                   # a lsn_phy_create_multi handle
                            [(pa, ka), (bare, kb)],                    # a Phy without a cell
                            [(pa, ka), (one, kb)],                     # a Phy with another antenna count than the file's
                            [(pa, ka), (pb, dict(kb, center_offset_hz=25e6))],    # a cell its single-cell call refuses
                            []):
                    with pytest.raises(ValueError):
                        la.process_file_cells(path, rate_in, bad, nof_antennas=2)
                    assert gpu_records(pa) == [] and gpu_records(pb) == []
                arr = (la.FileCell * 2)(la._file_cell(pa, ka), la._file_cell(None, dict(kb, nof_prb=100)))     # a null phy
                fc = la.FileCfg(2, 0, 0.0, la.FILE_CF32, 0.0)
                assert la.lib().lsn_file_process_cells(os.fsencode(path), C.byref(fc), rate_in, arr, 2) == INVALID
                assert arr[0].subframes_done == 0 and arr[0].status == INVALID and gpu_records(pa) == []
                for phy, kw, o in ((pa, ka, orecs[0]), (pb, kb, orecs[1])):
                    assert phy.process_file_rate(path, rate_in, **kw) == 12
                    assert gpu_records(phy) == o
            finally:
                for p in (pa, pb, multi, bare, one):
                    p.close()
