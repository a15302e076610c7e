"""The antenna map on the GPU (lsn_phy_set_antenna_map, lsn_resample_cells[_ring]_map; k_resample_map and its ring and wide-ratio twins):
the map kernels against the unmapped resampler bit for bit, the ring kernels against the linear ones, and end to end - UL_MODE from ONE antenna of a wideband
recording (file replay, multi-cell pass, stream) and two of four antennas - to the oracle's records (tests/test_antmap_model.py is the CPU round trip)."""
import contextlib
import ctypes as C
import itertools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from antmap_cases import (FOUR_NSF, FOUR_OFFSET, FOUR_RATE, UL_RECORDINGS, UL_RECORDS, four_antennas, ul_baseline, ul_recording)
from ddc_cases import quantise, recording
from parity import gpu_records
from resample_cases import FAR, LEAD
from resample_model import passband_hz
from srs_streams import edge_blocks, failed_records

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS

# (rate_in, rate_out, nof_prb): up-sampling, ratio 4 (the ordinary run), ratio 8 (8 lanes per output) and ratio 32 (32 lanes per output)
PAIRS = [(25e6, 30.72e6, 100), (30.72e6, 7.68e6, 25), (61.44e6, 7.68e6, 25), (122.88e6, 3.84e6, 15)]
MAPS = [(0, 0), (1, 0), (2, 2), (0, 1)]
N_OUT = 1300   # two and a half runs of 512


def _raw(rng, n, nant, fmt):
    if fmt == la.FILE_CF32:
        return (rng.standard_normal((n, nant)) + 1j * rng.standard_normal((n, nant))).astype(np.complex64), 0.0
    return rng.integers(-120, 120, (n, nant, 2)).astype((np.int16, np.int8)[fmt - 1]), 1.0 / 90.0     # (not a power of two: the conversion rounds)


def _offsets(rate_in, nof_prb):
    """-> (center, (offset 0, offset 1)): output 0 lands on the recording's centre - tuning word 0, the branch that does not mix -, output 1 near the other edge"""
    edge = rate_in / 2 - passband_hz(nof_prb)
    return 0.25 * edge, (-0.25 * edge, -1.2 * edge)


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_map_kernel_rows_are_the_unmapped_resamplers_bit_for_bit(rate_in, rate_out, nof_prb, fmt):
    """output antenna a of resample_cells_map = antenna src[a] of la.resample with center_offset_hz + offset_hz[a], on the same input: recordings of 1, 2 and 3
    antennas, every map they admit, in_base 0 and 2e10"""
    rng = np.random.default_rng(int(rate_in / 1e4) + fmt)
    B = passband_hz(nof_prb)
    center, offs = _offsets(rate_in, nof_prb)
    for first in (0, FAR):
        kw = dict(first_sample=first, first_frac=0.3, passband_hz=B)
        sp = la.resample_span(N_OUT, 0, rate_in, rate_out, **kw)
        base = max(sp["in_lo"], 0)
        for nant in (1, 2, 3):
            raw, scale = _raw(rng, sp["in_hi"] - base, nant, fmt)
            fk = dict(n_out=N_OUT, in_base=base, sample_format=fmt, sample_scale=scale)
            ref = [la.resample(raw, rate_in, rate_out, center_offset_hz=center + o, **kw, **fk) for o in offs]
            assert float(np.abs(ref[0]).max()) > 0 and not _eq(ref[0], ref[1])
            for src in MAPS:
                if max(src) >= nant:
                    with pytest.raises(ValueError):
                        la.resample_cells_map(raw, rate_in, [dict(rate_out=rate_out, center_offset_hz=center, src=src, offset_hz=offs, **kw)], **fk)
                    continue
                y, = la.resample_cells_map(raw, rate_in, [dict(rate_out=rate_out, center_offset_hz=center, src=src, offset_hz=offs, **kw)], **fk)
                assert y.shape == (2, N_OUT)
                for a in (0, 1):
                    assert _eq(y[a], ref[a][src[a]]), (first, nant, src, a)
            y, = la.resample_cells_map(raw, rate_in, [dict(rate_out=rate_out, center_offset_hz=center, src=(nant - 1,), offset_hz=offs[1:], **kw)], **fk)     # one output
            assert y.shape == (1, N_OUT) and _eq(y[0], ref[1][nant - 1])


@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS[1:3])
def test_one_mapped_call_and_three_pieces_are_bit_identical(rate_in, rate_out, nof_prb):
    rng = np.random.default_rng(3)
    B = passband_hz(nof_prb)
    center, offs = _offsets(rate_in, nof_prb)
    kw = dict(first_sample=FAR, first_frac=0.4375, passband_hz=B)
    sp = la.resample_span(N_OUT, 0, rate_in, rate_out, **kw)
    raw, _ = _raw(rng, sp["in_hi"] - sp["in_lo"], 2, la.FILE_CF32)
    cell = dict(rate_out=rate_out, center_offset_hz=center, src=(1, 0), offset_hz=offs, **kw)
    whole, = la.resample_cells_map(raw, rate_in, [cell], n_out=N_OUT, in_base=sp["in_lo"])
    parts = []
    for a, b in ((0, 1), (1, 513), (513, N_OUT)):
        p = la.resample_span(b - a, 0, rate_in, rate_out, out_first=a, **kw)
        parts.append(la.resample_cells_map(raw[p["in_lo"] - sp["in_lo"]:p["in_hi"] - sp["in_lo"]], rate_in, [dict(cell, out_first=a)], n_out=b - a, in_base=p["in_lo"])[0])
    assert _eq(whole, np.concatenate(parts, axis=1))


@pytest.mark.parametrize("rate_in,outs", [(30.72e6, ((7.68e6, 25), (15.36e6, 50))), (61.44e6, ((7.68e6, 25), (30.72e6, 100)))])
def test_a_mapped_and_an_identity_cell_of_different_geometry_in_one_launch(rate_in, outs):
    """30.72 MS/s: both cells in the ordinary run (ratios 4 and 2, one launch of k_resample_map); 61.44 MS/s: ratio 8 beside ratio 2, its two launches"""
    rng = np.random.default_rng(4)
    (ra, pa), (rb, pb) = outs
    center, offs = _offsets(rate_in, pa)
    fb = 0.5 * (rate_in / 2 - passband_hz(pb))
    n_in = max(la.resample_span(n, 0, rate_in, r, 100, 0.25, passband_hz=passband_hz(p))["in_hi"] for n, r, p in ((N_OUT, ra, pa), (2000, rb, pb)))
    raw, _ = _raw(rng, n_in, 3, la.FILE_CF32)
    a = dict(rate_out=ra, first_sample=100, first_frac=0.25, passband_hz=passband_hz(pa), center_offset_hz=center, n_out=N_OUT)
    b = dict(rate_out=rb, first_sample=100, first_frac=0.25, passband_hz=passband_hz(pb), center_offset_hz=fb, n_out=2000)
    ya, yb = la.resample_cells_map(raw, rate_in, [dict(a, src=(2, 0), offset_hz=offs), b])
    assert ya.shape == (2, N_OUT) and yb.shape == (3, 2000)
    plain = la.resample_cells(raw, rate_in, [dict(a, center_offset_hz=center + offs[0]), dict(a, center_offset_hz=center + offs[1]), b])
    assert _eq(ya[0], plain[0][2]) and _eq(ya[1], plain[1][0]) and _eq(yb, plain[2])
    yb2, ya2 = la.resample_cells_map(raw, rate_in, [b, dict(a, src=(2, 0), offset_hz=offs)])     # the other order
    assert _eq(ya2, ya) and _eq(yb2, yb)


RING = 4096


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb,n_out", [(30.72e6, 7.68e6, 25, 600), (61.44e6, 7.68e6, 25, 480)])
def test_ring_map_kernels_equal_the_linear_ones_at_the_end_of_the_ring(rate_in, rate_out, nof_prb, n_out, fmt):
    """a 4096-sample ring whose end falls on the first, a middle and the last sample the launch stages, near sample 12288 and 2e10 samples in"""
    rng = np.random.default_rng(5 + fmt)
    B = passband_hz(nof_prb)
    center, offs = _offsets(rate_in, nof_prb)
    sp0 = la.resample_span(n_out, 0, rate_in, rate_out, RING * 3, 0.0, passband_hz=B)
    n_in, back = sp0["in_hi"] - sp0["in_lo"], RING * 3 - sp0["in_lo"]      # what the launch reads, and how far in front of first_sample it starts
    assert n_in <= RING
    raw, scale = _raw(rng, n_in, 2, fmt)
    for far in (RING * 3, FAR - FAR % RING):
        for k in (0, n_in // 2, n_in - 1):        # the ring ends behind sample lo + k - 1 of the window
            first = far - k + back
            sp = la.resample_span(n_out, 0, rate_in, rate_out, first, 0.0, passband_hz=B)
            assert (sp["in_lo"] + k) % RING == 0 and sp["in_hi"] - sp["in_lo"] == n_in
            cells = [dict(rate_out=rate_out, first_sample=first, passband_hz=B, center_offset_hz=center, src=(1, 0), offset_hz=offs),
                     dict(rate_out=rate_out, first_sample=first, passband_hz=B, center_offset_hz=center + offs[1])]
            fk = dict(n_out=n_out, in_base=sp["in_lo"], sample_format=fmt, sample_scale=scale)
            lin = la.resample_cells_map(raw, rate_in, cells, **fk)
            ring = la.resample_cells_ring_map(raw, rate_in, cells, RING, **fk)
            assert float(np.abs(lin[0]).max()) > 0 and lin[0].shape == (2, n_out) and lin[1].shape == (2, n_out)
            assert _eq(ring[0], lin[0]) and _eq(ring[1], lin[1]), (far, k)
            assert _eq(lin[0][1], lin[1][0])


# ---- end to end ----
def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


def _ul_phy(sc):
    phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=16, pcapwriter=la.PcapWriter(None))
    assert phy.set_sampling(la.RATES_3GPP) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"]) and phy.setUlConfig(3, 5)
    return phy


@contextlib.contextmanager
def _block(n):
    """LSN_FILE_BLOCK = n inside: small block buffers, and blocks that divide neither 12 nor 20 subframes evenly"""
    old = os.environ.get("LSN_FILE_BLOCK")
    os.environ["LSN_FILE_BLOCK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LSN_FILE_BLOCK", None)
        else:
            os.environ["LSN_FILE_BLOCK"] = old


def test_identity_map_gives_the_unmapped_replays_records():
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording("two_cells_a")
    with tempfile.TemporaryDirectory() as td, _block(5):
        path = os.path.join(td, "c.cf32")
        f.astype(np.complex64).tofile(path)
        got = []
        for src in (None, (0, 1)):
            phy = _phy(sc, **opt)
            assert src is None or phy.set_antenna_map(src)
            assert phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, nof_antennas=2) == 12
            got.append(gpu_records(phy))
            phy.close()
    assert got[0] == orecs and got[1] == got[0]


def _pieces(raw, sizes):
    pos = 0
    for n in itertools.cycle(sizes):
        if pos >= len(raw):
            return
        yield raw[pos:pos + n]
        pos += n


@pytest.mark.parametrize("name", ["30", "61"])
def test_baseline_two_antenna_recording_replays_unmapped(name):
    """the same UL_MODE capture as an ordinary two-antenna recording, both antennas at one offset, through the unmapped path: passes without the antenna map"""
    sc, tti0, orecs, otrace, rate_in, fc, _ = ul_recording(name)
    nsf = UL_RECORDINGS[name][0]
    assert len(orecs) == UL_RECORDS[name] and edge_blocks(otrace) == [] and failed_records(orecs) == []
    with tempfile.TemporaryDirectory() as td, _block(16):
        path = os.path.join(td, "two.cf32")
        ul_baseline(name).astype(np.complex64).tofile(path)
        phy = _ul_phy(sc)
        try:
            assert phy.process_file_rate(path, rate_in, center_offset_hz=fc, start_tti=tti0, offset_time=LEAD, update_meta_period=25) == nsf
            g = gpu_records(phy)
        finally:
            phy.close()
    assert g == orecs, "baseline %s: %d records vs %d" % (name, len(g), len(orecs))


def _dl_phy(sc):
    phy = la.Phy(nof_rx_antennas=1, max_batch=16, pcapwriter=la.PcapWriter(None))
    assert phy.set_sampling(la.RATES_3GPP) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
    return phy


@contextlib.contextmanager
def _phys(*makers):
    """fresh Phys - a Phy keeps what it learnt of a cell's UEs, the oracle's worker starts with nothing -, closed behind the block"""
    phys = [m() for m in makers]
    try:
        yield phys
    finally:
        for p in phys:
            p.close()


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
@pytest.mark.parametrize("name", ["30", "61"])
def test_ul_mode_from_one_antenna(name, fmt):
    """downlink at +f and uplink at -f of ONE antenna, src = (0, 0), offsets (0, -2 f): process_file_rate, process_file_cells (the 61.44 MS/s recording together
    with an unmapped one-antenna downlink Phy in the same pass) and a Stream pushed whole and in pieces of 1 / 7919 / 33 samples -> the oracle's records"""
    sc, tti0, orecs, otrace, rate_in, fc, f = ul_recording(name)
    nsf = UL_RECORDINGS[name][0]
    assert len(orecs) == UL_RECORDS[name] and sum(1 for r in orecs if r[1] == 0) >= 1
    raw, scale, _ = quantise(f, fmt)
    kw = dict(center_offset_hz=fc, start_tti=tti0, offset_time=LEAD, update_meta_period=25)
    dkw = dict(center_offset_hz=fc, start_tti=tti0, offset_time=LEAD)
    fk = dict(nof_antennas=1, sample_format=fmt, sample_scale=scale)

    def mapped():
        phy = _ul_phy(sc)
        assert phy.set_antenna_map(src=(0, 0), offset_hz=(0.0, -2.0 * fc))
        return phy
    with tempfile.TemporaryDirectory() as td, _block(16):
        path = os.path.join(td, "one.raw")
        raw.tofile(path)
        with _phys(mapped) as (phy,):
            assert phy.process_file_rate(path, rate_in, **fk, **kw) == nsf
            g = gpu_records(phy)
            assert g == orecs, "process_file_rate %s fmt %d: %d records vs %d" % (name, fmt, len(g), len(orecs))
        if name == "61":
            with _phys(lambda: _dl_phy(sc)) as (dl,):
                assert dl.process_file_rate(path, rate_in, **fk, **dkw) == nsf
                alone = gpu_records(dl)
                assert len(alone) >= 10
            with _phys(mapped, lambda: _dl_phy(sc)) as (phy, dl):
                done, status = la.process_file_cells(path, rate_in, [(phy, kw), (dl, dkw)], with_status=True, **fk)
                assert done == [nsf, nsf] and status == [0, 0]
                g = gpu_records(phy)
                assert gpu_records(dl) == alone
        else:
            with _phys(mapped) as (phy,):
                assert la.process_file_cells(path, rate_in, [(phy, kw)], **fk) == [nsf]
                g = gpu_records(phy)
        assert g == orecs, "process_file_cells %s fmt %d: %d records vs %d" % (name, fmt, len(g), len(orecs))
        for sizes in ((len(raw),), (1, 7919, 33)):
            with _phys(mapped) as (phy,):
                with la.Stream(rate_in, [(phy, kw)], block_subframes=5, **fk) as st:
                    for piece in _pieces(raw, sizes):
                        st.push(piece)
                    assert st.flush() == [nsf]
                    s = st.status()
                    assert s["failed"] == 0 and s["status"] == [0] and s["samples_pushed"] == len(raw)
                g = gpu_records(phy)
            assert g == orecs, "stream %s fmt %d pieces %s: %d records vs %d" % (name, fmt, sizes[:3], len(g), len(orecs))


def test_two_of_four_antennas():
    """antennas 2, 3 of a four-antenna 15.36 MS/s recording hold the cell, 0 and 1 noise: src = (2, 3) returns the oracle's records, src = (0, 1) none, unmapped the
    recording is refused; LSN_TTI_FROM_MIB through the map finds the stream's TTI"""
    from ddc_cases import cell
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, f = four_antennas()
    _, _, iq, _, _, _ = cell("prb25_2port")
    kw = dict(center_offset_hz=FOUR_OFFSET, start_tti=tti0, offset_time=LEAD)

    def mapped(*src):
        def make():
            phy = _phy(sc, **opt)
            assert phy.set_antenna_map(src)
            return phy
        return make
    with tempfile.TemporaryDirectory() as td, _block(5):
        path = os.path.join(td, "four.cf32")
        f.astype(np.complex64).tofile(path)
        with _phys(lambda: _phy(sc, **opt)) as (phy,):
            with pytest.raises(RuntimeError):
                phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **kw)        # unmapped: four antennas are not the Phy's two
            with pytest.raises(ValueError):
                la.process_file_cells(path, FOUR_RATE, [(phy, kw)], nof_antennas=4)
            assert gpu_records(phy) == []
            assert phy.set_antenna_map((2, 3))                                       # ... and the same Phy with the map
            assert phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **kw) == FOUR_NSF
            assert gpu_records(phy) == orecs
        with _phys(mapped(2, 3)) as (phy,):
            assert la.process_file_cells(path, FOUR_RATE, [(phy, kw)], nof_antennas=4) == [FOUR_NSF]
            assert gpu_records(phy) == orecs
        with _phys(mapped(0, 1)) as (phy,):
            assert phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **kw) == FOUR_NSF
            assert gpu_records(phy) == []
        # the first subframe 0 of a radio frame, the TTI from its MIB - read from the mapped samples
        first0 = (10 - tti0 % 10) % 10
        _, _, want = run_oracle(sc, tti0 + first0, iq[first0:], taps=False, **opt)
        want = oracle_records(want)
        with _phys(mapped(2, 3)) as (phy,):
            n = phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **dict(kw, start_tti=la.TTI_FROM_MIB, offset_time=LEAD + first0 * 15360))
            assert n == FOUR_NSF - first0
            g = gpu_records(phy)
            assert len(want) >= 5 and g == want, (len(g), len(want))
            assert phy.set_antenna_map(None)
            with pytest.raises(RuntimeError):
                phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **kw)        # off again: refused again
        with _phys(mapped(0, 1)) as (phy,):                                          # ... and on the noise antennas no MIB is found
            with pytest.raises(RuntimeError):
                phy.process_file_rate(path, FOUR_RATE, nof_antennas=4, **dict(kw, start_tti=la.TTI_FROM_MIB, offset_time=LEAD + first0 * 15360))
            assert gpu_records(phy) == []


def test_refusals_decode_nothing_and_leave_the_phy_usable():
    sc, tti0, orecs, otrace, rate_in, fc, f = ul_recording("30")
    nsf = UL_RECORDINGS["30"][0]
    L = la.lib()
    good = (0.0, -2.0 * fc)
    kw = dict(center_offset_hz=fc, start_tti=tti0, offset_time=LEAD, update_meta_period=25)
    B = passband_hz(25)
    edge = rate_in / 2 - B
    with tempfile.TemporaryDirectory() as td, _block(16):
        path = os.path.join(td, "one.cf32")
        f.astype(np.complex64).tofile(path)
        phy = _ul_phy(sc)
        one = _phy(dict(sc, nof_rx=1), batch=16)
        multi = la.Phy(nof_rx_antennas=2, max_batch=4, pcapwriter=la.PcapWriter(None), devices=[0, 0])
        try:
            # the setter: the map stays as it was
            assert phy.set_antenna_map((0, 0), good)
            assert not phy.set_antenna_map((0,), (0.0,)) and not phy.set_antenna_map((0, 0, 0), (0.0, 0.0, 0.0))         # nof_out is not the Phy's antennas: 1, 3
            assert not phy.set_antenna_map((0, 8), good) and not phy.set_antenna_map((0, 0), (0.0, float("nan"))) and not phy.set_antenna_map((0, 0), (float("inf"), 0.0))
            assert not one.set_antenna_map((0, 0), good) and one.set_antenna_map((0,), (0.0,)) and one.set_antenna_map(None)
            m = la.antenna_map((0, 0), good)
            for size in (0, 24, 40):
                m.struct_size = size
                assert L.lsn_phy_set_antenna_map(phy._h, C.byref(m)) == INVALID
            m = la.antenna_map()
            assert L.lsn_phy_set_antenna_map(phy._h, C.byref(m)) == INVALID                                            # nof_out = 0
            assert not multi.set_antenna_map((0, 0), good)                                                          # a lsn_phy_create_multi handle
            done = C.c_uint64(99)

            def refused(center, nant=1):
                cfg = la.FileCfg(nant, LEAD, 0.0, la.FILE_CF32, 0.0)
                fr = la.FileRate(C.sizeof(la.FileRate), 0, rate_in, 0.0, center)
                rc = L.lsn_phy_process_file_rate(phy._h, os.fsencode(path), C.byref(cfg), C.byref(fr), tti0, 0, 25, C.byref(done))
                return rc == INVALID and done.value == 0 and gpu_records(phy) == []
            # the rule per output
            assert refused(edge + 1.0) and refused(fc + edge) and refused(float("nan")) and refused(float("inf"))
            assert refused(fc, nant=0) and refused(fc, nant=9)                                                          # the recording's antennas: 1 .. 8
            assert phy.set_antenna_map((0, 1), good) and refused(fc)                                                    # a source the recording does not have
            assert phy.set_antenna_map((0, 0), (0.0, -2.0 * fc - edge)) and refused(fc)                                  # output 1 outside the recording
            assert phy.set_antenna_map((0, 0), good)
            # a map together with the channel filter
            assert phy.set_channel_filter(4e6) and refused(fc)
            with pytest.raises(ValueError):
                la.process_file_cells(path, rate_in, [(phy, kw)], nof_antennas=1)
            with pytest.raises(ValueError):
                la.Stream(rate_in, [(phy, kw)], nof_antennas=1)
            assert phy.set_channel_filter(0.0)
            # lsn_phy_process_file has no rate and takes no map
            with pytest.raises(RuntimeError):
                phy.process_file(path, start_tti=tti0, nof_antennas=1)
            # the multi-cell pass: an unmapped Phy still needs the recording's antenna count; a mapped one its sources
            with pytest.raises(ValueError):
                la.process_file_cells(path, rate_in, [(phy, kw), (one, kw)], nof_antennas=2)
            with pytest.raises(ValueError):
                la.process_file_cells(path, rate_in, [(phy, dict(kw, center_offset_hz=fc + edge))], nof_antennas=1)
            assert gpu_records(phy) == [] and gpu_records(one) == []
            # the timing loop, re-acquisition and frame sync on a stream that has a mapped cell
            with la.Stream(rate_in, [(phy, kw)], nof_antennas=1, block_subframes=5) as st:
                with pytest.raises(ValueError):
                    st.track()
                with pytest.raises(ValueError):
                    st.reacquire()
                with pytest.raises(ValueError):
                    st.frame_sync()
                assert st.flush() == [0]
            with pytest.raises(ValueError):
                la.Stream(rate_in, [(phy, kw)], nof_antennas=1, block_subframes=5, track={})
            with pytest.raises(ValueError):                                                                              # TTI_FROM_MIB stays refused on a stream
                la.Stream(rate_in, [(phy, dict(kw, start_tti=la.TTI_FROM_MIB))], nof_antennas=1)
            assert gpu_records(phy) == []
            # ... and the Phy is usable: the good replay
            assert phy.process_file_rate(path, rate_in, nof_antennas=1, **kw) == nsf
            assert gpu_records(phy) == orecs
        finally:
            for p in (phy, one, multi):
                p.close()
