"""Carrier scan on the GPU (k_chan_bank, k_pss_corr with its channel dimension, k_scan_peaks; lsn_carrier_scan, lsn_file_carrier_scan, lsn_carrier_channel)
against the float64 model of tests/scan_model.py, against itself (batches, one call, pieces), against the cell search and its oracle, and end to end: the two
cells of the 61.44 MS/s recording found from nothing but the rate, their MIBs decoded and both replayed to their oracle records."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
import scan_model as M
from ddc_cases import quantise, recording
from resample_cases import FAR, LEAD
from test_sync_oracle import oracle_cell_search

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
FIELDS = ("found", "cell_id", "n_id_2", "n_id_1", "sf_idx", "pss_pos", "sf_start", "cp")
FLOATS = ("pss_peak", "pss_p2avg", "sss_metric", "sss_second", "cfo_hz", "cfo_coarse_hz")


def same(g, o):
    assert [getattr(g, f) for f in FIELDS] == [getattr(o, f) for f in FIELDS], ([getattr(g, f) for f in FIELDS], [getattr(o, f) for f in FIELDS])
    a = np.array([getattr(g, f) for f in FLOATS], dtype=np.float32)
    b = np.array([getattr(o, f) for f in FLOATS], dtype=np.float32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a, b)


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], {1: 0, 3: 1, 6: 2, 12: 3}[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate_in", [7.68e6, 25e6, 61.44e6, 122.88e6])
def test_kernel_against_the_model_within_the_dot_product_and_nco_bound(rate_in, fmt):
    """|y_gpu - y_model| <= ((T + 2) 2^-24 + 2^-18) sum_j |c_j| |x_j| per output: the float32 dot product of T terms plus the mixer, the bound derived in DESIGN
    3.1b and used by test_gpu_ddc.py - here with T up to 764.  Hypotheses: the largest |f_k| of the raster with both signs (one antenna, from sample 0) and
    100 kHz (two antennas, far into the recording, a fractional start)"""
    rng = np.random.default_rng(int(rate_in) % 1000 + fmt + 70)
    n_out = 3000
    hyp = M.hypotheses(rate_in)
    for (nant, first, frac), fs in (((1, 0, 0.0), (hyp[-1][1], hyp[0][1])), ((2, FAR, 0.3), (100e3,))):
        plan = M.ChannelPlan(rate_in, first, frac)
        lo, hi = plan.span(0, n_out)
        base = max(lo, 0)
        n_in = hi - base
        x = (rng.standard_normal((n_in, nant)) + 1j * rng.standard_normal((n_in, nant))) / np.sqrt(2)
        if fmt == la.FILE_CF32:
            raw = x.astype(np.complex64)
            x32, scale = raw, 0.0
        else:
            full, dt, scale = ((32767, np.int16, np.float32(1.0 / 9000.0)), (127, np.int8, np.float32(1.0 / 30.0)))[fmt - 1]   # not powers of two: the product rounds
            raw = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) / float(scale)), -full, full).astype(dt)
            v = raw.astype(np.float32) * scale
            x32 = v[..., 0] + 1j * v[..., 1]
        for f0 in fs:
            y = la.carrier_channel(raw, rate_in, f0, n_out=n_out, first_sample=first, first_frac=frac, in_base=base, sample_format=fmt, sample_scale=float(scale))
            ref, bound = M.channel(x32, rate_in, f0, n_out, in_base=base, first_sample=first, first_frac=frac, with_bound=True)
            assert y.shape == (nant, n_out)
            err = np.abs(y.T.astype(np.complex128) - ref)
            lim = ((plan.taps + 2) * 2.0 ** -24 + 2.0 ** -18) * bound
            worst = float(np.max(err / np.maximum(lim, 1e-300)))
            print("channel %.2f -> 1.92 MS/s fmt %d x%d offset %+.1f kHz first %d: T = %d, largest error / bound = %.3f" %
                  (rate_in / 1e6, fmt, nant, f0 / 1e3, first, plan.taps, worst))
            assert np.all(err <= lim), worst
            assert float(np.sqrt(np.mean(np.abs(ref) ** 2))) > 0.01    # (the comparison is not one of zeros)


def test_one_sample_one_value_scan_one_call_and_pieces():
    """25 MS/s (fractional phases): the channel a scan of seven hypotheses correlated for one of them, the channel of that offset in one call, and the same in
    pieces are the same bits; so is a scan of that hypothesis alone; and far into the recording one call equals its pieces"""
    rate, P, f0 = 25e6, 1, 200e3
    plan = la.carrier_scan_plan(rate, nof_periods=P)
    n_ch, n_in = plan["nof_channel_samples"], plan["nof_input_samples"]
    rng = np.random.default_rng(12)
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    found, metric = la.carrier_scan(x, rate, with_metric=True, nof_periods=P, f_lo_hz=-350e3, f_hi_hz=350e3)
    assert found == [] and [m.k for m in metric] == [-3, -2, -1, 0, 1, 2, 3]
    m = metric[5]
    assert m.f_hz == f0 and m.tuning_word == M.tuning_word(f0, rate)
    ch = la.carrier_channel(x, rate, f0, n_out=n_ch)
    rc, s, corr = la.cell_search(ch[0], 6, nof_periods=P, with_corr=True)
    assert rc == 0
    # the scan's peak IS the cell search's on that channel: value, root and lag
    assert (m.root, m.lag) == (s.n_id_2, s.pss_pos) and bits(np.float32(m.peak)) == bits(np.float32(s.pss_peak)), (m.root, m.lag, m.peak, s.n_id_2, s.pss_pos, s.pss_peak)
    assert abs(m.p2avg - s.pss_p2avg) <= 1e-6 * s.pss_p2avg
    # ... and the model's, in float64
    r_, n_, pk, p2 = M.metric(M.correlate(M.channel(x, rate, f0, n_ch), P))
    assert (r_, n_) == (m.root, m.lag) and abs(pk - m.peak) <= 1e-3 * pk and abs(p2 - m.p2avg) <= 1e-3 * p2, (r_, n_, pk, p2)
    # the hypothesis alone, and in a scan with another batch around it
    for kw in (dict(f_lo_hz=f0, f_hi_hz=f0), dict(f_lo_hz=150e3, f_hi_hz=1e6)):
        _, alone = la.carrier_scan(x, rate, with_metric=True, nof_periods=P, **kw)
        a = [h for h in alone if h.k == 2][0]
        assert bytes(a) == bytes(m)
    mp = M.ChannelPlan(rate)
    parts = []
    for a, b in ((0, 1), (1, 97), (97, 4000), (4000, n_ch)):
        lo, hi = mp.span(a, b - a)
        lo = max(lo, 0)
        parts.append(la.carrier_channel(x[lo:hi], rate, f0, n_out=b - a, in_base=lo, out_first=a))
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(ch))
    # far from 0, two antennas
    first, frac, n_out = FAR, 0.4375, 6000
    mp = M.ChannelPlan(rate, first, frac)
    lo, hi = mp.span(0, n_out)
    x2 = (rng.standard_normal((hi - lo, 2)) + 1j * rng.standard_normal((hi - lo, 2))).astype(np.complex64)
    whole = la.carrier_channel(x2, rate, -f0 * 0.77, n_out=n_out, first_sample=first, first_frac=frac, in_base=lo)
    parts = []
    for a, b in ((0, 1), (1, 2), (2, 513), (513, 6000)):
        plo, phi = mp.span(a, b - a)
        parts.append(la.carrier_channel(x2[plo - lo:phi - lo], rate, -f0 * 0.77, n_out=b - a, first_sample=first, first_frac=frac, in_base=plo, out_first=a))
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))
    assert float(np.abs(whole).max()) > 0


def _check_two_cells(found, metric, x, fmt=la.FILE_CF32, scale=0.0):
    _, truth = M.two_cell_recording()
    hyp, met, acc = M.model_scan("cells")
    n_ch = M.channel_samples(2)
    assert [c.center_offset_hz for c in found] == [hyp[i][1] for i in acc] == [1.5e6, -1.4e6], [(c.center_offset_hz, c.scan_p2avg) for c in found]
    assert [m.k for m in metric] == [h[0] for h in hyp]
    for c, t, i in zip(found, truth, acc):
        s = c.search
        assert c.center_offset_hz == t["f_hz"] and c.k == hyp[i][0]
        assert (s.found, s.cell_id, s.cp, s.sf_idx) == (1, t["cell_id"], t["cp"], t["sf_idx"]), (s.found, s.cell_id, s.cp, s.sf_idx, s.sf_start)
        assert abs(int(s.sf_start) - t["sf_start"]) <= 2, (s.sf_start, t["sf_start"])
        ch = la.carrier_channel(x, M.RATE_TWO, c.center_offset_hz, n_out=n_ch, sample_format=fmt, sample_scale=scale)
        rc, direct = la.cell_search(ch[0], 6, nof_periods=2)
        assert rc == 1 and bytes(direct) == bytes(s)
        ro, so, _ = oracle_cell_search(ch[0], 6, 2, -1, 20.0)
        assert ro == 1
        same(s, so)
        assert abs(c.scan_p2avg - s.pss_p2avg) <= 1e-6 * s.pss_p2avg, (c.scan_p2avg, s.pss_p2avg)
        assert (c.scan_root, c.scan_lag) == (s.n_id_2, s.pss_pos)
        if fmt == la.FILE_CF32:
            assert (met[i][0], met[i][1]) == (c.scan_root, c.scan_lag) and abs(met[i][3] - c.scan_p2avg) <= 1e-3 * met[i][3], (met[i], c.scan_p2avg)


def test_scan_against_the_cell_search_on_the_two_cell_recording():
    """the 7.68 MS/s recording of tests/scan_model.py (a 6-block cell at +1.5 MHz, a 15-block cell at -1.4 MHz 10 dB weaker): exactly the two planted carriers;
    each carrier's lsn_cell_search_t is the cell search's on lsn_carrier_channel's samples bit for bit, which is the oracle's; the scan's own p2avg agrees to 1e-6;
    noise of the same length gives none; the same recording as an sc16 file through lsn_file_carrier_scan"""
    x, truth = M.two_cell_recording()
    found, metric = la.carrier_scan(x, M.RATE_TWO, with_metric=True)
    _check_two_cells(found, metric, x)
    noise, nmet = la.carrier_scan(M.noise_recording(), M.RATE_TWO, with_metric=True)
    assert noise == [], "largest p2avg %.2f" % max(m.p2avg for m in nmet)
    assert max(m.p2avg for m in nmet) < 20.0
    raw, scale, _ = quantise(x.astype(np.complex128), 1)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "two.sc16")
        pad = np.zeros((333, 2), dtype=np.int16)
        np.concatenate([pad, raw]).tofile(path)       # the recording starts 333 samples into the file
        found, metric = la.file_carrier_scan(path, M.RATE_TWO, sample_format=la.FILE_SC16, sample_scale=scale, offset_time=333, with_metric=True)
        _check_two_cells(found, metric, raw, la.FILE_SC16, scale)
        in_mem, mem_metric = la.carrier_scan(raw, M.RATE_TWO, sample_format=la.FILE_SC16, sample_scale=scale, with_metric=True)
        assert [bytes(c) for c in in_mem] == [bytes(c) for c in found] and [bytes(m) for m in mem_metric] == [bytes(m) for m in metric]


def test_invalid_arguments_are_refused():
    L = la.lib()
    x = M.noise_recording()
    n = len(x)
    out = (la.Carrier * 4)()
    good = la.carrier_scan_cfg(M.RATE_TWO)

    def rc(cfg, ptr=x.ctypes.data, n_in=n, cap=4, carriers=out):
        return L.lsn_carrier_scan(0, ptr, 0, n_in, C.byref(cfg), carriers, cap, None)

    assert rc(good) == 0
    need = la.carrier_scan_plan(M.RATE_TWO)["nof_input_samples"]
    assert rc(good, n_in=need) == 0 and rc(good, n_in=need - 1) == INVALID          # the head is shorter than the scan reads
    assert rc(good, ptr=None) == INVALID and rc(good, carriers=None) == INVALID
    for kw in (dict(nof_antennas=0), dict(nof_antennas=9), dict(nof_antennas=2, antenna=2), dict(sample_format=3), dict(nof_periods=17), dict(raster_hz=1.0),
               dict(f_lo_hz=10e3, f_hi_hz=90e3), dict(threshold=-1.0), dict(min_spacing_hz=-1.0), dict(raster_offset_hz=float("nan"))):
        assert rc(la.carrier_scan_cfg(M.RATE_TWO, **kw)) == INVALID, kw
    for rate in (1.0e6, 123e6, float("nan")):
        assert rc(la.carrier_scan_cfg(rate)) == INVALID, rate
    bad = la.carrier_scan_cfg(M.RATE_TWO)
    bad.struct_size += 8
    assert rc(bad) == INVALID
    assert L.lsn_carrier_scan(99, x.ctypes.data, 0, n, C.byref(good), out, 4, None) == la.LSN_ERROR_NO_DEVICE
    fc = la.FileCfg(1, 0, 0.0, la.FILE_CF32, 0.0)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "short.cf32")
        x[:need - 1].tofile(path)
        assert L.lsn_file_carrier_scan(0, os.fsencode(path), C.byref(fc), C.byref(good), out, 4, None) == INVALID       # a file shorter than the head
        assert L.lsn_file_carrier_scan(0, os.fsencode(os.path.join(td, "none")), C.byref(fc), C.byref(good), out, 4, None) == INVALID
        assert L.lsn_file_carrier_scan(0, None, C.byref(fc), C.byref(good), out, 4, None) == INVALID
        neg = la.FileCfg(1, -1, 0.0, la.FILE_CF32, 0.0)
        assert L.lsn_file_carrier_scan(0, os.fsencode(path), C.byref(neg), C.byref(good), out, 4, None) == INVALID
    # the channel: an input that does not hold what the outputs read, an offset outside the recording, a wrong struct_size
    y = np.zeros((1, 100), dtype=np.complex64)
    cfg = la._channel_cfg(1, M.RATE_TWO, 1e6, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
    assert L.lsn_carrier_channel(0, x.ctypes.data, 0, n, C.byref(cfg), y.ctypes.data, 0, 100) == 0
    assert L.lsn_carrier_channel(0, x.ctypes.data, 0, 100, C.byref(cfg), y.ctypes.data, 0, 100) == INVALID
    assert L.lsn_carrier_channel(0, None, 0, n, C.byref(cfg), y.ctypes.data, 0, 100) == INVALID
    cfg = la._channel_cfg(1, M.RATE_TWO, 3.3e6, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
    assert L.lsn_carrier_channel(0, x.ctypes.data, 0, n, C.byref(cfg), y.ctypes.data, 0, 100) == INVALID
    cfg = la._channel_cfg(1, M.RATE_TWO, 1e6, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
    cfg.struct_size = 8
    assert L.lsn_carrier_channel(0, x.ctypes.data, 0, n, C.byref(cfg), y.ctypes.data, 0, 100) == INVALID


def test_the_whole_chain_two_cells_found_from_nothing_but_the_rate():
    """ddc_cases.recording("two_cells_a"): 61.44 MS/s, two 100-block cells 9.9 MHz either side of the centre, 12 subframes (so one period).  The scan, handed
    the file and its rate, finds exactly +9.9 MHz and -9.9 MHz with the two cell ids; carrier_mib on each carrier's channel says 100 blocks and the cell's ports;
    each cell replayed with the FOUND center_offset_hz gives its oracle records"""
    from parity import gpu_records
    a, b = recording("two_cells_a"), recording("two_cells_b")
    rate_in, f = a[5], a[-1]
    assert rate_in == 61.44e6
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "two.cf32")
        cap = f.astype(np.complex64)
        cap.tofile(path)
        nant = cap.shape[1]
        found = la.file_carrier_scan(path, rate_in, nof_antennas=nant, nof_periods=1)
        got = sorted((c.center_offset_hz, c.search.cell_id) for c in found)
        assert got == sorted((r[7], r[0]["cell_id"]) for r in (a, b)), [(c.center_offset_hz, c.search.cell_id, c.scan_p2avg) for c in found]
        assert sorted(g[0] for g in got) == [-9.9e6, 9.9e6]
        for c in found:
            r = a if c.center_offset_hz == a[7] else b
            sc, tti0, orecs, opt = r[0], r[1], r[2], r[4]
            assert c.search.found == 1 and c.search.cp == sc.get("cp", 0)
            ch = la.carrier_channel(cap, rate_in, c.center_offset_hz)
            mib = la.carrier_mib(ch, c.search)
            assert mib is not None and mib["nof_prb"] == 100 and mib["nof_ports"] == sc["nof_ports"], mib
            phy = _phy(sc, **opt)
            n = phy.process_file_rate(path, rate_in, center_offset_hz=c.center_offset_hz, start_tti=tti0, offset_time=LEAD)
            g = gpu_records(phy)
            phy.close()
            assert n == 12 and len(orecs) >= 10 and g == orecs, (n, len(g), len(orecs))
