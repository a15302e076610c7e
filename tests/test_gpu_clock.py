"""The sample-clock estimate on the GPU (k_pss_track: lsn_clock_track, lsn_clock_estimate, lsn_file_clock_estimate) against tests/clock_model.py - the
correlation bit for bit, the observations and fits of every round - on PSS trains whose clock error is known exactly, and end to end: cell search ->
clock estimate -> replay of recordings whose clock is off, to the oracle's records.

Windows of the C ABI are centre +- half_width, an odd number of lags: 63 and 65 lags bracket the 64-lane tile (the first tile of the 65 is exactly full, its
second holds one lag), 127 / 129 the two-tile edge, 301 is five tiles.  Errors the GPU path reaches (samples at the end of the recording): profiles/clock_estimate.txt."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
import clock_model as M
from clock_cases import TRAINS, drifted_capture, end_error, train
from parity import gpu_records
from resample_cases import CASES, LEAD, TAIL, native_stream, sinc_convert
from resample_model import passband_hz

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2
GEOM = [(6, la.RATES_3GPP, 128), (25, la.RATES_SRSRAN, 384), (100, la.RATES_3GPP, 2048)]


def _cfg(nof_prb, rates, pss_pos, n_id_2=1, cfo_hz=0.0, max_ppm=200.0, max_periods=0, sf_start=0):
    return la.ClockCfg(C.sizeof(la.ClockCfg), nof_prb, rates, n_id_2, pss_pos, cfo_hz, max_ppm, max_periods, sf_start)


def _lib_replica(cfg, N):
    r = np.zeros(N, dtype=np.complex64)
    assert la.lib().lsn_clock_replica(C.byref(cfg), r.ctypes.data) == 0
    return r


@pytest.mark.parametrize("nof_prb,rates,N", GEOM)
def test_track_is_bit_identical_to_the_model(nof_prb, rates, N):
    import torch
    rng = np.random.default_rng(N)
    cfg = _cfg(nof_prb, rates, 500, n_id_2=2, cfo_hz=1234.5)
    r = _lib_replica(cfg, N)
    halves = [4, 0, 31, 32, 64, 150]                      # 9, 1, 63, 65, 129 and 301 lags
    ns = 6 * (N + 400)
    x = (0.3 / np.sqrt(N) * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns))).astype(np.complex64)   # the replica has unit ENERGY
    centres = [4] + [q * (N + 400) + 170 for q in range(1, 5)] + [ns - N - 150]   # the first window starts at sample 0, the last ends on the last sample
    for c, d in zip(centres, (1, 0, -7, 20, -33, 60)):   # a PSS near every centre (not on it), so that the peaks are peaks
        x[c + d:c + d + N] += r
    x[centres[1]:centres[1] + N] = 0                     # the one-lag window reads nothing but zeros: e = 0, C = 0
    w = (la.ClockObs * 6)()
    for q, (c, h) in enumerate(zip(centres, halves)):
        w[q].period, w[q].centre, w[q].half_width = q, c, h
    nlag = sum(2 * h + 1 for h in halves)
    ref = M.corr(x, r, list(zip(centres, halves)))
    refc = np.concatenate(ref)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to("cuda:0")
    for ptr, on_dev in ((x.ctypes.data, 0), (d_x.data_ptr(), 1)):
        corr = np.full(nlag, -1.0, dtype=np.float32)
        assert la.lib().lsn_clock_track(0, ptr, on_dev, ns, C.byref(cfg), w, 6, corr.ctypes.data) == 0
        assert np.array_equal(corr.view(np.uint32), refc.view(np.uint32)), int(np.sum(corr.view(np.uint32) != refc.view(np.uint32)))
        for q, (c, h) in enumerate(zip(centres, halves)):
            valid, pos, peak = M.observe(ref[q], c, h)
            assert w[q].valid == valid and abs(w[q].pos - pos) <= 1e-9 and np.float32(w[q].peak) == np.float32(peak), q
    assert [int(o.valid) for o in w] == [1, 0, 1, 1, 1, 1] and abs(w[5].pos - (centres[5] + 60)) < 0.5
    # a window that does not lie inside the samples is refused
    w[5].centre += 1
    assert la.lib().lsn_clock_track(0, x.ctypes.data, 0, ns, C.byref(cfg), w, 6, None) == INVALID
    w[5].centre -= 1
    w[0].centre = 3
    assert la.lib().lsn_clock_track(0, x.ctypes.data, 0, ns, C.byref(cfg), w, 6, None) == INVALID


@functools.lru_cache(maxsize=None)
def _model(name):
    """the model's answer on a train, with the replica the library uses (lsn_clock_replica; the CPU suite checks it against the model's own)"""
    x, info = train(name)
    cfg = _cfg(6, 0, info["pss_pos"], n_id_2=info["n_id_2"], cfo_hz=info["cfo_hz"], sf_start=100)
    return M.estimate(x, info["N"], info["n_id_2"], info["pss_pos"], info["cfo_hz"], sf_start=100, rep=_lib_replica(cfg, info["N"]))


@pytest.mark.parametrize("name", sorted(TRAINS))
def test_estimate_equals_the_model_and_meets_the_half_sample_condition(name):
    x, info = train(name)
    res, obs = _model(name)
    s = la.CellSearch(n_id_2=info["n_id_2"], pss_pos=info["pss_pos"], sf_start=100, cfo_hz=info["cfo_hz"])
    est, gobs = la.clock_estimate(x, 6, s, with_obs=True)
    err = end_error(est.eps, info["eps"], len(x))
    print("clock GPU %-28s eps %+9.3f ppm -> %+9.3f ppm: %.4f sample at the end of %d samples (model %.4f); rounds %d, used %d / %d" %
          (name, info["eps"] * 1e6, est.eps * 1e6, err, len(x), end_error(res["eps"], info["eps"], len(x)), est.nof_rounds, est.nof_used, est.nof_periods))
    assert est.found == 1 == res["found"] and est.nof_rounds == res["nof_rounds"] == 3 and est.nof_used == res["nof_used"] and est.nof_periods == 120 == len(gobs)
    for g, (q, valid, c, h, pos, pk) in zip(gobs, obs):
        assert (g.period, g.valid, g.centre, g.half_width) == (q, valid, c, h) and abs(g.pos - pos) <= 1e-9 and np.float32(g.peak) == np.float32(pk)
    assert abs(est.eps - res["eps"]) * len(x) <= 1e-9 and abs(est.pss_pos0 - res["pss_pos0"]) <= 1e-9 and abs(est.sf_start - res["sf_start"]) <= 1e-9
    assert est.sample_rate_hz == 15000.0 * 128 * (1.0 + est.eps)
    assert err <= 0.5 and abs(est.pss_pos0 - info["p0"]) <= 0.5
    med = float(np.median([g.peak for g in gobs if g.valid]))
    for g in gobs:
        if g.period in info["blank"]:
            assert not g.valid or g.peak < 0.25 * med
    assert est.nof_used <= 120 - len(info["blank"])


def test_noise_only_is_not_found_and_refusals_leave_the_entry_usable():
    L = la.lib()
    rng = np.random.default_rng(5)
    ns = 100 + 40 * 9600
    x = (rng.standard_normal(ns) + 1j * rng.standard_normal(ns)).astype(np.complex64)
    out, obs = la.Clock(), (la.ClockObs * 64)()
    good = _cfg(6, 0, 100)
    assert L.lsn_clock_estimate(0, x.ctypes.data, 0, ns, C.byref(good), C.byref(out), obs, 64) == 0 and out.found == 0 and out.nof_rounds == 1
    bad = [_cfg(6, 0, 100, n_id_2=3), _cfg(7, 0, 100), _cfg(6, 5, 100), _cfg(6, 0, 100, max_ppm=0.0), _cfg(6, 0, 100, max_ppm=1000.5), _cfg(6, 0, 2)]
    for size in (0, 40, C.sizeof(la.ClockCfg) + 8):
        c = _cfg(6, 0, 100)
        c.struct_size = size
        bad.append(c)
    w = (la.ClockObs * 1)()
    w[0].centre, w[0].half_width = 5000, 4
    for c in bad:
        assert L.lsn_clock_estimate(0, x.ctypes.data, 0, ns, C.byref(c), C.byref(out), obs, 64) == INVALID
        if c.max_ppm == 200.0 and c.pss_pos == 100:
            assert L.lsn_clock_track(0, x.ctypes.data, 0, ns, C.byref(c), w, 1, None) == INVALID
    assert L.lsn_clock_estimate(0, x.ctypes.data, 0, 100 + 3 * 9600 + 100, C.byref(good), C.byref(out), obs, 64) == INVALID   # Q = 3
    assert L.lsn_clock_estimate(0, x.ctypes.data, 0, ns, C.byref(good), C.byref(out), obs, 39) == INVALID                    # obs_out too small for Q = 40
    assert L.lsn_clock_estimate(0, None, 0, ns, C.byref(good), C.byref(out), obs, 64) == INVALID
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "n.cf32")
        x.tofile(p)
        fc = la.FileCfg(1, 0, 0.0, la.FILE_CF32, 0.0)
        assert L.lsn_file_clock_estimate(0, os.fsencode(p), C.byref(fc), None, 0, C.byref(good), C.byref(out)) == 0 and out.found == 0
        assert L.lsn_file_clock_estimate(0, os.fsencode(p), C.byref(fc), None, 1, C.byref(good), C.byref(out)) == INVALID      # no such antenna
        fr = la.FileRate(C.sizeof(la.FileRate) + 8, 0, 2e6, 0.0, 0.0)
        assert L.lsn_file_clock_estimate(0, os.fsencode(p), C.byref(fc), C.byref(fr), 0, C.byref(good), C.byref(out)) == INVALID
        assert L.lsn_file_clock_estimate(0, os.fsencode(os.path.join(td, "none")), C.byref(fc), None, 0, C.byref(good), C.byref(out)) == INVALID
    # a good call behind all that
    xt, info = train("plus_3ppm")
    est = la.clock_estimate(xt, 6, la.CellSearch(n_id_2=info["n_id_2"], pss_pos=info["pss_pos"], sf_start=0, cfo_hz=0.0))
    assert est.found == 1 and end_error(est.eps, info["eps"], len(xt)) <= 0.5


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


def _write(td, f, fmt):
    if fmt == la.FILE_CF32:
        p = os.path.join(td, "c.cf32")
        f.astype(np.complex64).tofile(p)
        return p, 0.0
    scale = 2.0 ** -13
    assert float(np.abs(f.real).max()) < 3.9 and float(np.abs(f.imag).max()) < 3.9
    p = os.path.join(td, "c.sc16")
    np.round(np.stack([f.real, f.imag], axis=-1) / scale).astype(np.int16).tofile(p)
    return p, scale


@functools.lru_cache(maxsize=None)
def _stream():
    """the 25-PRB stream of the ppm cases at its own rate, and a memo of the oracle's records of its tail from subframe j on"""
    name, nsf, _ = CASES["prb25_plus_150ppm"]
    sc, tti0, iq, orecs, otrace, opt = native_stream(name, nsf)
    return sc, tti0, iq, opt, {0: orecs}


def _oracle_from(j):
    from parity import oracle_records, run_oracle
    sc, tti0, iq, opt, memo = _stream()
    if j not in memo:
        _, _, recs = run_oracle(sc, tti0 + j, iq[j:], taps=False, **opt)
        memo[j] = oracle_records(recs)
    return memo[j]


def _chain(path, fmt, scale, sc, tti0, s, file_rate, true_rate, sf_file, eps_true, nsamples, center=0.0):
    """clock estimate of the file -> replay at the measured rate from the measured subframe start -> (estimate, stream subframe the replay starts with, records)"""
    kw = dict(sample_rate=file_rate, center_offset_hz=center) if file_rate is not None else {}
    est = la.file_clock_estimate(path, 25, s, nof_antennas=sc["nof_rx"], antenna=0, sample_format=fmt, sample_scale=scale, **kw)
    assert est.found == 1 and est.nof_periods in (9, 10) and est.nof_rounds == 2
    err = end_error(est.eps, eps_true, nsamples)
    j = int(round((est.sf_start - LEAD) / sf_file))       # the stream's subframe that starts there
    print("clock GPU file fmt %d rate %s centre %+.0f: eps %+.3f ppm -> %+.3f ppm, %.4f sample at the end of %d samples; subframe start off by %+.3f" %
          (fmt, file_rate, center, eps_true * 1e6, est.eps * 1e6, err, nsamples, est.sf_start - (LEAD + j * sf_file)))
    assert err <= 0.5 and 0 <= j < 5 and (tti0 + j) % 5 == 0 and abs(est.sf_start - (LEAD + j * sf_file)) <= 0.5
    nominal = file_rate if file_rate is not None else 7.68e6
    assert abs(est.sample_rate_hz - true_rate) * nsamples / nominal <= 0.5
    phy = _phy(sc, **_stream()[3])
    n = phy.process_file(path, start_tti=tti0 + j, offset_time=int(est.sf_start), offset_time_frac=est.sf_start - int(est.sf_start), sample_format=fmt,
                         sample_scale=scale, sample_rate=est.sample_rate_hz, center_offset_hz=center, max_subframes=48 - j)
    g = gpu_records(phy)
    phy.close()
    assert n == 48 - j
    return est, j, g


@pytest.mark.parametrize("case", ["prb25_plus_150ppm", "prb25_minus_150ppm"])
def test_chain_cell_search_clock_estimate_replay_on_the_drifted_files(case):
    sc, tti0, orecs, opt, native, eps, f = drifted_capture(case)
    assert _stream()[1] == tti0 and _stream()[4][0] == orecs
    sf_file = 7680.0 * (1.0 + eps)
    rc, s = la.cell_search(f[:2 * 38400 + 512, 0].astype(np.complex64), 25, nof_periods=1)
    assert rc == 1 and s.cell_id == sc["cell_id"]
    with tempfile.TemporaryDirectory() as td:
        for fmt in (la.FILE_CF32, la.FILE_SC16):
            path, scale = _write(td, f, fmt)
            est, j, g = _chain(path, fmt, scale, sc, tti0, s, None, 7.68e6 * (1.0 + eps), sf_file, eps, len(f))
            o = _oracle_from(j)
            assert len(o) > 10 and g == o, (fmt, len(g), len(o))
        # control: the same file from the same place at the nominal rate loses records
        phy = _phy(sc, **opt)
        n = phy.process_file(path, start_tti=tti0 + j, offset_time=int(round(est.sf_start)), sample_format=fmt, sample_scale=scale, max_subframes=48 - j)
        g = gpu_records(phy)
        phy.close()
        assert n >= 40 and len(g) < len(o) and g != o, (n, len(g), len(o))


@pytest.mark.parametrize("center", [0.0, 1.5e6])
def test_chain_on_a_foreign_rate_recording_whose_clock_is_off(center):
    """the 25-PRB stream recorded at 10 MS/s x (1 + 60e-6) (sinc_convert accepts the ratio: 10 MS/s >= 2.06 x 2.265 MHz), once with the cell 1.5 MHz off the
    recording's centre (the mixer of ddc_cases)"""
    from ddc_cases import carrier
    sc, tti0, iq, opt, _ = _stream()
    eps, nominal, B = 60e-6, 10e6, passband_hz(25)
    true_rate = nominal * (1.0 + eps)
    f = _foreign(true_rate)
    if center:
        f = f * carrier(f.shape[0], center, nominal)[:, None]
    sf_file = 7680.0 * true_rate / 7.68e6
    head = la.resample(f[:int(0.012 * nominal), 0].astype(np.complex64), nominal, 7.68e6, passband_hz=B, center_offset_hz=center)[0]
    rc, s = la.cell_search(head, 25, nof_periods=1)
    assert rc == 1 and s.cell_id == sc["cell_id"]
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, la.FILE_CF32)
        est, j, g = _chain(path, la.FILE_CF32, scale, sc, tti0, s, nominal, true_rate, sf_file, eps, f.shape[0], center)
    o = _oracle_from(j)
    assert len(o) > 10 and g == o, (len(g), len(o))


@functools.lru_cache(maxsize=None)
def _foreign(true_rate):
    sc, tti0, iq, opt, _ = _stream()
    x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])
    n = int(np.ceil(x.shape[0] * true_rate / 7.68e6))
    f = sinc_convert(x, 7.68e6 / true_rate, -LEAD, n + TAIL)
    f.setflags(write=False)
    return f
