"""The sample-clock estimate without a GPU: the C ABI's plan and fit (host code, double) against tests/clock_model.py, the windows against the drift they
must hold, the refusals, and the accuracy of the DEFINITION itself - the model run on PSS trains whose clock error is known exactly.

Accuracy condition: |eps_hat - eps| x (samples of the recording) <= 0.5 - half a sample is the misalignment every plain-file replay lives with, because
offset_time_samples is an integer.  Values the model reaches on these inputs (samples at the end of the recording): profiles/clock_estimate.txt."""
import ctypes as C
import numpy as np
import pytest

import ltesniffer_amd as la
import clock_model as M
from clock_cases import TRAINS, drifted_capture, end_error, train

INVALID = -2
NEW = ["lsn_clock_plan", "lsn_clock_fit", "lsn_clock_replica", "lsn_clock_track", "lsn_clock_estimate", "lsn_file_clock_estimate"]
GEOM = [(6, la.RATES_3GPP, 128), (25, la.RATES_SRSRAN, 384), (100, la.RATES_3GPP, 2048)]


def _cfg(nof_prb, rates, pss_pos, n_id_2=1, cfo_hz=0.0, max_ppm=200.0, max_periods=0, sf_start=0):
    return la.ClockCfg(C.sizeof(la.ClockCfg), nof_prb, rates, n_id_2, pss_pos, cfo_hz, max_ppm, max_periods, sf_start)


def _plan(cfg, nof_samples, rnd, prev=None, cap=64):
    w = (la.ClockObs * cap)()
    p = None
    if prev is not None:
        p = la.Clock(found=1, eps=prev["eps"], pss_pos0=prev["pss_pos0"])
    n = la.lib().lsn_clock_plan(C.byref(cfg), nof_samples, rnd, C.byref(p) if p is not None else None, w, cap)
    return n, [(int(o.period), int(o.centre), int(o.half_width)) for o in w[:max(n, 0)]]


def test_the_six_symbols_are_declared_and_exported():
    for s in NEW:
        assert s in la.EXPORTS
        getattr(la.lib(), s)
    assert C.sizeof(la.ClockCfg) == 48 and C.sizeof(la.ClockObs) == 40 and C.sizeof(la.Clock) == 64


@pytest.mark.parametrize("nof_prb,rates,N", GEOM)
def test_plan_equals_the_model_and_its_windows_hold_the_drift(nof_prb, rates, N):
    assert la.symbol_sz(nof_prb, rates) == N
    W5, pss_pos, max_ppm = 75 * N, 5000, 200.0
    ns = pss_pos + 40 * W5                                   # 40 periods: rounds of 8, 32 and 40
    assert M.nof_periods(N, pss_pos, ns) == 40 and M.schedule(40) == [8, 32, 40]
    cfg = _cfg(nof_prb, rates, pss_pos)
    n, w0 = _plan(cfg, ns, 0)
    assert n == 8 and w0 == M.plan(N, pss_pos, ns, 0)
    assert la.lib().lsn_clock_plan(C.byref(cfg), ns, 0, None, None, 0) == 8          # the number alone
    assert la.lib().lsn_clock_plan(C.byref(cfg), ns, 1, None, None, 0) == INVALID    # a later round needs the fit in front of it
    assert _plan(cfg, ns, 0, cap=7)[0] == INVALID
    for eps in np.linspace(-max_ppm * 1e-6, max_ppm * 1e-6, 41):
        for dp in (-2.0, -0.4, 0.0, 1.7, 2.0):               # the cell search's pss_pos is an integer near p_0
            p0 = pss_pos + dp
            for q, c, h in w0:                               # round 0: every true position at least 2 lags inside
                pq = p0 + q * W5 * (1.0 + eps)
                assert c - h + 2 <= pq <= c + h - 2, (eps, dp, q)
            # later rounds: the fit in front is off by at most one sample at its first period and drifts by at most one more across its span
            for rnd, qp in ((1, 8), (2, 32)):
                for e0 in (-1.0, 0.0, 1.0):
                    for de in (-1.0, 0.0, 1.0):
                        prev = dict(pss_pos0=p0 + e0, eps=eps + de / ((qp - 1) * W5))
                        n, w = _plan(cfg, ns, rnd, prev)
                        assert n == (32 if rnd == 1 else 40) and w == M.plan(N, pss_pos, ns, rnd, prev)
                        for q, c, h in w:
                            pq = p0 + q * W5 * (1.0 + eps)
                            assert c - h + 2 <= pq <= c + h - 2, (eps, dp, rnd, e0, de, q, c, h, pq)
    assert _plan(cfg, ns, 3, dict(pss_pos0=float(pss_pos), eps=0.0))[0] == 0   # round 2 was the last
    # max_periods caps Q; a short buffer gives fewer periods
    assert _plan(_cfg(nof_prb, rates, pss_pos, max_periods=20), ns, 1, dict(pss_pos0=float(pss_pos), eps=0.0))[0] == 20
    assert _plan(cfg, pss_pos + 5 * W5, 0)[0] == 5 == M.nof_periods(N, pss_pos, pss_pos + 5 * W5)


def _obs_list(rows):
    a = (la.ClockObs * len(rows))()
    for o, (q, valid, pos, peak) in zip(a, rows):
        o.period, o.valid, o.pos, o.peak = q, valid, pos, peak
    return a


def _line(n, W5, eps, p0, noise, seed):
    rng = np.random.default_rng(seed)
    return [[q, 1, p0 + q * W5 * (1 + eps) + float(noise * rng.standard_normal()), float(np.float32(0.8 + 0.05 * rng.standard_normal()))] for q in range(n)]


FITS = {}
_r = _line(32, 9600, 37e-6, 4321.4, 0.05, 1)
for _q in (3, 17):
    _r[_q][1] = 0                       # invalid entries (their pos means nothing)
    _r[_q][2] = 1e9
for _q in (5, 20, 21):
    _r[_q][3] = float(np.float32(0.15))  # weak peaks, far off the line
    _r[_q][2] += 20.0
_r[9][2] += 3.0                          # two 3-sample outliers
_r[26][2] -= 3.0
FITS["invalid_weak_outliers"] = (_r, 9600, 1, 25)
_r = _line(8, 9600, -80e-6, 700.2, 0.05, 2)
for _q in (0, 2, 3, 5, 6):
    _r[_q][1] = 0
FITS["three_survivors"] = (_r, 9600, 0, 3)
_r = _line(32, 28800, 120e-6, 9000.7, 0.0, 3)
for _q in range(32):
    _r[_q][2] += 0.7 if _q % 2 else -0.7
FITS["rms_above_half"] = (_r, 28800, 0, 32)
_r = _line(20, 153600, 5e-6, 100000.1, 0.05, 4)
for _q in range(9, 20):
    _r[_q][1] = 0
FITS["fewer_than_half"] = (_r, 153600, 0, 9)
_r = _line(120, 9600, -200e-6, 1234.5, 0.08, 5)
FITS["clean_120"] = (_r, 9600, 1, 120)
_r = _line(8, 9600, 0.0, 50.0, 0.05, 6)
for _q in range(1, 8):
    _r[_q][1] = 0
FITS["one_left"] = (_r, 9600, 0, 1)


@pytest.mark.parametrize("name", sorted(FITS))
def test_fit_equals_the_model(name):
    rows, W5, found, used = FITS[name]
    out = la.Clock()
    rc = la.lib().lsn_clock_fit(_obs_list(rows), len(rows), W5, C.byref(out))
    m = M.fit([tuple(r) for r in rows], W5)
    assert rc == out.found == m["found"] == found
    assert out.nof_used == m["nof_used"] == used and out.nof_periods == len(rows)
    span = W5 * len(rows)
    assert abs(out.eps - m["eps"]) * span <= 1e-9 and abs(out.pss_pos0 - m["pss_pos0"]) <= 1e-9
    assert abs(out.rms_residual - m["rms_residual"]) <= 1e-9 and abs(out.max_residual - m["max_residual"]) <= 1e-9
    if name == "invalid_weak_outliers":
        assert abs(out.eps - 37e-6) * span <= 0.1 and abs(out.pss_pos0 - 4321.4) <= 0.1 and out.max_residual < 0.3
    assert la.lib().lsn_clock_fit(None, 4, W5, C.byref(out)) == INVALID and la.lib().lsn_clock_fit(_obs_list(rows), len(rows), 0, C.byref(out)) == INVALID


def _report(name, res, eps, ns, p0=None):
    err = end_error(res["eps"], eps, ns)
    print("clock model %-28s eps %+9.3f ppm -> %+9.3f ppm: %.4f sample at the end of %d samples; rounds %d, used %d / %d, rms %.3f, max %.3f%s" %
          (name, eps * 1e6, res["eps"] * 1e6, err, ns, res["nof_rounds"], res["nof_used"], res["nof_periods"], res["rms_residual"], res["max_residual"],
           "" if p0 is None else ", p0 off by %+.3f" % (res["pss_pos0"] - p0)))
    return err


@pytest.mark.parametrize("name", sorted(TRAINS))
def test_the_definition_meets_the_half_sample_condition_on_exact_trains(name):
    x, info = train(name)
    res, obs = M.estimate(x, info["N"], info["n_id_2"], info["pss_pos"], info["cfo_hz"])
    err = _report(name, res, info["eps"], len(x), info["p0"])
    assert res["found"] == 1 and res["nof_rounds"] == 3 and res["nof_periods"] == info["periods"] == 120
    assert err <= 0.5 and abs(res["pss_pos0"] - info["p0"]) <= 0.5
    med = float(np.median([pk for _, valid, _, _, _, pk in obs if valid]))
    for q, valid, c, h, pos, pk in obs:
        if q in info["blank"]:
            assert not valid or pk < 0.25 * med           # noise only: invalid, or dropped as a weak peak
    assert res["nof_used"] <= 120 - len(info["blank"]) and res["nof_used"] >= 100


def capture_pss_pos(sc, tti0, eps, N):
    """where the first PSS of a resample_cases file lies (sample LEAD = first sample of the stream, normal CP): (true position, the integer next to it)"""
    from resample_cases import LEAD
    k = (-tti0) % 5
    p0 = LEAD + (k * 15 * N + 160 * N // 2048 + 6 * (N + 144 * N // 2048)) * (1.0 + eps)
    return p0, int(round(p0))


@pytest.mark.parametrize("case", ["prb25_plus_150ppm", "prb25_minus_150ppm"])
def test_the_definition_meets_the_condition_on_the_drifted_25_prb_captures(case):
    sc, tti0, orecs, opt, native, eps, f = drifted_capture(case)
    assert sc["nof_prb"] == 25 and native == 7.68e6 and sc.get("cp", 0) == 0 and abs(abs(eps) - 150e-6) < 1e-12
    p0, pss_pos = capture_pss_pos(sc, tti0, eps, 512)
    x = f[:, 0].astype(np.complex64)
    res, obs = M.estimate(x, 512, sc["cell_id"] % 3, pss_pos)
    err = _report(case, res, eps, len(x), p0)
    assert res["found"] == 1 and res["nof_periods"] in (9, 10) and res["nof_rounds"] == 2
    assert err <= 0.5 and abs(res["pss_pos0"] - p0) <= 0.5


@pytest.mark.parametrize("nof_prb,rates,N", GEOM)
def test_replica_of_the_library_is_the_models(nof_prb, rates, N):
    """the same formula in double through the same libm: equal but for the last bit of a float where a cosine differs in its last bit"""
    for n_id_2, cfo in ((0, 0.0), (1, 2000.0), (2, -3511.5)):
        out = np.zeros(N, dtype=np.complex64)
        assert la.lib().lsn_clock_replica(C.byref(_cfg(nof_prb, rates, 100, n_id_2=n_id_2, cfo_hz=cfo)), out.ctypes.data) == 0
        r = M.replica(n_id_2, N, float(np.float32(cfo)))
        assert abs(float(np.sum(np.abs(out.astype(np.complex128)) ** 2)) - 1.0) < 1e-6
        d = np.maximum(np.abs(out.real - r.real), np.abs(out.imag - r.imag))
        assert float(d.max()) <= 2.0 ** -23 * float(np.abs(r).max()), float(d.max())


def test_refusals():
    L = la.lib()
    ns = 100 + 40 * 9600
    w = (la.ClockObs * 64)()
    good = _cfg(6, 0, 100)
    assert L.lsn_clock_plan(C.byref(good), ns, 0, None, w, 64) == 8
    bad = [_cfg(6, 0, 100, n_id_2=3), _cfg(7, 0, 100), _cfg(6, 5, 100), _cfg(6, -1, 100), _cfg(6, 0, 100, max_ppm=0.0), _cfg(6, 0, 100, max_ppm=-5.0),
           _cfg(6, 0, 100, max_ppm=1000.5), _cfg(6, 0, 100, max_ppm=float("nan")), _cfg(6, 0, 100, cfo_hz=float("inf")), _cfg(6, 0, 2)]   # the last: no room for window 0
    for size in (0, 40, C.sizeof(la.ClockCfg) + 8):
        c = _cfg(6, 0, 100)
        c.struct_size = size
        bad.append(c)
    for c in bad:
        assert L.lsn_clock_plan(C.byref(c), ns, 0, None, w, 64) == INVALID
    buf = np.zeros(4096, dtype=np.complex64)
    for c in bad[:3] + bad[-3:]:
        assert L.lsn_clock_replica(C.byref(c), buf.ctypes.data) == INVALID
    assert L.lsn_clock_plan(None, ns, 0, None, w, 64) == INVALID
    assert L.lsn_clock_plan(C.byref(good), 100 + 3 * 9600 + 100, 0, None, w, 64) == INVALID    # Q = 3
    assert L.lsn_clock_plan(C.byref(good), 100 + 4 * 9600, 0, None, w, 64) == 4                  # Q = 4 is enough
    # clock_cfg of the binding: a pss_pos in the first four samples moves to the next occurrence
    s = la.CellSearch(n_id_2=2, pss_pos=1, sf_start=5000, cfo_hz=12.5)
    c = la.clock_cfg(6, s)
    assert (c.pss_pos, c.n_id_2, c.sf_start, c.max_ppm, c.struct_size) == (9601, 2, 5000, 200.0, C.sizeof(la.ClockCfg))
