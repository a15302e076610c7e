"""The timing loop of a pushed stream without a GPU (lsn_stream_track_step, lsn_pss_timing_error): the library's loop against the float64 model bit for
bit, the model loop closed around the phase-domain plant with the loop's two-segment delay, the detector model against the true place of an exactly synthesised
PSS, and the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import ltesniffer_amd as la
import track_model as tm
from track_cases import DETECT_CHANNELS, DETECT_N, DETECT_OFFSETS, pss_subframe, rep

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
# the worst |e - truth| / d the detector model reaches over the cases below (printed by the test; DESIGN 3.1h quotes it); the test asserts twice that
DETECT_WORST = 0.0784


# ---- 1. the library's loop against the model: equal, not close ----

@pytest.mark.parametrize("seed,rates,gains", [
    (1, (30.72e6, 1.92e6), {}),
    (2, (61.44e6, 30.72e6), dict(kp=0.5, ki=0.125, max_ppm=120.0, lost_after=3)),
    (3, (23.04e6 * (1 + 37e-6), 7.68e6), dict(max_ppm=1.5)),      # a clamp that acts all the time
    (4, (11.52e6, 15.36e6), dict(kp=0.1, ki=0.01, max_ppm=50.0, lost_after=1)),
])
def test_loop_step_is_the_model_bit_for_bit(seed, rates, gains):
    rng = np.random.default_rng(seed)
    rate_in, rate_out = rates
    seglen = 5 * int(round(rate_out / 1000.0))
    lib_state = tm.new_state(12.5 if seed == 2 else 0.0, seglen)
    mod_state = dict(lib_state)
    clamped = invalid = 0
    lim = gains.get("max_ppm", tm.MAX_PPM) * 1e-6 * seglen
    for i in range(600):
        e = float(rng.standard_normal() * (0.3, 30.0, 300.0)[i % 3])
        valid = bool(rng.random() > 0.25) and not 200 <= i < 260      # sixty invalid ones in a row among them
        lib_state, d_lib = la.stream_track_step(lib_state, e, valid, rate_in, rate_out, seglen, **gains)
        mod_state, d_mod = tm.loop_step(mod_state, e, valid, rate_in, rate_out, seglen, **gains)
        assert lib_state == mod_state and d_lib == d_mod, (i, lib_state, mod_state, d_lib, d_mod)
        clamped += abs(mod_state["correction"]) == lim
        invalid += not valid
    assert clamped > 10 and invalid > 60
    # the delta is the correction as a rate, in units of 2^-64 input samples per output sample
    assert abs(d_mod - mod_state["correction"] / seglen * rate_in / rate_out * 2.0 ** 64) <= 2.0 ** 13


# ---- 2. the model loop closed around the plant x[h + 3] = x[h + 2] + delta - c[h] ----

@pytest.mark.parametrize("N", [128, 2048])
@pytest.mark.parametrize("ppm", [100.0, -100.0, 90.0, -90.0, 50.0, -50.0])
def test_cold_start_stays_inside_the_pull_in_range_and_settles(N, ppm):
    """From a cold start at a clock error of ppm the error never reaches the pull-in range 5 d and stays below 0.05 delta from segment 40 on.  The loop runs with
    max_ppm = 120, the largest value accepted: the correction is limited to max_ppm, and what it has above the clock error is all that recovers the start-up error.
    +-100 ppm: peak 4.19 delta = 4.02 d, the correction stays between 1.10 and 1.20 delta (the limit) from segment 4 to segment 28 and the integrator is held whenever
    its step would push the correction past the limit (the anti-windup of the definition), 0.018 delta from segment 40 on, below 0.05 delta from segment 36 on.  +-90 ppm: 0.006 delta, from segment 23 on.  +-50 ppm (the limit is never
    reached): peak 4.19 delta, undershoot 0.43 delta, below 0.05 delta from segment 31 on (0.0485), 0.014 delta from segment 40 on.  With max_ppm equal to the clock
    error nothing is left to recover with and the error stays at its peak: max_ppm needs headroom."""
    seglen, d = 75 * N, tm.lag_spacing(N)
    delta = ppm * 1e-6 * seglen
    x, c, _ = tm.simulate(delta, 200, seglen, max_ppm=120.0)
    x = np.abs(np.array(x))
    first = next(h for h in range(len(x)) if x[h:].max() < 0.05 * abs(delta))
    print("N %d %+.0f ppm: peak %.3f delta = %.3f d, error from segment 40 on %.4f delta, below 0.05 delta from segment %d on" %
          (N, ppm, x.max() / abs(delta), x.max() / d, x[40:].max() / abs(delta), first))
    assert x.max() < 5 * d
    assert x[40:].max() < 0.05 * abs(delta)


def test_a_ramp_of_the_clock_error_leaves_a_bounded_error():
    """eps moves by 20 ppm per second = 0.1 ppm per segment: the drift per segment grows by r = 1e-7 seglen every segment.  The loop with the plant is of type 2, so
    a ramp of the drift leaves the constant error r / Ki = 3.2e-6 seglen: 0.49 samples at N = 2048 (reached: 0.4915), 0.031 at N = 128."""
    for N in (128, 2048):
        seglen = 75 * N
        r = 20e-6 * 0.005 * seglen
        drift = [10e-6 * seglen + r * h for h in range(603)]
        x, _, _ = tm.simulate(drift, 600, seglen)
        tail = np.array(x[300:])
        print("N %d: error under a 20 ppm/s ramp %.4f samples (r / Ki = %.4f)" % (N, np.abs(tail).max(), r / tm.KI))
        assert np.abs(tail).max() < 1.01 * r / tm.KI and np.abs(tail - r / tm.KI).max() < 0.01 * r / tm.KI


def test_the_loop_damps_measurement_noise():
    rng = np.random.default_rng(5)
    noise = rng.standard_normal(4000)
    x, _, _ = tm.simulate(0.0, 4000, 75 * 512, noise=noise)
    ratio = float(np.std(x[100:]) / np.std(noise[100:]))
    print("timing error / measurement noise (standard deviations): %.3f" % ratio)
    assert ratio < 1.0


def test_sixty_invalid_segments_hold_the_rate_and_set_lost():
    seglen = 75 * 512
    delta = 30e-6 * seglen
    valid = [not 100 <= h < 160 for h in range(200)]
    x, c, st = tm.simulate(delta, 200, seglen, valid=valid)
    held = st[99]["integrator"]
    assert all(c[h] == held and st[h]["integrator"] == held for h in range(100, 160))       # exactly
    assert [s["lost"] for s in st[100:160]] == [0] * 39 + [1] * 21 and st[160]["lost"] == 0 and st[160]["invalid_run"] == 0
    assert abs(held - delta) < 1e-3 * delta and max(abs(v) for v in x[160:]) < 0.05 * delta


# ---- 3. the detector model against the truth ----

@pytest.mark.parametrize("N", DETECT_N)
def test_detector_model_finds_the_true_offset(N):
    """|e - truth| < d / 2 always - beyond that the wrong lag was picked - and within twice the worst value measured (DETECT_WORST, in units of d)"""
    d, p = tm.lag_spacing(N), tm.pss_index(N)
    offsets = DETECT_OFFSETS if N < 2048 else DETECT_OFFSETS[::2]
    worst = 0.0
    for snr_db, cfo_hz in DETECT_CHANNELS:
        r = rep(N, cfo_hz)
        for o in offsets:
            truth = o * d
            Cv = tm.corr13(pss_subframe(N, truth, snr_db, cfo_hz)[None, :], p, r, d)
            ok, e, peak = tm.observe(Cv, d)
            assert ok and abs(e - truth) < 0.5 * d, (N, snr_db, cfo_hz, o, e)
            lib_ok, lib_e, lib_peak = la.pss_timing_error(Cv.astype(np.float32), d)
            assert lib_ok and abs(lib_e - e) < 1e-4 * d and abs(lib_peak - peak) < 1e-6
            worst = max(worst, abs(e - truth) / d)
    print("N %d: worst |e - truth| = %.4f d" % (N, worst))
    assert worst <= 2.0 * DETECT_WORST


def test_observation_of_the_library_is_the_models():
    rng = np.random.default_rng(9)
    for i in range(200):
        Cv = rng.random(13).astype(np.float32)
        if i % 4 == 0:
            Cv[int(rng.integers(0, 13))] = 2.0
        if i % 50 == 1:
            Cv[:] = 0.0           # a subframe of zeros: the first maximum is lag 0
        ok, e, peak = tm.observe(Cv.astype(np.float64), 4)
        assert la.pss_timing_error(Cv, 4) == (ok, e, peak)
    pk = tm.Peaks()
    assert pk.accept(0.5) and not pk.accept(0.12) and pk.accept(0.13) and pk.hist == [0.5, 0.13]


# ---- 7 (its two conditions): the drifting recording through the float64 sampler, the model loop and the oracle ----

def test_round_trip_open_loop_loses_records_and_the_model_loop_finds_them():
    """what makes the GPU test of the drifting recording (tests/test_gpu_track.py) meaningful.  The 400-subframe 25-PRB stream recorded at 10 MS/s by a clock that
    is off by 60 ppm and slews to 80 ppm: replayed open loop at the nominal rate the oracle finds 12 of its 1040 records; resampled with the model loop it finds
    every record from segment 40 (TTI 200) on - 514 of 514 - and 374 of the 526 in front, none of them different; with initial_ppm = 60 all 1040 (run once by hand, not here: a third replay).  The error the
    model detector sees peaks at 9.1 samples (pull-in range 5 d = 20) and stays within 0.36 from segment 40 on, under the slew of 0.05 ppm per segment"""
    from parity import oracle_records, run_oracle
    from track_cases import DRIFT_NSF, drifting_recording, model_replay, record_tti
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    assert tti0 % 5 == 0 and len(orecs) > 1000

    def oracle(iq):
        return oracle_records(run_oracle(sc, tti0, iq, taps=False, **opt)[2])
    first = tti0 + 200
    late = [r for r in orecs if record_tti(r) >= first]
    assert len(late) > 400 and len(late) < len(orecs)
    got = oracle(model_replay(f, rate, DRIFT_NSF, track=False)[0])
    print("open loop: %d of %d records" % (len(got), len(orecs)))
    assert len(got) < len(orecs) // 2
    iq, log = model_replay(f, rate, DRIFT_NSF, track=True)
    got = oracle(iq)
    early = [r for r in got if record_tti(r) < first]
    print("model loop: %d of %d records, %d of %d in front of segment 40; largest |e| %.2f, from segment 40 on %.3f" %
          (len(got), len(orecs), len(early), len(orecs) - len(late), max(abs(e) for _, e, _ in log), max(abs(e) for _, e, _ in log[40:])))
    assert [r for r in got if record_tti(r) >= first] == late
    assert set(early) <= set(orecs)                                        # records may be missing in front of segment 40, none may differ
    assert all(ok for ok, _, _ in log) and max(abs(e) for _, e, _ in log) < 5 * 4


# ---- 4. refusals that need no device ----

def test_refusals_without_a_device():
    st = tm.new_state()
    for bad in (dict(kp=-0.25), dict(ki=-1.0), dict(kp=math.nan), dict(ki=math.inf), dict(max_ppm=-1.0), dict(max_ppm=120.5), dict(max_ppm=math.nan)):
        with pytest.raises(ValueError):
            la.stream_track_step(st, 0.1, True, 30.72e6, 7.68e6, 38400, **bad)
    assert la.stream_track_step(st, 0.1, True, 30.72e6, 7.68e6, 38400, max_ppm=120.0)[0]["lost"] == 0
    L = la.lib()
    cfg = la._track_cfg(0)
    state = la.StreamTrackState(0.0, 0.0, 0, 0)
    hi, lo = C.c_uint64(), C.c_uint64()
    args = (30.72e6, 7.68e6, 38400, C.byref(state), 0.1, 1, C.byref(hi), C.byref(lo))
    assert L.lsn_stream_track_step(C.byref(cfg), *args) == 0
    for size in (0, C.sizeof(la.StreamTrackCfg) - 4, C.sizeof(la.StreamTrackCfg) + 8):      # every other size
        cfg.struct_size = size
        assert L.lsn_stream_track_step(C.byref(cfg), *args) == INVALID
        assert L.lsn_stream_track(None, C.byref(cfg)) == INVALID
    cfg.struct_size = C.sizeof(la.StreamTrackCfg)
    assert L.lsn_stream_track(None, C.byref(cfg)) == INVALID and L.lsn_stream_track(None, None) == INVALID      # no stream
    status = la.StreamTrackStatus()
    assert L.lsn_stream_track_status(None, C.byref(status)) == INVALID
    assert L.lsn_stream_track_step(C.byref(cfg), 30.72e6, 0.0, 38400, C.byref(state), 0.1, 1, C.byref(hi), C.byref(lo)) == INVALID
    assert L.lsn_stream_track_step(C.byref(cfg), 30.72e6, 7.68e6, 0, C.byref(state), 0.1, 1, C.byref(hi), C.byref(lo)) == INVALID
    # the sizes the header states
    assert C.sizeof(la.StreamTrackCfg) == 32 + 4 * 8 + 8 * 8 + 4 * 8 and C.sizeof(la.StreamTrackStatus) == 8 + 3 * 64 + 32 + 4 * 64 and C.sizeof(la.StreamTrackState) == 24
    with pytest.raises(ValueError):      # lsn_pss_timing refuses before it touches a device
        la.pss_timing([dict(blocks=np.zeros((1, 1, 1920), np.complex64), occ=[(0, 832 + 1920)], replica=np.zeros(128, np.complex64), d=1)])
    with pytest.raises(ValueError):
        la.pss_timing([dict(blocks=np.zeros((1, 1, 1920), np.complex64), occ=[(1, 832)], replica=np.zeros(128, np.complex64), d=1)])
    with pytest.raises(ValueError):
        la.pss_timing([dict(blocks=np.zeros((1, 1, 1920), np.complex64), occ=[(0, 832)], replica=np.zeros(128, np.complex64), d=2)])
