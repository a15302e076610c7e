"""The resampler's filter, without a GPU: the float64 model written from DESIGN.md section 3.1b (tests/resample_model.py) against signals whose exact value
is known at every instant, and a round trip - a 3GPP-rate capture taken to a foreign rate by an independent exact method, brought back by the model,
decoded by the CPU oracle - that must leave the oracle's record stream unchanged byte for byte.  The GPU tests (test_gpu_resample.py) then hold the
kernel to this model within the float32 dot-product bound."""
import numpy as np
import pytest

import ltesniffer_amd as la
from resample_cases import CASES, FAR, LEAD, PAIRS, check_tones, foreign_capture
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records


def test_new_symbols_are_exported():
    for s in ("lsn_resample", "lsn_resample_span", "lsn_phy_process_file_rate"):
        assert s in la.EXPORTS
        getattr(la.lib(), s)


def _model(plan, x, in_base, n_out):
    return plan.apply(x, 0, n_out, in_base=in_base)


@pytest.mark.parametrize("first_sample", [0, FAR])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_model_meets_the_quality_requirement_on_exact_tones(rate_in, rate_out, nof_prb, first_sample):
    """a tone anywhere in the occupied band comes out within -60 dB relative RMS of its exact value; a tone that would alias or image into the occupied
    band arrives there at least 60 dB down - at the start of a recording and ten minutes into one"""
    worst_pass, worst_land = check_tones(_model, rate_in, rate_out, nof_prb, first_sample=first_sample)
    print("resample model %.6f -> %.2f MS/s, %d PRB, first_sample %d: pass band %.1f dB, landing in band %.1f dB" %
          (rate_in / 1e6, rate_out / 1e6, nof_prb, first_sample, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
    assert worst_pass <= 1e-3 and worst_land <= 1e-3, (worst_pass, worst_land)


def test_positions_are_integers_and_split_calls_agree():
    plan = Plan(25e6, 30.72e6, passband_hz(100), FAR, 0.7)
    assert plan.step == (2 * 625 * 2 ** 64 + 768) // (2 * 768) and plan.position(10 ** 9) == plan.start + 10 ** 9 * plan.step
    rng = np.random.default_rng(1)
    lo, hi = plan.span(0, 5000)
    x = rng.standard_normal(hi - lo) + 1j * rng.standard_normal(hi - lo)
    whole = plan.apply(x, 0, 5000, in_base=lo)
    parts = np.concatenate([plan.apply(x, a, b - a, in_base=lo) for a, b in ((0, 1), (1, 777), (777, 4096), (4096, 5000))])
    assert np.array_equal(whole, parts)


def test_refused_rate_pairs():
    for rate_in, rate_out, nprb in ((18e6, 30.72e6, 100), (123e6, 30.72e6, 100), (30.72e6 * 4.001, 30.72e6, 100), (1.0e6, 1.92e6, 6)):
        with pytest.raises(ValueError):
            Plan(rate_in, rate_out, passband_hz(nprb))
    for nprb, out in ((6, 1.92e6), (15, 3.84e6), (25, 7.68e6), (50, 15.36e6), (75, 23.04e6), (100, 30.72e6), (25, 5.76e6), (50, 11.52e6), (75, 15.36e6), (100, 23.04e6)):
        assert Plan(1.1 * 180e3 * nprb, out, passband_hz(nprb)).taps <= 192     # the lowest rate that must be accepted ...
        assert Plan(4 * out, out, passband_hz(nprb)).taps <= 192                # ... and the highest


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip_through_the_oracle_leaves_the_records_unchanged(case):
    """capture -> foreign rate (FFT zero-padding / truncation of the whole capture, or a direct sinc sum for the ppm pair) -> model -> complex64 -> oracle:
    every record of the oracle's run on the original capture, byte for byte; and the round trip leaves no code block at the edge (last turbo iteration,
    failed CRC), which is what the GPU record tests rest on"""
    from lsn_testlib import oracle_trace
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, rate_in, native, f = foreign_capture(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    nsf, nant, sflen = (len(f) - 2 * LEAD) * native / rate_in, f.shape[1], int(native) // 1000
    plan = Plan(rate_in, native, passband_hz(sc["nof_prb"]), LEAD, 0.0)
    nsf = min(int(round(nsf)), plan.max_out(len(f)) // sflen)
    assert nsf == CASES[case][1] or nsf == {"prb100_tm34_256qam": 12, "prb50_1port_extcp": 20}[CASES[case][0]]
    y = plan.apply(f, 0, nsf * sflen)                                            # [sample][antenna]
    iq = np.ascontiguousarray(y.reshape(nsf, sflen, nant).transpose(0, 2, 1)).astype(np.complex64)
    _, _, recs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    recs = oracle_records(recs)
    assert edge_blocks(oracle_trace()) == [] and failed_records(recs) == []
    assert recs == orecs, "records differ: %d vs %d" % (len(recs), len(orecs))
