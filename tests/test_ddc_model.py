"""Frequency translation in front of the resampler (center_offset_hz), without a GPU: the interface, the float64 model of tests/ddc_cases.py (mixer with the
exact integer phase, then resample_model.Plan) against exact tones that sit off the recording's centre, and the round trip of recordings that hold a cell off
their centre - alone, or next to a second cell 19.8 MHz away - through the model and the CPU oracle.  The GPU tests (test_gpu_ddc.py) hold the kernel to this
model and replay the recordings that pass the round trip here."""
import ctypes as C

import numpy as np
import pytest

import ltesniffer_amd as la
from ddc_cases import CASES, mix, model_resample, offset_hz, offsets_k0, quantise, recording, shifted, tuning_word
from resample_cases import FAR, LEAD, PAIRS, check_tones
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
B100 = passband_hz(100)


def _span(cfg, n_out=1000, in_end=10 ** 6):
    sp = la.ResampleSpan()
    rc = la.lib().lsn_resample_span(C.byref(cfg), n_out, in_end, C.byref(sp))
    return rc, (sp.in_lo, sp.in_hi, sp.max_out, sp.taps)


def test_the_mirrors_carry_center_offset_hz():
    assert la.FileRate._fields_[-1] == ("center_offset_hz", C.c_double) and la.ResampleCfg._fields_[-1] == ("center_offset_hz", C.c_double)
    assert C.sizeof(la.FileRate) == 32 and C.sizeof(la.ResampleCfg) == 80
    assert la.FileRate(32, 0, 25e6, 0.0).center_offset_hz == 0.0                      # the positional calls of before keep their meaning
    assert la._resample_cfg(1, 25e6, 30.72e6, 0, 0.0, 0, 0, B100, la.FILE_CF32, 0.0).center_offset_hz == 0.0
    assert la._resample_cfg(1, 25e6, 30.72e6, 0, 0.0, 0, 0, B100, la.FILE_CF32, 0.0, center_offset_hz=-1e6).center_offset_hz == -1e6
    assert la.resample_span(1000, 10 ** 6, 25e6, 30.72e6, passband_hz=B100, center_offset_hz=3e6) == la.resample_span(1000, 10 ** 6, 25e6, 30.72e6, passband_hz=B100)


def test_span_accepts_the_old_and_the_new_struct_size_and_refuses_the_others():
    new = la._resample_cfg(1, 25e6, 30.72e6, 12345, 0.25, 0, 77, B100, la.FILE_CF32, 0.0)
    old = la._resample_cfg(1, 25e6, 30.72e6, 12345, 0.25, 0, 77, B100, la.FILE_CF32, 0.0, center_offset_hz=float("nan"))   # behind the old size: not read
    old.struct_size = 72
    plan = Plan(25e6, 30.72e6, B100, 12345, 0.25)
    want = (0, plan.span(77, 1000) + (plan.max_out(10 ** 6) - 77, plan.taps))
    assert _span(new) == want and _span(old) == want
    for size in (0, 48, 71, 73, 76, 79, 81, 88, 160):
        new.struct_size = size
        assert _span(new)[0] == INVALID, size


def test_span_applies_the_acceptance_rule_of_the_offset():
    def rc(rate_in, rate_out, f0, passband=B100):
        return _span(la._resample_cfg(1, rate_in, rate_out, 0, 0.0, 0, 0, passband, la.FILE_CF32, 0.0, center_offset_hz=f0))[0]
    edge = 61.44e6 / 2 - B100                      # |f0| + B = rate_in / 2 exactly (whole Hz: the sum is exact)
    for f0 in (edge, -edge, 9.9e6, -9.9e6, 1.0, -1e-300):
        assert rc(61.44e6, 30.72e6, f0) == 0, f0
    for f0 in (edge + 1.0, -edge - 1.0, 30.72e6, 1e30, float("nan"), float("inf"), float("-inf")):
        assert rc(61.44e6, 30.72e6, f0) == INVALID, f0
    assert rc(30.72e6, 30.72e6, 5e6) == 0 and rc(30.72e6, 30.72e6, 0.0) == 0      # equal rates: the resampler takes it, with or without an offset
    assert rc(7.68e6, 7.68e6, 300e3, passband_hz(25)) == 0
    assert rc(20e6, 30.72e6, 0.985e6) == 0 and rc(20e6, 30.72e6, 0.986e6) == INVALID
    # passband_hz 0 stands for 0.44 min(rate): the rule uses that value
    assert rc(25e6, 30.72e6, 1.5e6, 0.0) == 0 and rc(25e6, 30.72e6, 1.51e6, 0.0) == INVALID
    # a rate pair that is refused stays refused whatever the offset
    assert rc(18e6, 30.72e6, 0.0) == INVALID and rc(18e6, 30.72e6, 1e3) == INVALID


def test_tuning_word_and_phase_are_integers():
    assert tuning_word(9.9e6, 61.44e6) == 165 * 2 ** 54 and tuning_word(-9.9e6, 61.44e6) == 2 ** 64 - 165 * 2 ** 54
    assert tuning_word(0.0, 25e6) == 0 and tuning_word(12.5e6, 25e6) == 2 ** 63 and tuning_word(-12.5e6, 25e6) == 2 ** 63
    assert tuning_word(3.9e6, 25e6) == (2 * 39 * 2 ** 64 + 250) // 500
    # the mixer is a function of the sample's index in the recording: a span mixed in pieces is the span mixed at once, also ten minutes in
    rng = np.random.default_rng(2)
    x = rng.standard_normal(3000) + 1j * rng.standard_normal(3000)
    W = tuning_word(3.9e6, 25e6)
    whole = mix(x, FAR, W)
    assert np.array_equal(whole, np.concatenate([mix(x[:1], FAR, W), mix(x[1:777], FAR + 1, W), mix(x[777:], FAR + 777, W)]))
    n = np.arange(3000)
    assert np.max(np.abs(mix(x, 0, W) - x * np.exp(-2j * np.pi * ((39 * n) % 250) / 250))) < 1e-12


@pytest.mark.parametrize("first_sample", [0, FAR])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_model_meets_the_quality_requirement_on_tones_off_the_centre(rate_in, rate_out, nof_prb, first_sample):
    """a tone at f0 + f, |f| <= B, comes out at f within -60 dB relative RMS of its exact value; a tone of the recording whose translated alias or image lands
    in |f| <= B arrives there at least 60 dB down - for the largest offset the acceptance rule admits and a small one, both signs"""
    for k0 in offsets_k0(rate_in, nof_prb):
        f0 = offset_hz(rate_in, k0)
        fn = shifted(lambda plan, x, in_base, n_out: model_resample(f0, plan, x, in_base, n_out), k0)
        worst_pass, worst_land = check_tones(fn, rate_in, rate_out, nof_prb, first_sample=first_sample)
        print("ddc model %.6f -> %.2f MS/s, %d PRB, offset %+.1f kHz, first_sample %d: pass band %.1f dB, landing in band %.1f dB" %
              (rate_in / 1e6, rate_out / 1e6, nof_prb, f0 / 1e3, first_sample, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
        assert worst_pass <= 1e-3 and worst_land <= 1e-3, (k0, worst_pass, worst_land)


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip_through_the_oracle_leaves_the_records_unchanged(case, fmt):
    """capture(s) -> file rate (FFT zero-padding of the whole capture) -> moved to their carriers and added -> file format -> model (mixer + filter) ->
    complex64 -> oracle: every record of the oracle's run on the wanted cell's original capture, byte for byte, and no code block at the edge.  The cases
    and formats that pass here are the ones test_gpu_ddc.py replays."""
    from lsn_testlib import oracle_trace
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    _, _, x = quantise(f, fmt)
    nant, sflen = f.shape[1], int(native) // 1000
    plan = Plan(rate_in, native, passband_hz(sc["nof_prb"]), LEAD, 0.0)
    nsf = min(int(round((len(f) - 2 * LEAD) * native / rate_in / sflen)), plan.max_out(len(f)) // sflen)
    assert nsf == {100: 12, 50: 20, 25: 24}[sc["nof_prb"]]
    y = model_resample(f0, plan, x, 0, nsf * sflen)                              # [sample][antenna]
    iq = np.ascontiguousarray(y.reshape(nsf, sflen, nant).transpose(0, 2, 1)).astype(np.complex64)
    _, _, recs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    recs = oracle_records(recs)
    assert edge_blocks(oracle_trace()) == [] and failed_records(recs) == []
    assert recs == orecs, "records differ: %d vs %d" % (len(recs), len(orecs))
