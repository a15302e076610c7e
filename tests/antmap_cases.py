"""Shared by the antenna-map tests (CPU and GPU): recordings whose antennas are not the Phy's, and the float64 model of a mapped cut.

UL_MODE recordings: a 25-PRB UL_MODE capture (srs_streams.ul_mode_stream: antenna 0 downlink, antenna 1 uplink) folded into ONE antenna of a wideband recording,
the downlink at +f and the uplink at -f - what a single radio channel wide enough for the duplex spacing records:
  "30"  30.72 MS/s, carriers +-7.5 MHz, 20 subframes: the ordinary run (ratio 4)
  "61"  61.44 MS/s, carriers +-15 MHz (the 30 MHz duplex spacing of band 12), 12 subframes: the wide-ratio run (ratio 8)
and, as the baseline the parent replays, the same capture as an ordinary two-antenna recording with both antennas at +f.

Four-antenna recording: 15.36 MS/s, antennas 2 and 3 hold the two receive antennas of prb25_2port at +300 kHz, antennas 0 and 1 noise of the same power.

Model: output antenna a = ddc_cases.model_resample(center + offset[a]) of input antenna src[a] with the cell's one plan - the mixer's exact phase, then
resample_model.Plan (ratio up to 4) or wide_resample_model.WidePlan."""
import functools

import numpy as np

from ddc_cases import model_resample, wideband
from resample_cases import LEAD
from resample_model import Plan, passband_hz
from wide_resample_model import WidePlan

NATIVE = 7.68e6          # 25 PRB at the 3GPP rate
SFLEN = 7680
# name -> (subframes, file rate as (num, den) of NATIVE, carrier of the downlink; the uplink sits at minus that)
UL_RECORDINGS = {"30": (20, (4, 1), 7.5e6), "61": (12, (8, 1), 15e6)}
UL_RECORDS = {"30": 73, "61": 38}      # what the oracle's UL_MODE worker writes for the two streams


@functools.lru_cache(maxsize=None)
def ul_stream(nsf):
    """computed once per session, shared and left unchanged by the tests -> srs_streams.ul_mode_stream(25, nsf)"""
    from srs_streams import ul_mode_stream
    return ul_mode_stream(25, nsf)


@functools.lru_cache(maxsize=None)
def ul_recording(name):
    """-> (sc, tti0, oracle records, oracle trace, rate_in, carrier, one-antenna recording [sample][1] complex128); sample LEAD is the first sample of the capture.
    Map of the replay: src = (0, 0), center_offset_hz = carrier, offset_hz = (0, -2 carrier)"""
    nsf, (num, den), fc = UL_RECORDINGS[name]
    sc, tti0, iq, orecs, otrace = ul_stream(nsf)
    rate_in, f = wideband([(iq[:, 0:1, :], fc, 1.0), (iq[:, 1:2, :], -fc, 1.0)], num, den, NATIVE, channel_hz=5e6)
    assert f.shape[1] == 1 and f.shape[0] > LEAD + nsf * SFLEN * num // den
    return sc, tti0, orecs, otrace, rate_in, fc, f


@functools.lru_cache(maxsize=None)
def ul_baseline(name):
    """the same capture as an ordinary two-antenna recording, both antennas at the one carrier: what the unmapped replay takes -> [sample][2] complex128"""
    nsf, (num, den), fc = UL_RECORDINGS[name]
    _, _, iq, _, _ = ul_stream(nsf)
    return wideband([(iq, fc, 1.0)], num, den, NATIVE, channel_hz=5e6)[1]


def extended(name, nsf_total):
    """the one-antenna and the two-antenna recording of `name` continued periodically to nsf_total subframes (tools/antmap_probe.py) -> (rate_in, carrier, f1, f2),
    the recordings as complex64"""
    nsf, (num, den), fc = UL_RECORDINGS[name]
    _, _, _, _, rate_in, _, f1 = ul_recording(name)
    f2 = ul_baseline(name)
    per = nsf * SFLEN * num // den
    reps = -(-nsf_total // nsf)

    def ext(f):
        # the body is periodic over `per` samples up to the carrier's phase, which is whole over a subframe: rate_in / 1000 samples hold fc / 1000 cycles
        f = f.astype(np.complex64)
        return np.concatenate([f[:LEAD]] + [f[LEAD:LEAD + per]] * reps + [f[LEAD + per:]])
    return rate_in, fc, ext(f1), ext(f2)


def plan_for(rate_in, first_sample=LEAD):
    cls = Plan if rate_in <= 4 * NATIVE else WidePlan
    return cls(rate_in, NATIVE, passband_hz(25), first_sample, 0.0)


def model_map(x, rate_in, center_hz, src, offset_hz, n_out, plan=None):
    """x[sample][antenna] (sample 0 = sample 0 of the recording) -> y[len(src)][n_out] complex128: row a cut from antenna src[a] at center_hz + offset_hz[a]"""
    plan = plan or plan_for(rate_in)
    return np.stack([model_resample(center_hz + o, plan, x[:, s:s + 1], 0, n_out)[:, 0] for s, o in zip(src, offset_hz)])


def oracle_ul(sc, tti0, y, nsf):
    """y[2][nsf SFLEN] (row 0 downlink, row 1 uplink) through the oracle's UL_MODE worker, as srs_streams.ul_mode_stream runs it -> (records, trace)"""
    from lsn_testlib import OracleWorkerUl, oracle_trace, oracle_trace_enable, parse_pcap
    from parity import oracle_records
    iq = y.astype(np.complex64).reshape(2, nsf, SFLEN)
    oracle_trace_enable(True)
    ow = OracleWorkerUl(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], 3, 5)
    for i in range(nsf):
        ow.work_ul(iq[0, i], iq[1, i], tti0 + i, update_meta=1 if i % 25 == 0 else 0)
    return oracle_records(parse_pcap(ow.pcap_bytes())), oracle_trace()


# ---- the four-antenna recording ----
FOUR_RATE, FOUR_OFFSET, FOUR_NSF = 15.36e6, 300e3, 24


@functools.lru_cache(maxsize=None)
def four_antennas():
    """-> (sc, tti0, oracle records, oracle trace, options, recording [sample][4] complex128): antennas 2, 3 = prb25_2port at +300 kHz, antennas 0, 1 = white noise of
    the same power"""
    from ddc_cases import cell
    sc, tti0, iq, orecs, otrace, opt = cell("prb25_2port")
    assert iq.shape == (FOUR_NSF, 2, SFLEN)
    rate_in, f = wideband([(iq, FOUR_OFFSET, 1.0)], 2, 1, NATIVE)
    assert rate_in == FOUR_RATE
    rng = np.random.default_rng(41)
    rms = float(np.sqrt(np.mean(np.abs(f) ** 2)))
    noise = (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)) * rms / np.sqrt(2.0)
    return sc, tti0, orecs, otrace, opt, np.concatenate([noise, f], axis=1)
