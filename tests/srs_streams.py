"""Shared by the srsRAN-rate tests (CPU and GPU): the streams that are decoded by the oracle at the 3GPP rate and by the product from the converted
capture, the oracle's transforms through ctypes, and the float32 restatement of what the front ends do to a sample in front of the transform."""
import ctypes as C

import numpy as np

from lsn_testlib import oracle, oracle_trace, scenario
from parity import gen_subframes, oracle_records, run_oracle
from rate_convert import convert_subframes

MAX_TURBO_ITER = 12

# name -> (preset, subframes, scenario overrides, oracle / Phy options).  One stream per bandwidth that has a new symbol size, chosen so that together they cover
# 1 / 2 / 4 CRS ports, the extended cyclic prefix, TM3 / TM4 with 256QAM UEs and harq_mode = 1.  All at 30 dB on a flat channel with zero timing and carrier
# offset, where the conversion is exact.  No faded stream: txgen's fading models add a fractional sampling offset of their own (timing_offset_samples), which
# the symbol-by-symbol conversion does not carry over exactly, so an EVA stream would test the converter, not the receiver.
STREAMS = {
    "prb25_2port": ("small", 24, dict(seed=11), {}),
    "prb50_1port_extcp": ("small", 20, dict(seed=35, cp=1, nof_prb=50, nof_ports=1, nof_rx=1), {}),
    "prb75_4port": ("small", 20, dict(seed=36, nof_prb=75, nof_ports=4, cfi=0, cell_id=77), {}),
    "prb100_tm34_256qam": ("cfg3", 12, dict(seed=9, n_rnti=30, dl_min=3, dl_max=5), {}),
    "prb100_harq": ("cfg2", 30, dict(seed=97, snr_db=30.0, n_rnti=6, dl_min=2, dl_max=3, ul_min=0, ul_max=1, pct_harq=60), dict(harq_mode=1, mcs_tracking_mode=0)),
}


def stream(name):
    """-> (sc, tti0, iq at the 3GPP rate, oracle records as bytes, oracle trace, options)"""
    preset, nsf, over, opt = STREAMS[name]
    sc = scenario(preset, **over)
    tti0, iq, _ = gen_subframes(sc, nsf)
    _, _, orecs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    return sc, tti0, iq, oracle_records(orecs), oracle_trace(), opt


def edge_blocks(otrace):
    """code blocks of the oracle's decode calls that passed their CRC only in the last allowed turbo iteration: a last-bit difference of the soft values
    could flip such a verdict, so a stream used for the record comparison must have none"""
    return [(o["tti"], o["rnti"], c["tb"], c["K"], c["iters"]) for o in otrace for c in o["cbs"] if c["ok"] and c["iters"] >= MAX_TURBO_ITER]


def failed_records(recs):
    """records (context header + PDU, parity.oracle_records) whose CRC verdict is "failed".  A code block the oracle gives up on after the last iteration is
    as much at the edge as one it passes there; such a block of a genuine transmission shows as a CRC-failed record (a trial decode with the wrong MCS table
    fails on both sides and writes no record), so a compared stream must have none either"""
    return [(i, r[:14].hex()) for i, r in enumerate(recs) if r[13] != 1]   # la.mac_lte_record: byte 12 is the CRC tag (7), byte 13 its value


def ul_mode_stream(nof_prb, nsf=40):
    """UL_MODE capture (antenna 0 downlink, antenna 1 uplink: DCI 0 at t, PUSCH at t + 4) at the 3GPP rate and the oracle's UL_MODE worker on it
    -> (sc, tti0, iq[nsf, 2, 15 N], oracle records as bytes, oracle trace)"""
    from lsn_testlib import OracleWorkerUl, gen_ul_mode_subframes, oracle_trace_enable, parse_pcap
    sc = scenario("cfg2", seed=5 + nof_prb, nof_prb=nof_prb, nof_rx=1, n_rnti=12, dl_min=2, dl_max=3, ul_min=2, ul_max=4, mcs_max=10, snr_db=30.0)
    tti0, iq, _ = gen_ul_mode_subframes(sc, nsf, ul_snr_db=30.0)
    oracle_trace_enable(True)
    ow = OracleWorkerUl(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], 3, 5)
    for i in range(nsf):
        ow.work_ul(iq[i, 0], iq[i, 1], tti0 + i, update_meta=1 if i % 25 == 0 else 0)
    return sc, tti0, iq, oracle_records(parse_pcap(ow.pcap_bytes())), oracle_trace()


def converted(sc, iq, uplink_antennas=()):
    return convert_subframes(iq, sc["nof_prb"], cp=sc.get("cp", 0), uplink_antennas=uplink_antennas)


# ---- the oracle's transform ----
def o_fft(x):
    """oracle o_fft on float32 complex x[N] (N = 1024 or 1536, ...) -> complex64[N]"""
    lib = oracle()
    N = x.shape[-1]
    lib.o_fft_twiddle_len.argtypes = [C.c_int]
    w = np.zeros(lib.o_fft_twiddle_len(N), dtype=np.complex64)
    lib.o_fft_twiddles(N, w.ctypes.data)
    a = np.ascontiguousarray(x, dtype=np.complex64).copy()
    lib.o_fft(N, w.ctypes.data, a.ctypes.data)
    return a


def _cmul32(ar, ai, br, bi):
    """complex product with one float32 rounding per operation, as the kernels and the oracle write it (no contraction)"""
    ar, ai, br, bi = (np.asarray(v, dtype=np.float32) for v in (ar, ai, br, bi))
    return ar * br - ai * bi, ar * bi + ai * br


def nco_rotate(x, pos, cfo_hz, N):
    """o_ofdm_rx's NCO on the useful samples x[N] (float32 complex) that start at sample `pos` of their subframe, for symbol size N"""
    lib = oracle()
    lib.o_nco_dphi.restype = C.c_uint32
    lib.o_nco_dphi.argtypes = [C.c_float, C.c_int]
    dphi = int(lib.o_nco_dphi(float(cfo_hz), int(N)))
    coarse, fine = np.zeros(4096, dtype=np.complex64), np.zeros(1024, dtype=np.complex64)
    lib.o_nco_tables.argtypes = [C.c_void_p, C.c_void_p]
    lib.o_nco_tables(coarse.ctypes.data, fine.ctypes.data)
    ph = ((pos + np.arange(N, dtype=np.uint64)) * dphi) & 0xFFFFFFFF
    c, f = coarse[(ph >> 20).astype(np.int64)], fine[((ph >> 10) & 1023).astype(np.int64)]
    rr, ri = _cmul32(c.real, c.imag, f.real, f.imag)
    x = np.asarray(x, dtype=np.complex64)
    yr, yi = _cmul32(x.real, x.imag, rr, ri)
    return (yr + 1j * yi).astype(np.complex64)


def ul_shift(x):
    """o_ul_fft's half-carrier shift on the useful samples x[N]: the table exp(-j pi n / N) in float32, one product per sample"""
    N = x.shape[-1]
    t = np.zeros(N, dtype=np.complex64)
    oracle().o_ul_shift_table.argtypes = [C.c_int, C.c_void_p]
    oracle().o_ul_shift_table(int(N), t.ctypes.data)
    x = np.asarray(x, dtype=np.complex64)
    yr, yi = _cmul32(x.real, x.imag, t.real, t.imag)
    return (yr + 1j * yi).astype(np.complex64)


def dl_bins(N, nre):
    k = np.arange(nre)
    return np.where(k < nre // 2, N - nre // 2 + k, k - nre // 2 + 1)


def ul_bins(N, nre):
    k = np.arange(nre)
    return np.where(k < nre // 2, N - nre // 2 + k, k - nre // 2)


def rel_rms(got, ref):
    return float(np.sqrt(np.sum(np.abs(got - ref) ** 2) / np.sum(np.abs(ref) ** 2)))


def oracle_fft1536_error(nof_symbols=28, seed=5):
    """largest relative RMS error, per symbol, of the oracle's 1536-point transform (three 512-point transforms + radix-3 combination, float32) against
    numpy's float64 transform of the same float32 samples, on OFDM symbols of a loaded 20 MHz cell at 30 dB rewritten at 1536 samples per symbol and
    rounded to float32 - the kind of symbol the 384- and 768-point transforms of the product are measured on"""
    from rate_convert import symbol_starts
    sc = scenario("cfg2", seed=seed)
    _, iq, _ = gen_subframes(sc, (nof_symbols + 13) // 14)
    x = converted(sc, iq)
    worst = 0.0
    n = 0
    for sf in range(x.shape[0]):
        for p, c in symbol_starts(1536, 0):
            if n >= nof_symbols:
                break
            s = x[sf, 0, p + c:p + c + 1536]
            worst = max(worst, rel_rms(o_fft(s).astype(np.complex128), np.fft.fft(s.astype(np.complex128))))
            n += 1
    return worst
