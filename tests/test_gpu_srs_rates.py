"""The srsRAN sampling mode (lsn_phy_set_sampling(LSN_RATES_SRSRAN): 384 / 768 / 1024 / 1536 samples per OFDM symbol at 25 / 50 / 75 / 100 PRB) on the GPU.
The oracle is frozen at the 3GPP sizes, so the new ground is pinned three ways: the transforms bit-exact where the oracle has one of that length (1024,
1536), against float64 where it has none (384, 768), and the decisions end to end - a stream decoded by the oracle at the 3GPP rate against the product
decoding the capture rewritten at srsRAN's rate (tests/rate_convert.py)."""
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from lsn_testlib import scenario
from parity import gen_subframes, gpu_records
from rate_convert import SYMBOL_SZ_3GPP, SYMBOL_SZ_SRSRAN, symbol_starts
from srs_streams import (STREAMS, converted, dl_bins, edge_blocks, nco_rotate, o_fft, failed_records, oracle_fft1536_error, rel_rms, stream, ul_bins, ul_mode_stream, ul_shift)

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}


def _phy(sc, batch, rates=la.RATES_SRSRAN, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(rates) and phy.get_sampling() == rates
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


def _grid(phy, sc, sf):
    nre = 12 * sc["nof_prb"]
    return phy.tap(la.TAP_GRID, sf, np.complex64, sc["nof_rx"] * 14 * nre).reshape(sc["nof_rx"], 14, nre)


def test_sampling_mode_is_chosen_before_the_cell():
    phy = la.Phy(nof_rx_antennas=1, max_batch=2, pcapwriter=la.PcapWriter(None))
    assert phy.get_sampling() == la.RATES_3GPP
    assert not phy.set_sampling(2) and not phy.set_sampling(-1) and phy.get_sampling() == la.RATES_3GPP
    assert phy.set_sampling(la.RATES_SRSRAN) and phy.set_sampling(la.RATES_3GPP) and phy.set_sampling(la.RATES_SRSRAN)
    assert phy.setCell(100, 1, 3)
    assert not phy.set_sampling(la.RATES_3GPP) and phy.get_sampling() == la.RATES_SRSRAN   # a configured Phy keeps its mode ...
    assert phy.set_sampling(la.RATES_SRSRAN)                                                # ... and says yes to the one it has
    w = phy.getAvail()
    assert la.lib().lsn_worker_buffer_len(w._h) == 3 * 15 * 1536
    phy.putPending(w)
    phy.joinPending()
    phy.close()


@pytest.mark.parametrize("nof_prb,cp,cfo", [(75, 0, 0.0), (75, 1, 0.0), (75, 0, 1234.5), (100, 0, 0.0), (100, 1, -777.0), (100, 0, 2500.0), (100, 1, 0.0)])
def test_downlink_grid_is_bit_identical_to_the_oracle_transform(nof_prb, cp, cfo):
    """75 PRB at srsRAN's rate is the 1024-point transform, 100 PRB the 1536-point one (radix-3 path, 1200 of 1536 bins kept): CP strip and NCO restated
    here in float32 as o_ofdm_rx has them (phase from pos + n at the NEW symbol size), the transform is the oracle's o_fft.  Zero differing words."""
    N, nre = SYMBOL_SZ_SRSRAN[nof_prb], 12 * nof_prb
    sc = scenario("cfg2", seed=3 + nof_prb, nof_prb=nof_prb, cp=cp, n_rnti=8, dl_min=2, dl_max=3)
    _, iq, _ = gen_subframes(sc, 2)
    x = converted(sc, iq)
    phy = _phy(sc, 2)
    if cfo:
        phy.setCfoCorrection(la.Phy.CFO_FIXED, cfo)
    phy.process_host(x, 0)
    ndiff = 0
    for sf in range(2):
        g = _grid(phy, sc, sf)
        for rx in range(sc["nof_rx"]):
            for l, (p, c) in enumerate(symbol_starts(N, cp)):
                s = x[sf, rx, p + c:p + c + N]
                if cfo:
                    s = nco_rotate(s, p + c, cfo, N)
                ref = o_fft(s)[dl_bins(N, nre)]
                ndiff += int(np.count_nonzero(g[rx, l].view(np.uint32) != ref.view(np.uint32)))
    phy.close()
    assert ndiff == 0, ndiff


@pytest.mark.parametrize("nof_prb,cp", [(75, 0), (75, 1), (100, 0), (100, 1)])
def test_uplink_grid_is_bit_identical_to_the_oracle_transform(nof_prb, cp):
    """k_ul_fft at 1024 / 1536: the half-carrier shift is one float32 product with the table exp(-j pi n / N) (o_ul_shift_table at the new N), then o_fft"""
    N, nre = SYMBOL_SZ_SRSRAN[nof_prb], 12 * nof_prb
    sc = scenario("cfg2", seed=50 + nof_prb, nof_prb=nof_prb, cp=cp, nof_rx=1, n_rnti=8, dl_min=2, dl_max=3)
    _, iq, _ = gen_subframes(sc, 2)
    x = converted(sc, iq)[:, 0]   # any band-limited samples do: the test is about the transform
    phy = _phy(sc, 2)
    assert phy.setUlConfig(3, 5)
    phy.pusch_decode(x, 0, [])
    ndiff = 0
    for sf in range(2):
        g = phy.tap_ul_grid(sf)
        for l, (p, c) in enumerate(symbol_starts(N, cp)):
            ref = o_fft(ul_shift(x[sf, p + c:p + c + N]))[ul_bins(N, nre)]
            ndiff += int(np.count_nonzero(g[l].view(np.uint32) != ref.view(np.uint32)))
    phy.close()
    assert ndiff == 0, ndiff


@pytest.mark.parametrize("nof_prb", [25, 50])
def test_transforms_384_and_768_against_float64(nof_prb):
    """No oracle transform of these lengths exists.  Grid tap against numpy's float64 transform of the very float32 samples the GPU was given, relative RMS
    error per symbol, downlink (normal and extended CP) and uplink.  Bound: twice the same error of the oracle's o_fft(1536) - the same three-way structure
    with two / one more radix-2 stages - measured on the CPU on the same kind of symbol (srs_streams.oracle_fft1536_error): the shallower transform must
    not be worse than the deeper reference.
    Measured: oracle o_fft(1536) 1.274e-07 -> bound 2.548e-07.  Largest GPU error (MI355X): 384 points 1.128e-07, 768 points 1.137e-07 (profiles/srs_rates.txt)."""
    N, nre = SYMBOL_SZ_SRSRAN[nof_prb], 12 * nof_prb
    e_ref = oracle_fft1536_error()
    bound = 2.0 * e_ref
    worst = {}
    for cp in (0, 1):
        sc = scenario("cfg2", seed=20 + nof_prb + cp, nof_prb=nof_prb, cp=cp, n_rnti=8, dl_min=2, dl_max=3)
        _, iq, _ = gen_subframes(sc, 2)
        x = converted(sc, iq)
        phy = _phy(sc, 2)
        phy.process_host(x, 0)
        assert phy.setUlConfig(3, 5)
        grids = [_grid(phy, sc, sf) for sf in range(2)]
        phy.pusch_decode(x[:, 0], 0, [])
        for sf in range(2):
            ug = phy.tap_ul_grid(sf)
            for l, (p, c) in enumerate(symbol_starts(N, cp)):
                for rx in range(sc["nof_rx"]):
                    s = x[sf, rx, p + c:p + c + N].astype(np.complex128)
                    e = rel_rms(grids[sf][rx, l].astype(np.complex128), np.fft.fft(s)[dl_bins(N, nre)])
                    worst["dl", cp] = max(worst.get(("dl", cp), 0.0), e)
                # uplink: the shift table is float32 in the kernel, so the float64 reference transforms the float32 product the kernel forms
                s = ul_shift(x[sf, 0, p + c:p + c + N]).astype(np.complex128)
                e = rel_rms(ug[l].astype(np.complex128), np.fft.fft(s)[ul_bins(N, nre)])
                worst["ul", cp] = max(worst.get(("ul", cp), 0.0), e)
        phy.close()
    print("srs_rates fft N=%d: oracle o_fft(1536) error %.3e, bound %.3e, GPU %s" % (N, e_ref, bound, {k: "%.3e" % v for k, v in sorted(worst.items())}))
    assert max(worst.values()) <= bound, (worst, bound)


def _records_srs(name):
    sc, tti0, iq, orecs, otrace, opt = stream(name)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    x = converted(sc, iq)
    phy = _phy(sc, 8, **opt)
    for b in range(0, x.shape[0], 8):
        phy.process_host(x[b:b + 8], tti0 + b)
    g = gpu_records(phy)
    phy.close()
    return g, orecs


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_records_equal_the_oracle_at_the_3gpp_rate(name):
    """(TTI, RNTI, direction, RNTI type, CRC verdict, PDU bytes) of every record, none left out: the oracle on the 3GPP-rate capture, the product on the converted one"""
    g, o = _records_srs(name)
    assert g == o, "records differ: gpu %d vs oracle %d, first difference at %s" % (len(g), len(o), next((i for i, (a, b) in enumerate(zip(g, o)) if a != b), min(len(g), len(o))))


def test_every_entry_point_at_100_prb_1536():
    """process_device, submit / wait, int16 host samples, a cf32 and an sc16 file with an offset counted in samples of the file's rate, the worker pool fed
    23 040 samples per subframe, two engines on one device - each gives the record list of the stream.  The 16-bit legs quantise to 1 / 8192 (13 bits
    below a full scale of 4; the capture's RMS is near 1): quantisation noise 2^-26 / 6 per sample, 80 dB under the signal and 50 dB under the
    stream's own noise, so the records are demanded equal without allowance."""
    import torch
    name = "prb100_tm34_256qam"
    sc, tti0, iq, orecs, otrace, _ = stream(name)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == []
    x = converted(sc, iq)
    nsf, A, sflen = x.shape[0], sc["nof_rx"], 15 * 1536
    assert x.shape[2] == sflen == 23040
    d = torch.from_numpy(x.view(np.float32)).to("cuda:0")
    got = {}
    phy = _phy(sc, 8)
    phy.process_device(d.data_ptr(), nsf, tti0, 0, torch.cuda.current_stream().cuda_stream)
    got["process_device"] = gpu_records(phy)
    phy.close()
    phy = _phy(sc, 4)
    phy.submit_device(d.data_ptr(), nsf, tti0)
    phy.wait()
    got["submit_wait"] = gpu_records(phy)
    phy.close()
    phy = _phy(sc, 4, devices=[0, 0])
    phy.process_device(d.data_ptr(), nsf, tti0)
    got["two_engines"] = gpu_records(phy)
    phy.close()
    # worker pool: the producer copies one subframe of 23 040 samples per antenna into a buffer of 3 x 23 040
    phy = _phy(sc, 8)
    for i in range(nsf):
        w = phy.getAvail()
        bufs = w.getBuffers()
        assert len(bufs[0]) == 3 * sflen
        for rx in range(A):
            bufs[rx][:sflen] = x[i, rx]
        tti = tti0 + i
        w.prepare(tti % 10, (tti // 10) % 1024, False)
        phy.putPending(w)
    phy.joinPending()
    got["worker_pool"] = gpu_records(phy)
    phy.close()
    with tempfile.TemporaryDirectory() as td:
        lead = 777   # samples of the FILE's rate in front of the first subframe
        inter = np.ascontiguousarray(x.transpose(0, 2, 1).reshape(nsf * sflen, A))   # antennas interleaved per sample
        pad = np.zeros((lead, A), dtype=np.complex64)
        p32 = os.path.join(td, "c.cf32")
        np.concatenate([pad, inter]).tofile(p32)
        phy = _phy(sc, 8)
        assert phy.process_file(p32, start_tti=tti0, offset_time=lead) == nsf
        got["file_cf32"] = gpu_records(phy)
        phy.close()
        # 16-bit samples: one LSB = 2^-13 (exact in float32), as a radio asked for sc16 delivers them
        scale = 2.0 ** -13
        assert float(np.abs(x.view(np.float32)).max()) < 3.9
        q = np.round(x.view(np.float32).reshape(nsf, A, sflen, 2) / scale).astype(np.int16)
        phy = _phy(sc, 8)
        phy.process_host_int(q, tti0, sample_scale=scale)
        got["host_int16"] = gpu_records(phy)
        phy.close()
        p16 = os.path.join(td, "c.sc16")
        np.concatenate([np.zeros((lead, A, 2), dtype=np.int16), np.ascontiguousarray(q.transpose(0, 2, 1, 3)).reshape(nsf * sflen, A, 2)]).tofile(p16)
        phy = _phy(sc, 8)
        assert phy.process_file(p16, start_tti=tti0, offset_time=lead, sample_format=la.FILE_SC16, sample_scale=scale) == nsf
        got["file_sc16"] = gpu_records(phy)
        phy.close()
    for k, g in got.items():
        assert g == orecs, "%s: %d records vs %d" % (k, len(g), len(orecs))


def test_cell_search_mib_and_file_replay_chained_at_srsran_rate():
    """A recording that starts at an unknown sample: L samples of receiver noise at the 3GPP rate, round(L N_r / N) at srsRAN's, in front of a stream that
    itself starts inside a radio frame.  The search at srsRAN's rate finds cell id, CP and half-frame index of the 3GPP-rate search and sf_start equal to
    its sf_start scaled by N_r / N, within one sample; the MIB decoded on the next subframe 0 is the transmitted one; the file replayed from there (offset in
    samples of the file's rate, SFN from the MIB) gives the records of the oracle run on the same subframes at the 3GPP rate."""
    from parity import oracle_records, run_oracle
    sc = scenario("cfg2", seed=9, start_tti=10 * 300 + 2, nof_prb=100, nof_rx=1, cell_id=401, n_rnti=8, dl_min=2, dl_max=3, snr_db=30.0)
    N, Nr = SYMBOL_SZ_3GPP[100], SYMBOL_SZ_SRSRAN[100]
    tti0, iq, _ = gen_subframes(sc, 30)
    x = converted(sc, iq)
    L = 4 * 1237          # 4948 samples at 30.72 MS/s = 3711 at 23.04 MS/s: no multiple of a symbol or a subframe
    Lr = L * Nr // N
    assert Lr * N == L * Nr and Lr % (15 * Nr) != 0
    rng = np.random.default_rng(3)
    noise = lambda n: (0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    cap3, caps = np.concatenate([noise(L), iq[:, 0].reshape(-1)]), np.concatenate([noise(Lr), x[:, 0].reshape(-1)])
    r3, s3 = la.cell_search(cap3, 100, nof_periods=1)
    rs, ss = la.cell_search(caps, 100, nof_periods=1, rates=la.RATES_SRSRAN)
    assert r3 == rs == 1 and ss.cell_id == s3.cell_id == 401 and ss.cp == s3.cp == 0 and ss.sf_idx == s3.sf_idx
    assert abs(int(ss.sf_start) - int(s3.sf_start) * Nr / N) <= 1.0, (ss.sf_start, s3.sf_start)
    k = (ss.sf_idx - tti0) % 5                                   # the stream's subframe that sf_start points at
    assert abs(int(ss.sf_start) - (Lr + k * 15 * Nr)) <= 1, (ss.sf_start, Lr, k)
    # The replay starts at the search's own answer, as a user's would: a start one sample off (the tolerance above) moves the FFT window by one sample, which
    # the receiver has to take (early: a phase ramp inside the cyclic prefix; late: 1 / 1536 of the next symbol's prefix leaks in, 32 dB down).
    first0 = k + ((10 - ss.sf_idx) % 10)                         # subframe 0 of the next radio frame
    off = int(ss.sf_start) + (first0 - k) * 15 * Nr
    phy = _phy(sc, 8)
    m = phy.mib_decode(caps[off:off + 15 * Nr][None])
    assert m["found"] == 1 and (m["nof_prb"], m["nof_ports"]) == (100, sc["nof_ports"]) and m["sfn"] == ((tti0 + first0) // 10) % 1024
    _, _, orecs = run_oracle(sc, tti0 + first0, iq[first0:], taps=False)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "capture.cf32")
        caps.tofile(path)
        n = phy.process_file(path, start_tti=m["sfn"] * 10, offset_time=off)
    assert n >= 30 - first0 - 1
    g, o = gpu_records(phy), oracle_records(orecs)
    phy.close()
    if n < 30 - first0:   # a start one sample late leaves the last subframe of the file one sample short: its records are not there to compare
        last = (tti0 + 29) % 10240
        fs = ((last // 10) << 4) | (last % 10)
        o = [r for r in o if (r[10] << 8 | r[11]) != fs]
    assert len(o) > 10 and g == o, (len(g), len(o))


@pytest.mark.parametrize("nof_prb", [50, 100])
def test_ul_mode_pusch_records_equal_the_oracle_at_the_3gpp_rate(nof_prb):
    """UL_MODE at 768 / 1536 samples per symbol: antenna 0 downlink, antenna 1 uplink (converted between the half-carrier shifts).  DCI 0 at t, DMRS
    estimate and PUSCH decode at t + 4: uplink and downlink records equal to the oracle's UL_MODE worker on the 3GPP-rate capture"""
    sc, tti0, iq, orecs, otrace = ul_mode_stream(nof_prb)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == []
    assert sum(1 for r in orecs if r[1] == 0) >= 10 and sum(1 for r in orecs if r[1] == 1) >= 5
    x = converted(sc, iq, uplink_antennas=(1,))
    phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=16, pcapwriter=la.PcapWriter(None))
    assert phy.set_sampling(la.RATES_SRSRAN) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"]) and phy.setUlConfig(3, 5)
    phy.process_host(x, tti0, 25)
    g = gpu_records(phy)
    phy.close()
    assert g == orecs, "UL_MODE records differ: gpu %d vs oracle %d" % (len(g), len(orecs))


@pytest.mark.parametrize("nof_prb,zcz,root,fo", [(50, 5, 10, 4), (100, 1, 700, 20), (100, 12, 837, 94)])
def test_prach_detections_equal_the_oracle_at_the_3gpp_rate(nof_prb, zcz, root, fo):
    """PRACH-only uplink subframes (no PUSCH in them), each converted over the detector's own window: the product at 12 x 768 / 12 x 1536 samples finds the
    preambles the oracle finds at the 3GPP rate, each timing within one lag of the 839-point correlation"""
    from lsn_testlib import oracle_prach_api, prach_subframe
    from rate_convert import convert_prach_subframe
    from test_gpu_prach import oracle_run
    o = oracle_prach_api()
    N = SYMBOL_SZ_3GPP[nof_prb]
    rng = np.random.default_rng(nof_prb + zcz)
    sfs, want = [], []
    for s in range(4):
        ues = [(int(rng.integers(0, 64)), int(rng.integers(0, 150) * N / 2048), float(rng.uniform(-3, 3))) for _ in range(s)]   # delays inside the prefix
        ues = list({u[0]: u for u in ues}.values())
        iq = prach_subframe(nof_prb, ues, snr_db=6.0, seed=200 + s, zero_corr_zone=zcz, root_seq_idx=root, freq_offset=fo)
        det, _ = oracle_run(o, nof_prb, iq, 14, root, zcz, fo)
        assert sorted(d[0] for d in det) == sorted(u[0] for u in ues)
        want.append(sorted((d[0], d[1]) for d in det))
        sfs.append(convert_prach_subframe(iq, nof_prb))
    phy = la.Phy(nof_rx_antennas=1, max_batch=4)
    assert phy.set_sampling(la.RATES_SRSRAN) and phy.setCell(nof_prb, 1, 1) and phy.setPrachConfig(14, root, zcz, fo)
    got = phy.prach_detect(np.stack(sfs), start_tti=7)
    phy.close()
    for s, w in enumerate(want):
        mine = sorted((d["preamble"], d["offset"]) for d in got if d["sf"] == s)
        assert [m[0] for m in mine] == [a[0] for a in w], (s, mine, w)
        assert all(abs(m[1] - a[1]) <= 1 for m, a in zip(mine, w)), (s, mine, w)


@pytest.mark.parametrize("i", [14, 20, 27, 30])
def test_control_chain_on_spec_transmitter_grids_modulated_at_srsran_rate(i, monkeypatch):
    """tests/spec_downlink.py (the transmitter written from TS 36.211 / 36.212 alone, independent of txgen, the oracle and the rate converter) modulating its
    grid directly at N_r = 384 / 768 / 1024 / 1536: CFI, soft bits against the float64 model, CCE power and every placed DCI as in test_gpu_spec_control.py
    (cases 14, 20, 27, 30 of its covering design: 25 PRB 2 ports, 50 PRB 2 ports, 75 PRB 2 ports extended CP, 100 PRB 1 port)"""
    import spec_downlink as SD
    from test_gpu_spec_control import _gpu_checks
    from test_spec_control_oracle import BWS, case
    nprb = BWS[i // 6]
    monkeypatch.setitem(SD.FFT, nprb, SYMBOL_SZ_SRSRAN[nprb])
    p, iq, truth = case(i)
    assert iq.shape[1] == 15 * SYMBOL_SZ_SRSRAN[nprb]
    phy = la.Phy(nof_rx_antennas=p["nof_rx"], max_batch=4)
    assert phy.set_sampling(la.RATES_SRSRAN) and phy.setCell(p["nof_prb"], p["nof_ports"], p["cell_id"], SD.PHICH_NG[p["ng_x6"]], cp=p["cp"])
    phy.setCandidatePruning(la.Phy.PRUNE_OFF)
    phy.process_host(iq[None], 10 * p["sfn"] + p["sf_idx"], 0)
    _gpu_checks(phy, p, truth)
    phy.close()


@pytest.mark.parametrize("nprb,ports,q", [(25, 1, 0), (50, 2, 1), (75, 4, 2), (100, 2, 3)])
def test_mib_of_spec_transmitter_grids_modulated_at_srsran_rate(nprb, ports, q, monkeypatch):
    import spec_downlink as SD
    monkeypatch.setitem(SD.FFT, nprb, SYMBOL_SZ_SRSRAN[nprb])
    p = dict(nof_prb=nprb, nof_ports=ports, cp=q // 2, nof_rx=1 + q % 2, ng_x6=(1, 3, 6, 12)[q], cfi=1 + q % 3, cell_id=(0, 503, 301, 77)[q], sf_idx=0, sfn=4 * 57 + q)
    iq, truth = SD.control_subframe(seed=40 + q, **p)
    assert iq.shape[1] == 15 * SYMBOL_SZ_SRSRAN[nprb]
    phy = la.Phy(nof_rx_antennas=p["nof_rx"], max_batch=4)
    assert phy.set_sampling(la.RATES_SRSRAN) and phy.setCell(nprb, ports, p["cell_id"], SD.PHICH_NG[p["ng_x6"]], cp=p["cp"])
    g, llr = phy.mib_decode(iq, with_llr=True)
    mib = int("".join(map(str, truth["mib"])), 2)
    assert g["found"] == 1 and (g["sfn"], g["sfn_offset"], g["nof_prb"], g["nof_ports"], g["phich_resources_x6"], g["phich_length"], g["mib_bits"]) == \
        (p["sfn"], q, nprb, ports, p["ng_x6"], 0, mib), (p, g)
    n = len(truth["pbch_bits"])
    assert np.array_equal(llr[:n] > 0, truth["pbch_bits"] == 1) and not np.any(llr[n:])
    phy.close()
