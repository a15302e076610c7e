"""Per-grant uplink arrival time on the GPU (lsn_phy_set_ul_timing; k_pusch_toa, k_ul_fft_win of ul_timing.hip): (a) the measurement against the float64 model
on the product's own grid, inside the model's float32 bound, with everything else bit for bit as without it; (b) the re-cut window inside the first prefix,
bit for bit the oracle on the subframe as it was sent; (c) the rows of the measured table that fail in the common window: lost in mode 0, decoded in mode 2,
bit for bit the oracle on the re-cut buffer; (d) two UEs with different arrivals on one subframe; (e) UL_MODE with the uplink antenna early by N / 8;
(f) what the interface refuses.  The points, the model, the bound and the conditions on the inputs are tests/ul_timing_model.py's; the CPU side of every point
is checked in tests/test_ul_timing_model.py."""
import os

import numpy as np
import pytest

import ltesniffer_amd as la
import spec_uplink as SU
import ul_timing_model as M
from lsn_testlib import OracleWorkerUl, parse_pcap
from parity import gpu_records, oracle_records
from test_spec_pusch_oracle import UL_STREAMS, check_ul_records, oracle_grant, oracle_grid, receiver_grant, ul_stream

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ul_timing.txt")
TOA_LINE = "k_pusch_toa against the float64 model"
_worst = {}


def _phy(cell):
    phy = la.Phy(nof_rx_antennas=1)
    assert phy.setCell(cell["nof_prb"], 1, cell["cell_id"], cp=cell["cp"])
    assert phy.setUlConfig(cell["cyclic_shift"], cell["delta_ss"], cell["hopping_offset"], cell["group_hopping"], cell["sequence_hopping"])
    return phy


def _decode(phy, buf, sf, grants, mode, **thr):
    """-> per grant dict(crc_ok, iterations, snr_db bits, payload, llr, cbs, timing)"""
    assert phy.setUlTiming(mode, **thr) == la.LSN_SUCCESS
    res = phy.pusch_decode(np.asarray(buf, dtype=np.complex64)[None], 10 * 37 + sf, grants)
    tim = phy.pusch_timing()
    assert len(tim) == len(grants)
    out = []
    for k, (r, g) in enumerate(zip(res, grants)):
        out.append(dict(crc_ok=r["crc_ok"], iterations=r["iterations"], snr=int(np.float32(r["snr_db"]).view(np.uint32)), snr_db=r["snr_db"], payload=r["payload"],
                        llr=phy.tap_ul_llr(k, 144 * g["L_prb"] * g["mod"]), cbs=phy.tap_ul_cbs(k), timing=tim[k]))
    return out


def _same(a, b, what):
    """two results of one grant, bit for bit: soft bits, code blocks with their de-rate-matched words, iterations, verdict, payload, the bits of snr_db"""
    assert np.array_equal(a["llr"], b["llr"]), (what, "llr")
    assert (a["crc_ok"], a["iterations"], a["payload"], a["snr"]) == (b["crc_ok"], b["iterations"], b["payload"], b["snr"]), (what, a["crc_ok"], b["crc_ok"], a["snr_db"], b["snr_db"])
    key = lambda c: (c["K"], c["F"], c["E"], c["rv"], c["ok"], c["iters"])
    assert [key(c) for c in a["cbs"]] == [key(c) for c in b["cbs"]], what
    for x, y in zip(a["cbs"], b["cbs"]):
        assert np.array_equal(x["d3"], y["d3"]), (what, "d3")


def _oracle(cell, sf, buf, rg):
    o = oracle_grant(cell, sf, oracle_grid(cell, buf), rg)
    o["snr"] = int(np.float32(o["snr_db"]).view(np.uint32))
    return o


def _rows(cell, grid):
    nre = 12 * cell["nof_prb"]
    return np.asarray(grid).reshape(-1)[:(12 if cell["cp"] else 14) * nre]


# ---------------------------------------------------------------------------------------------------------------------------- (a)
@pytest.fixture(scope="module", autouse=True)
def _profile_line():
    yield
    if not _worst:
        return
    name, (ratio, err, bound) = max(_worst.items(), key=lambda kv: kv[1][0])
    line = "%s: largest |tau - tau64| / bound = %.4f (|tau - tau64| = %.3e samples, bound %.3e) at %s, over %d points\n" % (TOA_LINE, ratio, err, bound, name, len(_worst))
    try:
        old = [l for l in open(PROFILE).read().splitlines(True) if not l.startswith(TOA_LINE)] if os.path.exists(PROFILE) else []
        with open(PROFILE, "w") as f:
            f.writelines(old + [line])
    except OSError:
        pass


@pytest.mark.parametrize("cp", (0, 1))
@pytest.mark.parametrize("name", sorted(M.TOA_GRANTS))
def test_toa_against_the_model(name, cp):
    cell, sf, iq, t = M.toa_case(name, cp)
    rg = receiver_grant(t)
    N = SU.FFT[cell["nof_prb"]]
    phy = _phy(cell)
    for a in M.toa_arrivals(N):
        buf = M.early(iq, a)
        r0 = _decode(phy, buf, sf, [rg], 0)[0]
        assert r0["timing"] == dict(measured=0, tau=0.0, shift=0, flags=0, residual=0.0, toa_us=0.0, confidence=0.0)
        r1 = _decode(phy, buf, sf, [rg], 1)[0]
        _same(r1, r0, (name, cp, a))
        tm = r1["timing"]
        m = M.toa(cell, sf, rg, phy.tap_ul_grid(0))          # the model on the product's own grid
        err = abs(tm["tau"] - m["tau"])
        print("toa", name, cp, a, "tau %.5f model %.5f err %.3e bound %.3e" % (tm["tau"], m["tau"], err, m["bound"]))
        _worst[(name, cp, a)] = (err / m["bound"], err, m["bound"])
        assert err <= m["bound"], (a, tm["tau"], m["tau"], m["bound"])
        assert M.half_distance(m["tau"]) >= M.HALF_MARGIN
        assert (tm["shift"], tm["flags"]) == M.decide(m["tau"], N), (a, tm, m["tau"])
        assert tm["measured"] == 1 and tm["residual"] == 0.0 and abs(tm["confidence"] - m["conf"]) <= 1e-4 * m["conf"]
        assert tm["toa_us"] == pytest.approx(tm["tau"] / (15000.0 * N) * 1e6, rel=1e-5, abs=1e-9)
        with pytest.raises(RuntimeError):
            phy.tap_ul_priv_grid(0)                          # nothing was re-cut
    phy.close()


# ---------------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", sorted(M.RECUT_EXACT))
def test_recut_inside_the_first_prefix(name):
    cell, sf, iq, t = M.toa_case(name, 0)
    rg = receiver_grant(t)
    want = _oracle(cell, sf, iq, rg)
    assert want["crc_ok"] == 1 and want["payload"] == t["payload"]
    want_grid = _rows(cell, oracle_grid(cell, iq))
    phy = _phy(cell)
    for a in M.RECUT_EXACT[name]:
        buf = M.early(iq, a)
        r2 = _decode(phy, buf, sf, [rg], 2, min_shift=1)[0]
        assert r2["timing"]["shift"] == a and r2["timing"]["flags"] == (la.TOA_FLAG_BELOW if a == 0 else 0), (a, r2["timing"])
        _same(r2, want, (name, a))
        assert np.array_equal(_rows(cell, phy.tap_ul_priv_grid(0)).view(np.uint32), want_grid.view(np.uint32)), a
        mr = M.toa(cell, sf, rg, phy.tap_ul_priv_grid(0))     # the residual is the same measurement on the private rows
        assert abs(r2["timing"]["residual"] - mr["tau"]) <= mr["bound"] and abs(mr["tau"]) < 0.5, (a, r2["timing"], mr["tau"])
        if a == 0:     # no transform: the private rows are the common ones, the results those of mode 0
            assert np.array_equal(_rows(cell, phy.tap_ul_priv_grid(0)).view(np.uint32), _rows(cell, phy.tap_ul_grid(0)).view(np.uint32))
            _same(r2, _decode(phy, buf, sf, [rg], 0)[0], (name, "mode 0"))
    phy.close()


# ---------------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("row", [r for r in M.TABLE if not r[5]], ids=lambda r: "%dprb_L%d_mcs%d_a%d" % (r[0], r[2], r[3], r[4]))
def test_beyond_the_prefix(row):
    a = row[4]
    cell, sf, iq, t = M.table_case(row)
    rg = receiver_grant(t)
    buf = M.early(iq, a)
    phy = _phy(cell)
    r0 = _decode(phy, buf, sf, [rg], 0)[0]
    assert r0["crc_ok"] == 0
    r2 = _decode(phy, buf, sf, [rg], 2)[0]
    tm = r2["timing"]
    print("beyond", row, tm, r0["snr_db"], r2["snr_db"])
    assert r2["crc_ok"] == 1 and r2["payload"] == t["payload"]
    assert abs(tm["shift"] - a) <= M.arrival_tolerance(a) and abs(tm["residual"]) <= M.arrival_tolerance(a), tm
    m = M.toa(cell, sf, rg, phy.tap_ul_grid(0))
    assert abs(tm["tau"] - m["tau"]) <= m["bound"] and (tm["shift"], tm["flags"]) == M.decide(m["tau"], SU.FFT[cell["nof_prb"]]), (tm, m["tau"])
    mr = M.toa(cell, sf, rg, phy.tap_ul_priv_grid(0))
    assert abs(tm["residual"] - mr["tau"]) <= mr["bound"], (tm, mr["tau"])
    cut = M.recut(buf, tm["shift"])
    _same(r2, _oracle(cell, sf, cut, rg), row)
    assert np.array_equal(_rows(cell, phy.tap_ul_priv_grid(0)).view(np.uint32), _rows(cell, oracle_grid(cell, cut)).view(np.uint32))
    assert tm["toa_us"] == pytest.approx((tm["shift"] + tm["residual"]) / (15000.0 * SU.FFT[cell["nof_prb"]]) * 1e6, rel=1e-5)
    phy.close()


# ---------------------------------------------------------------------------------------------------------------------------- (d)
def test_two_ues_on_one_subframe():
    cell, sf, iq, truths, arr = M.two_ues()
    grants = [receiver_grant(t) for t in truths]
    phy = _phy(cell)
    r0 = _decode(phy, iq, sf, grants, 0)
    assert [r["crc_ok"] for r in r0] == [1, 0]
    r2 = _decode(phy, iq, sf, grants, 2)
    for k, (r, t, a) in enumerate(zip(r2, truths, arr)):
        assert r["crc_ok"] == 1 and r["payload"] == t["payload"], k
        assert abs(r["timing"]["shift"] - a) <= M.arrival_tolerance(a) and (r["timing"]["shift"] != 0) == (a != 0), r["timing"]
        _same(r, _oracle(cell, sf, M.recut(iq, r["timing"]["shift"]), grants[k]), k)      # each UE in its own window
    _same(r2[0], r0[0], "the UE inside the prefix is untouched")
    phy.close()


# ---------------------------------------------------------------------------------------------------------------------------- (e)
def _ul_mode(sc, tti0, iq, mode, max_batch):
    phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=max_batch, pcapwriter=la.PcapWriter(None))
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], cp=sc["cp"]) and phy.setUlConfig(sc["cyclic_shift"], sc["delta_ss"], sc["hopping_offset"])
    assert phy.setUlTiming(mode) == la.LSN_SUCCESS
    phy.process_host(iq, tti0, 25)
    return phy, parse_pcap(phy.pcapwriter.bytes())


def _oracle_ul_mode(sc, tti0, iq):
    ow = OracleWorkerUl(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], sc["cyclic_shift"], sc["delta_ss"], sc["hopping_offset"], cp=sc["cp"])
    for j in range(iq.shape[0]):
        ow.work_ul(iq[j, 0], iq[j, 1], (tti0 + j) % 10240, update_meta=1 if j == 0 else 0)
    return parse_pcap(ow.pcap_bytes())


@pytest.mark.parametrize("k", range(len(UL_STREAMS)))
def test_ul_mode_with_the_uplink_antenna_early(k):
    """The uplink antenna's stream early by N / 8, the downlink antenna untouched.  Mode 0 is the oracle worker on the same stream: no uplink record for
    streams 0 and 2; stream 1 (16QAM at MCS 12 on six PRB, rate 0.3) survives N / 8 in the common window on the oracle as well, which is asserted as such."""
    sc, tti0, iq, want = ul_stream(k)
    N = SU.FFT[sc["nof_prb"]]
    a = N // 8
    early = iq.copy()
    early[:, 1] = M.early(iq[:, 1].reshape(-1), a).reshape(iq.shape[0], -1)
    assert np.array_equal(early[:, 0], iq[:, 0])
    orecs = _oracle_ul_mode(sc, tti0, early)
    n_ul = sum(r["direction"] == 0 for r in orecs)
    assert n_ul == (1 if k == 1 else 0)
    phy, recs0 = _ul_mode(sc, tti0, early, 0, 4)
    assert oracle_records(recs0) == oracle_records(orecs) and sum(r["direction"] == 0 for r in recs0) == n_ul
    st = phy.ul_ue_stats(want[0][0])
    assert st is None or (st["measured"] == 0 and st["mean_toa_us"] == 0.0 and st["mean_toa_samples"] == 0.0)
    phy.close()
    per_batch = []
    for mb in (1, 4):
        phy, recs2 = _ul_mode(sc, tti0, early, 2, mb)
        check_ul_records(recs2, want)
        assert oracle_records([r for r in recs2 if r["direction"] != 0]) == oracle_records([r for r in orecs if r["direction"] != 0])
        st = phy.ul_ue_stats(want[0][0])
        print("ul_mode", k, mb, st)
        assert st is not None and st["active"] == 1 and st["success"] == 1 and st["measured"] == 1, st
        assert abs(st["mean_toa_samples"] - a) <= 1.0 and st["mean_toa_us"] == pytest.approx(st["mean_toa_samples"] / (15000.0 * N) * 1e6, rel=1e-5), st
        assert st["mean_snr_db"] >= 1.0
        per_batch.append(oracle_records(recs2))
        phy.close()
    assert per_batch[0] == per_batch[1]
    # the streams as they were sent: mode 2 gives the records of mode 0
    phy, plain0 = _ul_mode(sc, tti0, iq, 0, 4)
    phy.close()
    phy, plain2 = _ul_mode(sc, tti0, iq, 2, 4)
    phy.close()
    assert oracle_records(plain2) == oracle_records(plain0)
    check_ul_records(plain2, want)


# ---------------------------------------------------------------------------------------------------------------------------- (f)
def test_refusals():
    import torch
    from lsn_testlib import scenario
    from parity import gen_subframes
    sc = scenario("small", seed=7)
    tti0, iq, _ = gen_subframes(sc, 12)
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=12, device=0, pcapwriter=la.PcapWriter(None))
    assert phy.setUlTiming(1) == la.LSN_ERROR                                  # no cell: the thresholds are in samples of the cell
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
    N = SU.FFT[sc["nof_prb"]]
    assert phy.setUlTiming(3) == la.LSN_ERROR_INVALID_INPUTS
    assert phy.setUlTiming(2, 0, N // 2 + 1) == la.LSN_ERROR_INVALID_INPUTS and phy.setUlTiming(2, N // 2 + 1, 0) == la.LSN_ERROR_INVALID_INPUTS
    assert phy.setUlTiming(2, 1, N // 2) == la.LSN_SUCCESS and phy.setUlTiming(0) == la.LSN_SUCCESS
    with pytest.raises(RuntimeError):
        phy.ul_ue_stats(0x1234)                                                # a DL_MODE Phy
    d_iq = torch.from_numpy(iq.view(np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    phy.submit_device(d_iq.data_ptr(), 12, tti0)
    assert phy.setUlTiming(1) == la.LSN_ERROR                                  # a submitted block is in flight
    phy.wait()
    assert phy.setUlTiming(1) == la.LSN_SUCCESS
    phy.close()
