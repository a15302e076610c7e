"""The HIP uplink chain (k_ul_fft, k_pusch_chest, k_pusch_demod, k_rm, k_turbo) on the streams of the independent spec transmitter (tests/spec_uplink.py,
tests/spec_dci.py): the ground-truth checks of tests/test_spec_pusch_oracle.py on the product's own taps and results, then bit-exact parity with the oracle on the
same streams, which reach parameter points no txgen stream does.  The cases, the checks, the conditions on the inputs and the AWGN level are described in that file."""
import numpy as np
import pytest

import ltesniffer_amd as la
from parity import gpu_records, oracle_records
from test_spec_pusch_oracle import (CASES, NCASES, NOISY, NOISY_SNR_DB, UL_STREAMS, case, check_grant, check_ul_records, oracle_grant, oracle_grid, receiver_grant,
                                    run_oracle_ul_stream, ul_stream)
from lsn_testlib import parse_pcap

pytestmark = pytest.mark.gpu


def _phy(cell):
    phy = la.Phy(nof_rx_antennas=1)
    assert phy.setCell(cell["nof_prb"], 1, cell["cell_id"], cp=cell["cp"])
    assert phy.setUlConfig(cell["cyclic_shift"], cell["delta_ss"], cell["hopping_offset"], cell["group_hopping"], cell["sequence_hopping"])
    return phy


def _taps(phy, k, r, g):
    return dict(crc_ok=r["crc_ok"], payload=r["payload"], llr=phy.tap_ul_llr(k, 144 * g["L_prb"] * g["mod"]), cbs=phy.tap_ul_cbs(k))


def _run(i, snr_db=None):
    cell, sf, iq, truths = case(i, snr_db)
    tti = 10 * (200 + 3 * i) + sf
    grants = [receiver_grant(t) for t in truths]
    phy = _phy(cell)
    res = phy.pusch_decode(iq[None], tti, grants)
    # the truth of the transmitter on the product's own taps
    for k, (t, r, g) in enumerate(zip(truths, res, grants)):
        ncb, nllr = check_grant(_taps(phy, k, r, g), t, noisy=snr_db is not None)
        assert ncb == t["seg"]["C"] and nllr == t["G"]
    # parity with the oracle, bit for bit
    grid = oracle_grid(cell, iq)
    n = (12 if cell["cp"] else 14) * 12 * cell["nof_prb"]
    assert np.array_equal(phy.tap_ul_grid(0).reshape(-1)[:n].view(np.uint32), grid[:n].view(np.uint32)), i
    for k, (r, g) in enumerate(zip(res, grants)):
        o = oracle_grant(cell, sf, grid, g)
        got = _taps(phy, k, r, g)
        assert np.array_equal(got["llr"], o["llr"]), (i, k)
        assert (r["crc_ok"], r["iterations"], r["payload"]) == (o["crc_ok"], o["iterations"], o["payload"]), (i, k, r["crc_ok"], r["iterations"], o["crc_ok"], o["iterations"])
        assert np.float32(r["snr_db"]).view(np.uint32) == np.float32(o["snr_db"]).view(np.uint32), (i, k, r["snr_db"], o["snr_db"])
        assert [(c["K"], c["F"], c["E"], c["rv"], c["ok"], c["iters"]) for c in got["cbs"]] == [(c["K"], c["F"], c["E"], c["rv"], c["ok"], c["iters"]) for c in o["cbs"]], (i, k)
        for q, (a, b) in enumerate(zip(got["cbs"], o["cbs"])):
            assert np.array_equal(a["d3"], b["d3"]), ("k_rm differs from the oracle", i, k, q)
    return phy, cell, sf, iq, truths, tti


@pytest.mark.parametrize("i", range(NCASES))
def test_gpu_pusch_chain_on_the_spec_transmitter(i):
    phy, cell, sf, iq, truths, tti = _run(i)
    # (d): the RNTI / the cyclic-shift field off by one; verdicts as the oracle's
    wrong = [receiver_grant(t, rnti_xor=1) for t in truths] + [receiver_grant(t, nd_add=1) for t in truths]
    res = phy.pusch_decode(iq[None], tti, wrong)
    assert [r["crc_ok"] for r in res] == [0] * len(wrong)
    phy.close()


@pytest.mark.parametrize("i", NOISY)
def test_gpu_payloads_survive_awgn(i):
    phy = _run(i, NOISY_SNR_DB)[0]
    phy.close()


@pytest.mark.parametrize("k", range(len(UL_STREAMS)))
def test_gpu_ul_mode_from_a_spec_dci_format0(k):
    sc, tti0, iq, want = ul_stream(k)
    ow, orecs = run_oracle_ul_stream(k)
    phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=4, pcapwriter=la.PcapWriter(None))
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], cp=sc["cp"]) and phy.setUlConfig(sc["cyclic_shift"], sc["delta_ss"], sc["hopping_offset"])
    phy.process_host(iq, tti0, 25)
    assert gpu_records(phy) == oracle_records(orecs)
    check_ul_records(parse_pcap(phy.pcapwriter.bytes()), want)
    st, ost = phy.getStats(), ow.stats()
    assert st.nof_decoded_locations == ost.nof_decoded_locations and st.nof_subframes == ost.nof_subframes
    phy.close()
