"""The HIP PDSCH chain (DCI search and grant conversion on the host, k_pdsch_demod, k_rm, k_turbo) on the streams of the independent spec transmitter
(tests/spec_pdsch.py, tests/spec_dci.py): the ground-truth checks of tests/test_spec_pdsch_oracle.py on the product's own stage-C taps and record
stream, then bit-exact parity with the oracle on the same streams, which reach parameter points no txgen stream does.  The cases, the checks and the
three documented departures (band-edge channel estimate, a grant whose first block is disabled, P_B on one port) are described in that file."""
import numpy as np
import pytest

import ltesniffer_amd as la
import spec_downlink as SD
from lsn_testlib import oracle_trace, parse_pcap
from parity import compare_stage_c, compare_taps, gpu_records, oracle_records, run_oracle
from test_spec_pdsch_oracle import CASES, NCASES, NOISY, NOISY_SNR_DB, case, check_accepted, check_job, check_records, matching_jobs

pytestmark = pytest.mark.gpu


def _run(i, snr_db=None):
    p, iq, truth, records, dci = case(i, snr_db)
    tti = 10 * p["sfn"] + p["sf_idx"]
    phy = la.Phy(nof_rx_antennas=p["nof_rx"], max_batch=4, pcapwriter=la.PcapWriter(None))
    assert phy.setCell(p["nof_prb"], p["nof_ports"], p["cell_id"], SD.PHICH_NG[p["ng_x6"]], cp=p["cp"])
    phy.set_stage_c_taps(True)
    phy.process_host(iq[None], tti, 0)
    assert int(phy.tap(la.TAP_CFI, 0, np.uint32, 1)[0]) == p["cfi"], ("SET-UP: CFI", i)
    check_accepted(phy.tap(la.TAP_ACCEPTED, 0, np.uint32, 64 * 6).reshape(-1, 6), i, dci)
    check_records(parse_pcap(phy.pcapwriter.bytes()), records)
    return phy, p, iq, truth["pdsch"][0], tti


def _parity(phy, p, iq, tti):
    sc = dict(p, phich_ng_x6=p["ng_x6"])
    _, per_sf, orecs = run_oracle(sc, tti, iq[None], trace=True)
    otrace = oracle_trace()
    bad = compare_taps(phy, per_sf, sc, 0, 1)
    assert not bad, (p, bad[:3])
    bad, ncall, _, _, _ = compare_stage_c(phy, otrace, tti, 1)
    assert not bad and ncall == len(otrace), (p, ncall, len(otrace), bad[:3])
    assert gpu_records(phy) == oracle_records(orecs)


@pytest.mark.parametrize("i", range(NCASES))
def test_gpu_pdsch_chain_on_the_spec_transmitter(i):
    phy, p, iq, ch, tti = _run(i)
    jobs = phy.stage_c_jobs()
    if CASES[i].get("gated"):
        assert not [j for j in jobs if j["rnti"] == ch["rnti"]]
    else:
        mine = matching_jobs(jobs, ch, tti)
        assert len(mine) == 1, ("decode jobs with the transmitted parameters", len(mine), [(hex(j["rnti"]), j["qm"], j["nof_re"], j["have"]) for j in jobs])
        nchk, njudged = check_job(mine[0], ch, 12 * p["nof_prb"], i)
        assert nchk == sum(cw["seg"]["C"] for cw in ch["cw"]) and njudged == sum(cw["G"] for cw in ch["cw"])
        if CASES[i].get("t256"):    # the table is found by trial: the 64QAM-table attempt on the same elements fails
            first = [j for j in jobs if j["have"] and (j["tti"], j["rnti"], j["nof_re"]) == (tti, ch["rnti"], len(ch["res"])) and j["qm"] != mine[0]["qm"]]
            assert len(first) == 1 and not any(first[0]["crc"]) and not any(cb["ok"] for cb in first[0]["cbs"])
    _parity(phy, p, iq, tti)
    phy.close()


@pytest.mark.parametrize("i", NOISY)
def test_gpu_payloads_survive_awgn(i):
    phy, p, iq, _, tti = _run(i, NOISY_SNR_DB)
    _parity(phy, p, iq, tti)
    phy.close()
