"""k_turbo with the short sub-block of a window first (lsn_turbo_core.h) against the oracle's decoder, through the stage-C taps: verdict and iteration count of
every code block the oracle decoded, on a 25-PRB cell (two ports, two antennas, MCS 0 - 28) at 30 dB and at an SNR where blocks need several iterations and
some fail.  What the captures must contain is checked on the ORACLE's trace (seed and length were picked from it on the CPU): one- and two-wavefront blocks with
W mod 16 zero, even and odd, late and failing decodes with a short sub-block, and chunks with more small blocks than decoder launches (the paired layout)."""
import pytest

import ltesniffer_amd as la
from lsn_testlib import oracle_trace, scenario
from parity import compare_stage_c, gen_capture, run_oracle

pytestmark = pytest.mark.gpu

NSF, BATCH = 48, 16
PAIR_KMAX = 2752   # LSN_TURBO_PAIR_KMAX: blocks up to this size share a workgroup, one per wavefront


def capture(snr_db, seed):
    sc = scenario("small", seed=seed, snr_db=snr_db, mcs_min=0, mcs_max=28, n_rnti=6, dl_min=1, dl_max=3, ul_min=0, ul_max=0)
    tti0, iq = gen_capture(sc, NSF, threads=4)
    run_oracle(sc, tti0, iq, taps=False, trace=True)
    return sc, tti0, iq, [o for o in oracle_trace() if not o["is_ul"]]


def decoded_blocks(otrace):
    """code blocks of the oracle's trace that first-block gating cannot take away from the product: the first block of a transport block, and the others when
    that first block passed -> list of (tti, K, windows, W mod 16, iterations, ok)"""
    out = []
    for o in otrace:
        first_ok = {}
        for c in o["cbs"]:
            first_ok.setdefault(c["tb"], c["ok"])
        seen = set()
        for c in o["cbs"]:
            if c["tb"] in seen and not first_ok[c["tb"]]:
                continue
            seen.add(c["tb"])
            P = la.turbo_nwin(c["K"])
            out.append((o["tti"], c["K"], P, (c["K"] // P) % 16, c["iters"], c["ok"]))
    return out


def coverage(blocks):
    """-> set of (two wavefronts?, 'zero' / 'even' / 'odd') the blocks cover"""
    return {(P > 64, "zero" if r == 0 else ("odd" if r & 1 else "even")) for _, _, P, r, _, _ in blocks}


ALL_CLASSES = {(two, r) for two in (False, True) for r in ("zero", "even", "odd")}


def run(snr_db, seed):
    sc, tti0, iq, otrace = capture(snr_db, seed)
    blocks = decoded_blocks(otrace)
    assert coverage(blocks) == ALL_CLASSES, sorted(ALL_CLASSES - coverage(blocks))
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=BATCH)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
    phy.set_stage_c_taps(True)
    i128 = la.KERNELS.index("k_turbo<128>")
    bad, ncall, ncb, it_o, it_g, launches, paired = [], 0, 0, 0, 0, 0, False
    for base in range(0, NSF, BATCH):
        phy.process_host(iq[base:base + BATCH], tti0 + base, 0)
        b, c, k, io, ig = compare_stage_c(phy, otrace, tti0 + base, BATCH)
        bad += [(base,) + x for x in b]
        ncall, ncb, it_o, it_g = ncall + c, ncb + k, it_o + io, it_g + ig
        now = int(phy.perf().kernel_launches[i128])
        small = sum(1 for t, K, _, _, _, _ in blocks if 0 <= (t - tti0 - base) % 10240 < BATCH and K <= PAIR_KMAX)
        paired = paired or small > now - launches > 0   # more small blocks than launches in this chunk: two of them shared a launch
        launches = now
    phy.close()
    print("%g dB: %d calls, %d code blocks compared (%d the gating cannot skip), iterations oracle %d product %d, %d launches" % (snr_db, ncall, ncb, len(blocks), it_o, it_g, launches))
    assert not bad, (len(bad), bad[:5])
    assert ncall == len(otrace) > 0 and ncb >= len(blocks) and it_o == it_g
    assert paired
    return blocks


def test_every_sub_block_class_decodes_as_the_oracle_at_30_db():
    run(30.0, SEED_HIGH)


def test_late_and_failing_decodes_with_a_short_sub_block_at_low_snr():
    blocks = run(SNR_LOW, SEED_LOW)
    assert any(it >= 3 and ok for _, _, _, _, it, ok in blocks), "no block needed three iterations"
    assert any(it == 12 and not ok and r != 0 for _, _, _, r, it, ok in blocks), "no failing block with a short sub-block"


# picked on the CPU from the oracle's trace alone (the conditions above hold for these; the tests fail when they do not)
SEED_HIGH, SEED_LOW, SNR_LOW = 5, 6, 10.0
