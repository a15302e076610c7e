#!/usr/bin/env python3
"""tools/srs_rate_probe.py - what the srsRAN sampling mode does to the link-bound legs (a measurement, no pass / fail).

The cfg3 capture of bench.py (tools/make_cfg3_golden.py: scenario("cfg3", seed=3), 20 MHz, two antennas) is rewritten at 23.04 MS/s by
tests/rate_convert.py and decoded in LSN_RATES_SRSRAN mode, interleaved with the same legs on the original 30.72 MS/s capture in the default mode:
  host    lsn_phy_process_host from a page-locked buffer (first H2D copy to last PDU): a cold pass, then `--passes - 1` warm passes with the TTI
          advancing and every sequential state carried over, as bench.py replays its stream
  file    lsn_phy_process_file of the capture written as cf32 (cold state)
  device  lsn_phy_process_device with the capture resident in HBM (cold state): the rate with no link in the way
Every pass is hashed in blocks of 200 subframes (lsn_pcap_set_digest_blocks) and compared with tests/golden/cfg3_stream_oracle.json; the number of differing
blocks is printed next to each figure.  The golden stream walks the 20 000 distinct subframes: with --subframes below 20 000 only passes from cold state
have an oracle block to be compared with, and warm passes are printed as "ungated".

  python tools/srs_rate_probe.py [--subframes 20000] [--passes 3] [--rounds 2] [--out profiles/srs_rates_probe.txt]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=20000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import ltesniffer_amd as la
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    from rate_convert import convert_subframes
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")))["blocks"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq3 = gen_capture(sc, nsf)
    caps = {la.RATES_3GPP: iq3}
    srs = np.empty((nsf, sc["nof_rx"], 15 * 1536), dtype=np.complex64)
    for b in range(0, nsf, 200):
        srs[b:b + 200] = convert_subframes(iq3[b:b + 200], 100)
    caps[la.RATES_SRSRAN] = srs
    say("srs_rate_probe: cfg3 capture, %d of %d distinct subframes, 2 antennas; rendered and converted in %.0f s" % (nsf, NSF, time.time() - t))
    for r, name in ((la.RATES_3GPP, "30.72 MS/s"), (la.RATES_SRSRAN, "23.04 MS/s")):
        per = caps[r].shape[2] * 8
        say("  %s: %d bytes per subframe and antenna, %d per subframe" % (name, per, per * sc["nof_rx"]))
    pinned = {r: torch.from_numpy(c).pin_memory() for r, c in caps.items()}
    td = tempfile.mkdtemp(prefix="srs_probe_")
    files = {}
    for r, c in caps.items():
        files[r] = os.path.join(td, "cap_%d.cf32" % r)
        with open(files[r], "wb") as f:
            for b in range(0, nsf, 200):
                np.ascontiguousarray(c[b:b + 200].transpose(0, 2, 1)).tofile(f)

    def gate(w, first_block):
        blocks = w.block_digests()
        if first_block + len(blocks) > len(golden) or (nsf < NSF and first_block):
            return "ungated"
        bad = sum(1 for j, (d, c) in enumerate(blocks) if ["%016x" % d, c] != list(golden[first_block + j]))
        return "%d of %d blocks differ" % (bad, len(blocks))

    def phy_for(r, w):
        phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=a.batch, pcapwriter=w)
        assert phy.set_sampling(r) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
        return phy

    def writer(first_tti):
        w = la.PcapWriter(None)
        w.set_store(False)
        w.set_digest_blocks(BLOCK, first_tti)
        return w

    def leg_host(r):
        w = writer(tti0)
        phy = phy_for(r, w)
        out = []
        for p in range(a.passes):
            w.reset()
            w.set_digest_blocks(BLOCK, (tti0 + p * nsf) % 10240)
            t0 = time.perf_counter()
            la._check(la.lib().lsn_phy_process_host(phy._h, pinned[r].data_ptr(), nsf, (tti0 + p * nsf) % 10240, META), "process_host")
            dt = time.perf_counter() - t0
            out.append("%s %.0f sf/s (%s)" % ("cold" if p == 0 else "warm", nsf / dt, gate(w, p * nsf // BLOCK)))
        phy.close()
        return ", ".join(out)

    def leg_file(r):
        w = writer(tti0)
        phy = phy_for(r, w)
        phy.prepare_file()
        t0 = time.perf_counter()
        n = phy.process_file(files[r], start_tti=tti0, update_meta_period=META)
        dt = time.perf_counter() - t0
        s = "cold %.0f sf/s (%s)" % (n / dt, gate(w, 0))
        phy.close()
        return s

    def leg_device(r):
        n = min(nsf, 4000)   # 4000 subframes at 30.72 MS/s are 1.97 GB of HBM
        d = torch.from_numpy(caps[r][:n].view(np.float32)).to("cuda:0")
        torch.cuda.synchronize()
        w = writer(tti0)
        phy = phy_for(r, w)
        t0 = time.perf_counter()
        phy.process_device(d.data_ptr(), n, tti0, META)
        dt = time.perf_counter() - t0
        s = "cold %.0f sf/s over %d subframes (%s)" % (n / dt, n, gate(w, 0))
        phy.close()
        del d
        return s

    try:
        for rnd in range(a.rounds):
            for leg, fn in (("host pinned", leg_host), ("file cf32", leg_file), ("device resident", leg_device)):
                for r, name in ((la.RATES_3GPP, "30.72 MS/s 3GPP"), (la.RATES_SRSRAN, "23.04 MS/s srsRAN")):
                    say("round %d  %-16s %-18s %s" % (rnd + 1, leg, name, fn(r)))
    finally:
        for f in files.values():
            os.remove(f)
        os.rmdir(td)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
