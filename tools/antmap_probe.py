#!/usr/bin/env python3
"""tools/antmap_probe.py - UL_MODE from ONE antenna of a 61.44 MS/s recording through the antenna map, against the same capture as an ordinary two-antenna
recording (a measurement, no pass / fail).  DESIGN.md section 3.1s.

The 25-PRB UL_MODE capture of tests/antmap_cases.py ("61": downlink at +15 MHz, uplink at -15 MHz of one antenna; 12 subframes) is continued periodically to
--subframes subframes and written twice as cf32: the one-antenna recording, and the baseline - both antennas of the capture at +15 MHz of a two-antenna recording,
twice the bytes.  Two ways, interleaved round by round, each from a cold UL_MODE Phy with the block buffers reserved, timed around the replay call only:
  (a) unmapped   process_file_rate of the two-antenna recording: k_resample_wide, grid.y = 2 antennas read, 2 rows written
  (b) mapped     set_antenna_map(src=(0, 0), offset_hz=(0, -30 MHz)) and process_file_rate of the one-antenna recording: k_resample_map_wide, the one antenna read
                 twice with two tuning words, 2 rows written
Printed per leg: cell-subframes per second, bytes of the file read and copied per cell-subframe, the number of records and whether the record digest equals the
unmapped leg's of the same round (the continued capture repeats its 12 subframes under a running TTI, so the records are not the oracle's; both ways must decode
the same ones).  Last line: the median of the rounds per way.

  python tools/antmap_probe.py [--subframes 800] [--rounds 3] [--block 100] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every replay")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["LSN_FILE_BLOCK"] = str(a.block)
    import numpy as np
    import ltesniffer_amd as la
    from antmap_cases import extended, ul_recording
    from resample_cases import LEAD
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    sc, tti0, _, _, _, _, _ = ul_recording("61")
    rate_in, fc, f1, f2 = extended("61", a.subframes)
    nsf = -(-a.subframes // 12) * 12   # whole periods of the 12-subframe capture
    td = tempfile.mkdtemp(prefix="antmap_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    files = {"unmapped": (os.path.join(td, "two.cf32"), 2), "mapped": (os.path.join(td, "one.cf32"), 1)}
    f2.tofile(files["unmapped"][0])
    f1.tofile(files["mapped"][0])
    assert f1.dtype == f2.dtype == np.complex64
    del f1, f2
    say("antmap_probe: 25-PRB UL_MODE capture, %d subframes, in a %.2f MS/s recording (downlink %+.1f MHz, uplink %+.1f MHz), cf32, LSN_FILE_BLOCK %d, library %s; built in %.0f s" %
        (nsf, rate_in / 1e6, fc / 1e6, -fc / 1e6, a.block, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
    for way, (p, nant) in files.items():
        size = os.path.getsize(p)
        say("  %-9s %d antenna(s), %d bytes; read and copied per cell-subframe: %d" % (way, nant, size, size // nsf))
        with open(p, "rb", buffering=0) as fh:   # read once: the first read of freshly written page-cache pages is slow whoever reads them
            buf = bytearray(64 << 20)
            while fh.readinto(buf):
                pass

    def leg(way, yard):
        p, nant = files[way]
        w = la.PcapWriter(None)
        phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=100, pcapwriter=w)
        assert phy.set_sampling(la.RATES_3GPP) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"]) and phy.setUlConfig(3, 5)
        phy.prepare_file()
        if way == "mapped":
            assert phy.set_antenna_map(src=(0, 0), offset_hz=(0.0, -2.0 * fc))
        t0 = time.perf_counter()
        done = phy.process_file_rate(p, rate_in, center_offset_hz=fc, start_tti=tti0, offset_time=LEAD, update_meta_period=25, nof_antennas=nant)
        dt = time.perf_counter() - t0
        digest, n = w.digest(), w.nof_records()
        phy.close()
        if way == "unmapped":
            yard[:] = [digest]
        return done / dt, "%d subframes, %.0f cell-sf/s, %.1f ms, %d records (digest %s the unmapped replay's)" % (done, done / dt, dt * 1e3, n, "equals" if [digest] == yard else "DIFFERS from")

    rates = {"unmapped": [], "mapped": []}
    try:
        for rnd in range(a.rounds):
            yard = []
            for way in ("unmapped", "mapped"):
                r, text = leg(way, yard)
                rates[way].append(r)
                say("round %d  %-9s %s" % (rnd + 1, way, text))
    finally:
        for p, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    say("median of %d rounds: unmapped %.0f cell-sf/s, mapped %.0f cell-sf/s" % (a.rounds, statistics.median(rates["unmapped"]), statistics.median(rates["mapped"])))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
