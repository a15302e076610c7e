#!/usr/bin/env python3
"""tools/multicell_probe.py - the successive cell search on an MI355X: wall time of lsn_cell_search and of lsn_cell_search_all at 100 resource blocks and 8
periods on a two-cell head in host memory, and what a round after the first costs against a full re-correlation, written to profiles/multicell_search.txt
(a measurement, no pass / fail; there is no parent figure to compare with).

  head        one antenna, cf32, 30.72 MS/s, (8 + 1) 153600 + 2048 samples (11 MB): cell 301 (900 Hz off) plus cell 304 (-400 Hz off) 3 dB below it at another
              timing, from the synthetic transmitter.
  timed       cell_search (one correlation over 3 x 153600 lags, one SSS decision); cell_search_all with max_cells = 1 (the same plus the accumulated SSS
              decision and one cancellation) and with the default max_cells (two cells: one patched round and the round that finds nothing more);
              cell_search on the residual of lsn_pss_cancel: what every further round would cost if it correlated all lags again.
              --rounds times each; the first pass pays for the runtime's start and is shown apart.

  python tools/multicell_probe.py [--rounds 5] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import ltesniffer_amd as la
    from lsn_testlib import scenario, sync_capture
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    P, prb = 8, 100
    t = time.time()
    parts = []
    for cid, seed, lead, cfo in ((301, 5, 1234, 900.0), (304, 6, 36000, -400.0)):
        sc = scenario("small", seed=seed, start_tti=773, nof_prb=prb, cell_id=cid, cfo_hz=cfo)
        parts.append(sync_capture(sc, lead, P)[0])
    n = min(len(p) for p in parts)
    x = (parts[0][:n] + np.float32(10.0 ** (-3.0 / 20.0)) * parts[1][:n]).astype(np.complex64)
    say("head: %d samples at 30.72 MS/s (%.1f MB cf32), cells 301 and 304 (-3 dB), built in %.1f s" % (len(x), x.nbytes / 1e6, time.time() - t))

    def timed(what, f):
        ts, r = [], None
        for _ in range(a.rounds + 1):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        say("%-46s wall ms first %.1f, then %s (median %.1f)" % (what, ts[0], " ".join("%.1f" % v for v in ts[1:]), float(np.median(ts[1:]))))
        return r, float(np.median(ts[1:]))

    (rc, s), t_one = timed("cell_search", lambda: la.cell_search(x, prb, nof_periods=P))
    one, t_first = timed("cell_search_all, max_cells 1", lambda: la.cell_search_all(x, prb, nof_periods=P, max_cells=1))
    cells, t_all = timed("cell_search_all", lambda: la.cell_search_all(x, prb, nof_periods=P))
    say("cells: %s" % [(c.cell.cell_id, c.round, c.cell.pss_pos, round(c.cell.pss_p2avg, 1), round(c.sss_ratio, 2), round(c.rel_power_db, 2)) for c in cells])
    res, _ = la.pss_cancel(x, prb, s.n_id_2, s.pss_pos, cfo_hz=s.cfo_hz, nof_periods=P)
    _, t_full = timed("cell_search on the residual (all lags again)", lambda: la.cell_search(res, prb, nof_periods=P))
    rounds = max(c.round for c in cells) + (1 if len(cells) < 8 else 0) if cells else 0
    if rounds:
        say("a round after the first (patch of 4095 of 153600 lags, peaks, accumulated SSS, cancellation): %.2f ms each over %d round(s); a full re-correlation "
            "with one SSS decision: %.1f ms" % ((t_all - t_first) / rounds, rounds, t_full))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
