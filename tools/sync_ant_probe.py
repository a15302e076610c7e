#!/usr/bin/env python3
"""tools/sync_ant_probe.py - what the search over all receive antennas costs on an MI355X, written to profiles/sync_ant.txt (a
measurement, no pass / fail).

  search   wall time of cell_search (k_pss_corr) against cell_search_ant (k_pss_corr_ant) with A = 1 and A = 2 on a 100-block head (N = 2048, 30.72 MS/s) of 8
           periods in host memory: white noise with a PSS train (tests/clock_cases.pss_train, 20 dB), the second antenna with noise of its own.  The yardstick is
           cell_search on the same box (profiles/multicell_search.txt holds an earlier box's figure for it).
  scan     a 61.44 MS/s two-antenna head at the 100 kHz raster (603 hypotheses), antenna = 0 against antenna = "all" (profiles/carrier_scan.txt: one antenna).

Every call ends in the library's own stream synchronise.  The legs are interleaved: --rounds rounds, each running every leg --calls times; a leg's figure is the
median of its rounds' medians.  The first call of a leg pays for the runtime's start and is shown apart.

  python tools/sync_ant_probe.py [--rounds 3] [--calls 5] [--out FILE] [--build-only]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-only", action="store_true", help="build the inputs and stop (a rehearsal without a GPU)")
    a = ap.parse_args()
    import numpy as np
    import ltesniffer_amd as la
    from clock_cases import pss_train
    from ddc_cases import carrier
    from resample_cases import fft_convert
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def measure(title, legs):
        """legs: [(name, call)] -> prints one line per leg"""
        first, rounds = {}, {n: [] for n, _ in legs}
        for n, f in legs:
            t = time.perf_counter()
            f()
            first[n] = (time.perf_counter() - t) * 1e3
        for _ in range(a.rounds):
            for n, f in legs:
                ts = []
                for _ in range(a.calls):
                    t = time.perf_counter()
                    f()
                    ts.append((time.perf_counter() - t) * 1e3)
                rounds[n].append(float(np.median(ts)))
        base = float(np.median(rounds[legs[0][0]]))
        for n, _ in legs:
            med = float(np.median(rounds[n]))
            say("%s %-34s wall ms first %.1f, rounds %s (median %.2f, %.2f x the first leg)" % (title, n, first[n], " ".join("%.2f" % v for v in rounds[n]), med, med / base))

    t = time.time()
    P, N = 8, 2048
    need = (P + 1) * 75 * N + N
    x0, _ = pss_train(N, P + 2, 0.0, 20.0)
    rng = np.random.default_rng(9)
    x1 = (1j * x0 + 0.1 * (rng.standard_normal(len(x0)) + 1j * rng.standard_normal(len(x0)))).astype(np.complex64)
    x = np.ascontiguousarray(np.stack([x0.astype(np.complex64), x1])[:, :need])
    say("search head: 2 x %d samples at 30.72 MS/s (%.1f MB cf32 per antenna), 8 periods, built in %.1f s" % (need, need * 8 / 1e6, time.time() - t))
    t = time.time()
    rate = 61.44e6
    y0, _ = pss_train(128, 4, 0.0, 20.0)
    y = fft_convert(y0, 32, 1)
    y = y * carrier(len(y), 9.9e6, rate)
    w = 0.1 * (rng.standard_normal((len(y), 2)) + 1j * rng.standard_normal((len(y), 2)))
    w[:, 0] += y
    w[:, 1] -= y
    y2 = w.astype(np.complex64)
    say("scan head: %d samples x 2 antennas at 61.44 MS/s (%.1f MB cf32), carrier +9900.0 kHz, built in %.1f s" % (len(y2), y2.nbytes / 1e6, time.time() - t))
    if a.build_only:
        return

    res = {}

    def leg(name, f):
        def run():
            res[name] = f()
        return name, run

    measure("search", [leg("cell_search (antenna 0)", lambda: la.cell_search(x[0], 100, nof_periods=P)),
                       leg("cell_search_ant A = 1", lambda: la.cell_search_ant(x[:1], 100, nof_periods=P)),
                       leg("cell_search_ant A = 2", lambda: la.cell_search_ant(x, 100, nof_periods=P))])
    say("search answers: %s" % [(n, r[0], r[1].cell_id, r[1].pss_pos, round(r[1].pss_p2avg, 1)) for n, r in res.items()])
    res.clear()
    plan = la.carrier_scan_plan(rate)
    measure("scan  ", [leg("antenna = 0", lambda: la.carrier_scan(y2, rate, antenna=0)), leg('antenna = "all"', lambda: la.carrier_scan(y2, rate, antenna="all"))])
    say("scan: %d hypotheses, %d taps, head %d samples; carriers %s" %
        (plan["nof_hypotheses"], plan["taps"], plan["nof_input_samples"], [(n, [(c.center_offset_hz, c.search.n_id_2, round(c.scan_p2avg, 1)) for c in r]) for n, r in res.items()]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
