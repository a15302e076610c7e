#!/usr/bin/env python3
"""tools/scan_probe.py - the carrier scan on an MI355X: wall time of a scan of the head of a 61.44 MS/s recording at the 100 kHz raster (603 hypotheses) and at
a 10 kHz raster (6033), written to profiles/carrier_scan.txt (a measurement, no pass / fail; there is no parent figure to compare with).

  recording   one antenna, cf32, 61.44 MS/s: white noise with a PSS train (tests/clock_cases.pss_train at 1.92 MS/s, 20 dB, brought to 61.44 MS/s by
              resample_cases.fft_convert) moved to --carrier Hz.  The head of P = 2 periods the scan reads is 925 856 samples (7.4 MB).
  timed       lsn_file_carrier_scan (pread of the head, upload, batches of k_chan_bank -> k_pss_corr -> k_scan_peaks, decision, cell search on the accepted
              carriers) and lsn_carrier_scan on the same samples in host memory, --rounds times each; the first pass pays for the runtime's start and is
              shown apart.

  python tools/scan_probe.py [--rounds 5] [--carrier 9.9e6] [--out FILE]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--carrier", type=float, default=9.9e6)
    ap.add_argument("--out", default=None)
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

    rate = 61.44e6
    t = time.time()
    x, info = pss_train(128, 4, 0.0, 20.0)
    y = fft_convert(x, 32, 1)
    y = y * carrier(len(y), a.carrier, rate)
    rng = np.random.default_rng(5)
    y = (y + 0.1 * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y)))).astype(np.complex64)
    say("recording: %d samples at 61.44 MS/s (%.1f MB cf32), carrier %+.1f kHz, built in %.1f s" % (len(y), y.nbytes / 1e6, a.carrier / 1e3, time.time() - t))
    td = tempfile.mkdtemp(prefix="scan_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(td, "head.cf32")
    try:
        y.tofile(path)
        for raster in (100e3, 10e3):
            plan = la.carrier_scan_plan(rate, raster_hz=raster)
            for leg in ("file", "memory"):
                ts = []
                for _ in range(a.rounds + 1):
                    t = time.perf_counter()
                    found = la.file_carrier_scan(path, rate, raster_hz=raster) if leg == "file" else la.carrier_scan(y, rate, raster_hz=raster)
                    ts.append((time.perf_counter() - t) * 1e3)
                say("raster %5.0f kHz, %4d hypotheses, %3d taps, head %d samples, %-6s: carriers %s; wall ms first %.1f, then %s (median %.1f)" %
                    (raster / 1e3, plan["nof_hypotheses"], plan["taps"], plan["nof_input_samples"], leg,
                     [(c.center_offset_hz, c.search.n_id_2, round(c.scan_p2avg, 1)) for c in found], ts[0], " ".join("%.1f" % v for v in ts[1:]), float(np.median(ts[1:]))))
    finally:
        if os.path.exists(path):
            os.unlink(path)
        os.rmdir(td)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
