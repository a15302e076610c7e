#!/usr/bin/env python3
"""tools/clock_probe.py - the sample-clock estimate on an MI355X: wall time on a long recording, and the table of profiles/clock_estimate.txt
(a measurement, no pass / fail; there is no parent figure to compare with).

  wall time   a 1 s, 100-PRB (30.72 MS/s), one-antenna cf32 recording - a PSS train at +7 ppm, 20 dB, synthesised in continuous time (tests/clock_cases.pss_train
              without the neighbour symbols) - is written to a file; lsn_file_clock_estimate (all rounds: 8 -> 32 -> 128 -> 200 periods, only the slices read) is
              timed --rounds times, and lsn_clock_estimate on the same samples in host memory next to it.
  --table     every input of tests/test_clock_model.py / tests/test_gpu_clock.py that needs no oracle: the error at the end of the recording, in samples, of the
              model (tests/clock_model.py) and of the GPU path.

  python tools/clock_probe.py [--rounds 5] [--seconds 1.0] [--table] [--out FILE]"""
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
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import ltesniffer_amd as la
    import clock_model as M
    from clock_cases import TRAINS, end_error, pss_train, train
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.table:
        say("%-30s %10s %10s %14s %14s" % ("input", "eps ppm", "samples", "model error", "GPU error"))
        for name in sorted(TRAINS):
            x, info = train(name)
            res, _ = M.estimate(x, info["N"], info["n_id_2"], info["pss_pos"], info["cfo_hz"])
            s = la.CellSearch(n_id_2=info["n_id_2"], pss_pos=info["pss_pos"], sf_start=0, cfo_hz=info["cfo_hz"])
            est = la.clock_estimate(x, 6, s)
            say("%-30s %+10.1f %10d %14.4f %14.4f   (rounds %d, used %d / %d, rms residual %.3f, max %.3f)" %
                (name, info["eps"] * 1e6, len(x), end_error(res["eps"], info["eps"], len(x)), end_error(est.eps, info["eps"], len(x)), est.nof_rounds, est.nof_used,
                 est.nof_periods, est.rms_residual, est.max_residual))
    periods = int(round(a.seconds * 200))
    eps = 7e-6
    t = time.time()
    x, info = pss_train(2048, periods, eps, 20.0, loaded=False)
    say("recording: %d periods, %d samples (%.0f MB cf32), built in %.1f s" % (periods, len(x), x.nbytes / 1e6, time.time() - t))
    td = tempfile.mkdtemp(prefix="clock_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(td, "train.cf32")
    try:
        x.tofile(path)
        s = la.CellSearch(n_id_2=info["n_id_2"], pss_pos=info["pss_pos"], sf_start=0, cfo_hz=0.0)
        for leg in ("file", "memory"):
            ts = []
            for _ in range(a.rounds + 1):   # the first pass pays for the runtime's start and is left out
                t = time.perf_counter()
                est = la.file_clock_estimate(path, 100, s) if leg == "file" else la.clock_estimate(x, 100, s)
                ts.append((time.perf_counter() - t) * 1e3)
            say("%-6s lsn_%sclock_estimate: found %d, %d rounds, %d / %d used, error %.4f sample at the end; wall ms first %.1f, then %s (median %.1f)" %
                (leg, "file_" if leg == "file" else "", est.found, est.nof_rounds, est.nof_used, est.nof_periods, end_error(est.eps, eps, len(x)), ts[0],
                 " ".join("%.1f" % v for v in ts[1:]), float(np.median(ts[1:]))))
    finally:
        if os.path.exists(path):
            os.unlink(path)
        os.rmdir(td)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
