#!/usr/bin/env python3
"""tools/track_probe.py - what the timing loop of a stream costs (a measurement, no pass / fail).

tools/stream_probe.py's recording and method: a cut of the cfg3 capture of bench.py on both carriers (+9.9 and -9.9 MHz) of a two-cell 61.44 MS/s recording, cf32,
read into ONE pinned host buffer and pushed through a Stream in pieces of 1 ms, each leg from cold Phys with reserved block buffers, timed from the first push to
the end of the flush.  Per round the SAME stream runs with tracking off and with tracking on (every cell enabled), interleaved; the summary is the median of the
rounds, in cell-subframes per second.  The comparison is tracking off in the same run, which must stay within the run-to-run spread of profiles/stream.txt.  The
recording's clock is right, so the loop has nothing to correct: the block digests of the tracked legs are compared with the untracked ones and the loop's status
is printed.

k_pss_timing's own time comes from a run of its own: with --kernel-trace the probe starts a child (this script with --leg) under rocprofv3 --kernel-trace --stats
and reads the kernel's row out of the statistics it writes.

  python tools/track_probe.py [--subframes 800] [--rounds 3] [--block 100] [--stream-block 100] [--piece 61440] [--kernel-trace] [--out profiles/track.txt]"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def kernel_trace(a, say):
    """a tracked leg alone under rocprofv3 (the program goes behind --) -> the k_pss_timing row of its kernel statistics"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        say("kernel trace: rocprofv3 not found - k_pss_timing's time NOT measured")
        return
    td = tempfile.mkdtemp(prefix="track_probe_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", td, "-o", "track", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--leg",
               "--subframes", str(a.subframes), "--block", str(a.block), "--stream-block", str(a.stream_block), "--piece", str(a.piece)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        rows = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            with open(p, newline="") as fh:
                rows += [row for row in csv.DictReader(fh) if "k_pss_timing" in row.get("Name", "") or "k_resample_ring" in row.get("Name", "")]
        if r.returncode or not rows:
            say("kernel trace: no k_pss_timing row (exit %d) - NOT measured; last output: %s" % (r.returncode, r.stdout[-300:].replace("\n", " | ")))
            return
        for row in rows:
            say("kernel trace  %-60s calls %s, total %s ns, average %s ns, min %s, max %s" % (row.get("Name", "")[:60], row.get("Calls"), row.get("TotalDurationNs"),
                                                                                          row.get("AverageNs"), row.get("MinNs"), row.get("MaxNs")))
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every stream (two Phys hold their block buffers at once)")
    ap.add_argument("--stream-block", type=int, default=100, help="block_subframes of the streams")
    ap.add_argument("--piece", type=int, default=61440, help="samples per push (61 440 = 1 ms)")
    ap.add_argument("--kernel-trace", action="store_true", help="afterwards, one tracked leg in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--leg", action="store_true", help="one tracked leg and nothing else (what --kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["LSN_FILE_BLOCK"] = str(a.block)
    import numpy as np
    import torch
    import ltesniffer_amd as la
    from ddc_cases import SPACING, wideband
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    from resample_cases import LEAD
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    offsets = (9.9e6, -9.9e6)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    rate_in, f = wideband([(iq, f0, 1.0) for f0 in offsets], 2, 1, 30.72e6, channel_hz=SPACING)
    del iq
    raw = f.astype(np.complex64)
    del f
    pinned = torch.from_numpy(raw.view(np.float32).reshape(len(raw), -1)).pin_memory()   # what a radio driver's buffers are
    host = pinned.numpy().view(raw.dtype).reshape(raw.shape)
    del raw
    say("track_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, cf32, LSN_FILE_BLOCK %d, blocks of %d subframes, "
        "%d pushes of %d samples from a pinned buffer, library %s; built in %.0f s" % (rate_in / 1e6, nsf, a.block, a.stream_block, -(-len(host) // a.piece), a.piece,
                                                                                       os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))

    def leg(track):
        ps = []
        for _ in offsets:
            w = la.PcapWriter(None)
            w.set_store(False)
            w.set_digest_blocks(BLOCK, tti0)
            phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=400, pcapwriter=w)
            assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
            phy.prepare_file()
            ps.append((phy, w))
        cells = [(ps[i][0], dict(center_offset_hz=offsets[i], start_tti=tti0, offset_time=LEAD, update_meta_period=META)) for i in (0, 1)]
        st = la.Stream(rate_in, cells, block_subframes=a.stream_block, track=dict() if track else None)
        t0 = time.perf_counter()
        for pos in range(0, len(host), a.piece):
            st.push(host[pos:pos + a.piece])
        done = st.flush()
        dt = time.perf_counter() - t0
        ts = st.track_status() if track else None
        st.close()
        digests = []
        for phy, w in ps:
            digests.append(list(w.block_digests()))
            phy.close()
        return done, dt, digests, ts

    if a.leg:
        done, dt, _, ts = leg(True)
        print("leg: %s subframes, %.1f ms, %r" % (done, dt * 1e3, ts))
        return
    rates = {}
    for rnd in range(a.rounds):
        yard = None
        for track in (False, True):
            done, dt, digests, ts = leg(track)
            if not track:
                yard = (done, digests)
            name = "track on" if track else "track off"
            rates.setdefault(name, []).append(sum(done) / dt)
            say("round %d  %-9s %s subframes, %.0f cell-sf/s, %.1f ms%s" % (rnd + 1, name, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3,
                                                                         "" if not track else " (counts and digests %s the untracked leg's; valid %r invalid %r, correction %s ppm, drift %s samples)" % (
                                                                             "equal" if (done, digests) == yard else "DIFFER from", ts["valid"], ts["invalid"],
                                                                             ", ".join("%+.3f" % v for v in ts["correction_ppm"]), ", ".join("%+.3f" % v for v in ts["position_drift"]))))
    for name, v in rates.items():
        say("median of %d  %-9s %.0f cell-sf/s (%.3f of track off; %.0f .. %.0f)" % (len(v), name, statistics.median(v), statistics.median(v) / statistics.median(rates["track off"]),
                                                                                 min(v), max(v)))
    if a.kernel_trace:
        kernel_trace(a, say)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
