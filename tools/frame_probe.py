#!/usr/bin/env python3
"""tools/frame_probe.py - what frame sync costs a re-acquiring stream that loses nothing, and what one check takes (a measurement, no pass / fail).

tools/reacq_probe.py's recording and method: a cut of the cfg3 capture of bench.py on both carriers (+9.9 and -9.9 MHz) of a two-cell 61.44 MS/s recording
(N = 2048, two antennas), cf32, read into ONE pinned host buffer and pushed through a tracked, re-acquiring Stream in pieces of 1 ms, each leg from cold Phys,
timed from the first push to the end of the flush.  Per round the SAME stream runs with frame sync off and on, interleaved; nothing is lost, so no check may
start, the block digests must be equal and the rates are compared with each other in this run.  One more leg pushes the recording with --cut samples removed in
the middle - more than 2.5 ms, so that the jump lands on another half frame - and prints what the check found and how far behind the jump the relabel came.

The launch times of one attempt come from a run of its own: with --kernel-trace the probe starts a child (this script with --leg: the leg with the cut) under
rocprofv3 --kernel-trace --stats and reads the PBCH kernels' rows, and from the kernel trace, for every k_pbch_viterbi, the time from the start of the k_ofdm in
front of it (the attempt's own, one subframe) to its end.

  python tools/frame_probe.py [--subframes 800] [--rounds 3] [--block 100] [--stream-block 100] [--piece 61440] [--cut 430081] [--kernel-trace] [--out profiles/frame_sync.txt]"""
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
    """the leg with the cut alone under rocprofv3 (the program goes behind --) -> the PBCH kernels' rows of the kernel statistics, and the attempts of the trace"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        say("kernel trace: rocprofv3 not found - the launch times of an attempt NOT measured")
        return
    td = tempfile.mkdtemp(prefix="frame_probe_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", td, "-o", "frame", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--leg",
               "--subframes", str(a.subframes), "--block", str(a.block), "--stream-block", str(a.stream_block), "--piece", str(a.piece), "--cut", str(a.cut)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        rows = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            with open(p, newline="") as fh:
                rows += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in ("k_pbch", "k_pss_timing", "k_pss_acquire"))]
        if r.returncode or not any("k_pbch_viterbi" in row.get("Name", "") for row in rows):
            say("kernel trace: no k_pbch_viterbi row (exit %d) - NOT measured; last output: %s" % (r.returncode, r.stdout[-300:].replace("\n", " | ")))
            return
        for row in rows:
            say("kernel trace  %-60s calls %s, total %s ns, average %s ns, min %s, max %s" % (row.get("Name", "")[:60], row.get("Calls"), row.get("TotalDurationNs"),
                                                                                          row.get("AverageNs"), row.get("MinNs"), row.get("MaxNs")))
        launches = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            with open(p, newline="") as fh:
                for row in csv.DictReader(fh):
                    try:
                        launches.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
                    except (KeyError, ValueError):
                        launches = None
                        break
            if launches is None:
                break
        if not launches:
            say("kernel trace: no per-launch rows with Kernel_Name / Start_Timestamp / End_Timestamp - one attempt NOT measured on its own")
            return
        launches.sort()
        for i, (t0, t1, name) in enumerate(launches):
            if "k_pbch_viterbi" not in name:
                continue
            prev = [l for l in launches[:i] if "k_ofdm" in l[2]]
            if not prev:
                continue
            mine = [l for l in launches[:i + 1] if l[0] >= prev[-1][0] and any(k in l[2] for k in ("k_ofdm", "k_chest", "k_pbch"))]
            say("kernel trace  one attempt: %s; first start to last end %.1f us" % (", ".join("%s %.1f us" % (n.split("(")[0].split()[-1], (e - s) / 1e3) for s, e, n in mine),
                                                                                   (t1 - prev[-1][0]) / 1e3))
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every stream (two Phys hold their block buffers at once)")
    ap.add_argument("--stream-block", type=int, default=100, help="block_subframes of the streams")
    ap.add_argument("--piece", type=int, default=61440, help="samples per push (61 440 = 1 ms)")
    ap.add_argument("--cut", type=int, default=430081, help="samples removed in the middle of the recording for the leg with a loss (430 081: 7 ms and a sample)")
    ap.add_argument("--kernel-trace", action="store_true", help="afterwards, the leg with the cut in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--leg", action="store_true", help="the leg with the cut and nothing else (what --kernel-trace runs)")
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

    def pin(x):
        pinned = torch.from_numpy(x.view(np.float32).reshape(len(x), -1)).pin_memory()   # what a radio driver's buffers are
        return pinned, pinned.numpy().view(x.dtype).reshape(x.shape)
    at = LEAD + (len(raw) // 2) // a.piece * a.piece + 12345
    keep_cut, host_cut = pin(np.concatenate([raw[:at], raw[at + a.cut:]]))
    keep, host = pin(raw)
    del raw
    say("frame_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, cf32, LSN_FILE_BLOCK %d, blocks of %d subframes, "
        "%d pushes of %d samples from a pinned buffer, library %s; built in %.0f s" % (rate_in / 1e6, nsf, a.block, a.stream_block, -(-len(host) // a.piece), a.piece,
                                                                                       os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))

    def leg(buf, frame_sync):
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
        st = la.Stream(rate_in, cells, block_subframes=a.stream_block, track=dict(), reacquire=dict(after=4), frame_sync=dict() if frame_sync else None)
        t0 = time.perf_counter()
        for pos in range(0, len(buf), a.piece):
            st.push(buf[pos:pos + a.piece])
        done = st.flush()
        dt = time.perf_counter() - t0
        ts, rs = st.track_status(), st.reacquire_status()
        fs = st.frame_sync_status() if frame_sync else None
        st.close()
        digests = []
        for phy, w in ps:
            digests.append(list(w.block_digests()))
            phy.close()
        return done, dt, digests, ts, rs, fs

    def cut_leg():
        done, dt, _, ts, rs, fs = leg(host_cut, True)
        behind = [r - j if r else None for r, j in zip(fs["relabel_segment"], rs["jump_segment"])]
        return ("%d samples removed at sample %d (subframe %.1f): %s subframes, %.1f ms; searches accepted %r, offset %r output samples, jump in force at segment %r; "
                "checks %r, attempts %r, confirmed %r, relabelled %r, given up %r, accepted at segment %r, sfn %r, delta %r, relabel in force at segment %r - %r segments "
                "(5 ms of the stream each) behind the jump -, %r subframes held" %
                (a.cut, at, (at - LEAD) / 61440.0, "+".join(str(n) for n in done), dt * 1e3, rs["accepted"], rs["last_offset"], rs["jump_segment"], fs["checks"], fs["attempts"],
                 fs["confirmed"], fs["relabelled"], fs["given_up"], fs["accept_segment"], fs["last_sfn"], fs["last_delta"], fs["relabel_segment"], behind, fs["held"]))

    if a.leg:
        print("leg: " + cut_leg())
        return
    rates = {}
    for rnd in range(a.rounds):
        yard = None
        for frame_sync in (False, True):
            done, dt, digests, ts, rs, fs = leg(host, frame_sync)
            if not frame_sync:
                yard = (done, digests, ts, rs)
            name = "frame sync on" if frame_sync else "frame sync off"
            rates.setdefault(name, []).append(sum(done) / dt)
            say("round %d  %-14s %s subframes, %.0f cell-sf/s, %.1f ms%s" % (rnd + 1, name, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3,
                                                                          "" if not frame_sync else " (counts, digests, track and reacquire status %s the leg's without; checks %r, attempts %r)" % (
                                                                              "equal" if (done, digests, ts, rs) == yard else "DIFFER from", fs["checks"], fs["attempts"])))
    for name, v in rates.items():
        say("median of %d  %-14s %.0f cell-sf/s (%.3f of frame sync off; %.0f .. %.0f)" % (len(v), name, statistics.median(v),
                                                                                       statistics.median(v) / statistics.median(rates["frame sync off"]), min(v), max(v)))
    say("with a loss  " + cut_leg())
    if a.kernel_trace:
        kernel_trace(a, say)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
