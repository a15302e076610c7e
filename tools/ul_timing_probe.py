#!/usr/bin/env python3
"""tools/ul_timing_probe.py - what the per-grant uplink arrival-time measurement costs in UL_MODE (a measurement, no pass / fail).

The UL_MODE leg of tools/bench_legs.py (cfg4_ul_mode_64_rnti: bench.py's capture, host buffers, the cold pass untimed, the following passes timed) with
lsn_phy_set_ul_timing mode 0, 1 and 2, interleaved in one run, each leg on a fresh Phy.  All three are gated on the leg's cached oracle stream: the stream has
no offsets, so the records must not change.  Then the same with every UE early by N / 8 (the uplink antenna's stream moved N / 8 samples ahead; the downlink
antenna untouched): no oracle stream exists for it, the uplink records of each mode are counted.  The comparison is mode 0 IN THE SAME RUN.

The two new kernels' own times come from a run of their own: with --kernel-trace the probe starts a child (this script with --leg) under rocprofv3
--kernel-trace --stats and reads k_pusch_toa's and k_ul_fft_win's rows out of the statistics it writes.

  python tools/ul_timing_probe.py [--rounds 2] [--passes 3] [--kernel-trace] [--out profiles/ul_timing.txt]"""
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

LEG = "cfg4_ul_mode_64_rnti"
KERNELS = ("k_pusch_toa", "k_ul_fft_win", "k_ul_fft", "k_pusch_chest", "k_pusch_demod")


def kernel_trace(a, say):
    """the early stream in mode 2 alone under rocprofv3 (the program goes behind --) -> the uplink kernels' rows of its kernel statistics"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        say("kernel trace: rocprofv3 not found - the kernels' times NOT measured")
        return
    td = tempfile.mkdtemp(prefix="ul_timing_probe_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", td, "-o", "ul_timing", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--leg", "--passes", "2"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        rows = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            with open(p, newline="") as fh:
                rows += [row for row in csv.DictReader(fh) if any(k + "(" in row.get("Name", "") or row.get("Name", "").startswith(k) for k in KERNELS)]
        if r.returncode or not rows:
            say("kernel trace: no row of the uplink kernels (exit %d) - NOT measured; last output: %s" % (r.returncode, r.stdout[-300:].replace("\n", " | ")))
            return
        say("kernel trace (mode 2, every UE early by N / 8, two passes of the leg):")
        for row in rows:
            say("kernel trace  %-40s calls %s, total %s ns, average %s ns, min %s, max %s" % (row.get("Name", "")[:40], row.get("Calls"), row.get("TotalDurationNs"),
                                                                                          row.get("AverageNs"), row.get("MinNs"), row.get("MaxNs")))
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=None, help="passes over the capture, the first untimed (default: the leg's)")
    ap.add_argument("--kernel-trace", action="store_true", help="afterwards, the early stream in mode 2 in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--leg", action="store_true", help="the early stream in mode 2 and nothing else (what --kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench_legs as bl
    import ltesniffer_amd as la
    ld = bl.LEGS[LEG]
    npass = a.passes or ld["passes"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    sc, tti0, iq = bl.leg_capture(LEG)
    golden, gnote = bl.load_golden(LEG, iq, tti0)
    nsf = iq.shape[0]
    N = iq.shape[2] // 15
    adv = N // 8
    early = iq.copy()
    ul = iq[:, 1].reshape(-1)
    early[:, 1] = np.concatenate([ul[adv:], np.zeros(adv, dtype=ul.dtype)]).reshape(nsf, -1)
    streams = {"as sent": torch.from_numpy(iq).pin_memory(), "early N/8": torch.from_numpy(early).pin_memory()}
    del iq, early
    if not a.leg:
        say("ul_timing_probe: %s, %d subframes x %d passes (the first untimed), N = %d, host buffers (two antenna streams), library %s; built in %.0f s%s" % (
            LEG, nsf, npass, N, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t, "" if golden is not None else "; NO oracle gate: " + str(gnote)))

    def leg(stream, mode):
        w = la.PcapWriter(None)
        w.set_store(False)
        w.set_digest_blocks(bl.BLOCK, tti0)
        phy = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=200, pcapwriter=w)
        assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"]) and phy.setUlConfig(ld["cyclic_shift"], ld["delta_ss"])
        assert phy.setUlTiming(mode) == la.LSN_SUCCESS
        h = streams[stream].numpy()
        phy.process_host(h, tti0 % 10240, bl.META_PERIOD)
        t0 = time.perf_counter()
        for r in range(1, npass):
            phy.process_host(h, (tti0 + r * nsf) % 10240, bl.META_PERIOD)
        dt = time.perf_counter() - t0
        pf = phy.perf()
        nb = npass * nsf // bl.BLOCK
        blocks = w.block_digests()[:nb]
        blocks += [(0x9E3779B97F4A7C15, 0)] * (nb - len(blocks))
        nrec = w.nof_records()
        phy.close()
        return (npass - 1) * nsf / dt, blocks, nrec, pf.nof_tb_decodes, pf.nof_pdus

    if a.leg:
        rate, _, nrec, ntb, npdu = leg("early N/8", 2)
        print("leg: %.0f sf/s, %d records" % (rate, nrec))
        return
    rates = {}
    for rnd in range(a.rounds):
        for stream in streams:
            yard = None
            for mode in (0, 1, 2):
                rate, blocks, nrec, ntb, npdu = leg(stream, mode)
                yard = blocks if mode == 0 else yard
                rates.setdefault((stream, mode), []).append(rate)
                if stream == "as sent":
                    cov, bad, rd = bl.check_blocks(golden, blocks, 0)
                    gate = "oracle blocks compared %d, mismatching %s" % (cov, bad)
                else:
                    gate = "no oracle stream; blocks equal to mode 0's: %s" % ("yes" if blocks == yard else "no")
                say("round %d  %-9s mode %d  %8.0f sf/s, records (all passes) %d, PDUs of the last pass %d, transport-block decodes of the last pass %d; %s" % (
                    rnd + 1, stream, mode, rate, nrec, npdu, ntb, gate))
    for (stream, mode), v in rates.items():
        base = statistics.median(rates[(stream, 0)])
        say("median of %d  %-9s mode %d  %8.0f sf/s (%.3f of mode 0 on the same stream; %.0f .. %.0f)" % (len(v), stream, mode, statistics.median(v), statistics.median(v) / base, min(v), max(v)))
    if a.kernel_trace:
        kernel_trace(a, say)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
