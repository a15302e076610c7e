#!/usr/bin/env python3
"""tools/wide_resample_probe.py - the resampler's wide-ratio run: the kernel alone, and what a narrow cell costs a replay (a measurement, no pass / fail).

  python tools/wide_resample_probe.py --kernels [--rounds 6] [--out FILE]
      kernel durations from a `rocprofv3 --kernel-trace` run of its own (the workload is this script's --child, a fresh process).  40 ms of a 122.88 MS/s cf32
      recording, one antenna, input and output resident on the device.  Per round, in this order: k_resample_wide to 3.84 MS/s (15 PRB, ratio 32, 32 lanes per
      output - the widest ratio the resampler accepts), k_resample_wide to 7.68 MS/s (25 PRB, ratio 16), k_chan_bank to 1.92 MS/s on the same samples (the carrier
      scan's channel, ratio 64: the parent commit's code for the same arithmetic and the yardstick; the resampler itself refuses a 1.92 MS/s output above ratio 4,
      so the two do not run the same pair), and k_resample to 30.72 MS/s (ratio 4, one lane per output).  The first round is a warm-up and is left out.  Printed
      per leg: median and range, input samples per second, and tap products (outputs x taps) per second - the figure that compares legs of different pairs.
  python tools/wide_resample_probe.py --replay [--subframes 100] [--rounds 3] [--out FILE]
      one pass of process_file_cells and one pushed stream over a 61.44 MS/s cf32 recording of a 100-PRB cell at -9.9 MHz and a 25-PRB cell at +17 MHz (ratio 8),
      in cell-subframes per second; beside it the same 100-PRB cell alone, from the same file.  Each leg from cold Phys with the block buffers reserved, timed
      around the replay call / the pushes and the flush."""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
RATE_IN, HEAD_S = 122.88e6, 0.040
# (label, kernel name, rate_out, nof_prb or None for the scan's channel)
LEGS = [("k_resample_wide -> 3.84 MS/s", "k_resample_wide", 3.84e6, 15), ("k_resample_wide -> 7.68 MS/s", "k_resample_wide", 7.68e6, 25),
        ("k_chan_bank     -> 1.92 MS/s", "k_chan_bank", 1.92e6, None), ("k_resample      -> 30.72 MS/s", "k_resample<", 30.72e6, 100)]


def _legs():
    """-> [(label, kernel, cfg, n_out, taps)] for the input of HEAD_S seconds"""
    import ltesniffer_amd as la
    n_in = int(RATE_IN * HEAD_S)
    out = []
    for label, kernel, rate_out, prb in LEGS:
        sp = la.ResampleSpan()
        if prb is None:
            cfg = la._channel_cfg(1, RATE_IN, 0.0, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
            assert la.lib().lsn_carrier_channel_span(C.byref(cfg), 0, n_in, C.byref(sp)) == 0
        else:
            cfg = la._resample_cfg(1, RATE_IN, rate_out, 0, 0.0, 0, 0, 15000.0 * (6 * prb + 1), la.FILE_CF32, 0.0)
            assert la.lib().lsn_resample_span(C.byref(cfg), 0, n_in, C.byref(sp)) == 0
        out.append((label, kernel, cfg, int(sp.max_out), int(sp.taps)))
    return n_in, out


def child(rounds):
    import torch
    import ltesniffer_amd as la
    L = la.lib()
    n_in, legs = _legs()
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn((n_in, 1, 2), generator=g, dtype=torch.float32).to("cuda:0")
    outs = [torch.zeros((1, n_out, 2), dtype=torch.float32, device="cuda:0") for _, _, _, n_out, _ in legs]
    for _ in range(rounds + 1):
        for (label, kernel, cfg, n_out, _), out in zip(legs, outs):
            call = L.lsn_carrier_channel if kernel == "k_chan_bank" else L.lsn_resample
            rc = call(0, C.c_void_p(x.data_ptr()), 1, n_in, C.byref(cfg), C.c_void_p(out.data_ptr()), 1, n_out)
            assert rc == 0, (label, rc)
        torch.cuda.synchronize()


def _col(row, *want):
    for k in row:
        if all(w in k.lower() for w in want):
            return k
    raise KeyError(want)


def kernels(rounds, say):
    import ltesniffer_amd as la
    from tree_hash import tree_hash
    td = tempfile.mkdtemp(prefix="wide_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(rounds)]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = []
    for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            name = r[_col(r, "kernel_name")]
            if re.search(r"k_resample|k_chan_bank", name):
                rows.append((int(r[_col(r, "start_timestamp")]), int(r[_col(r, "end_timestamp")]), name))
    shutil.rmtree(td, ignore_errors=True)
    rows.sort()
    n_in, legs = _legs()
    assert len(rows) == (rounds + 1) * len(legs), (len(rows), rounds, [r[2] for r in rows[:8]])
    say("wide_resample_probe --kernels: tree %s, library %s; %.0f ms of a %.2f MS/s cf32 recording (%d samples), one antenna, %d timed rounds interleaved, warm-up left out" %
        (tree_hash(), os.path.relpath(la.LIB_PATH, ROOT), HEAD_S * 1e3, RATE_IN / 1e6, n_in, rounds))
    for i, (label, kernel, _, n_out, taps) in enumerate(legs):
        mine = rows[i::len(legs)][1:]
        assert all(kernel in r[2] for r in mine), (kernel, mine[0][2])
        d = sorted(e - s for s, e, _ in mine)
        med = d[len(d) // 2]
        say("  %-30s %4d taps, %7d outputs: %8.1f us median (%.1f - %.1f, n = %d)  %7.2f G input samples/s  %7.2f G tap products/s" %
            (label, taps, n_out, med / 1e3, d[0] / 1e3, d[-1] / 1e3, len(d), n_in / med, n_out * taps / med))


def replay(nsf, rounds, say):
    import numpy as np
    import ltesniffer_amd as la
    from ddc_cases import carrier
    from lsn_testlib import scenario
    from parity import gen_subframes
    from resample_cases import LEAD, TAIL, fft_convert
    from srs_streams import STREAMS
    from tree_hash import tree_hash
    rate = 61.44e6
    t = time.time()
    cells, total = [], None
    for name, f0, channel_hz, (num, den) in (("prb100_tm34_256qam", -9.9e6, 19.8e6, (2, 1)), ("prb25_2port", 17e6, 5e6, (8, 1))):
        preset, _, over, opt = STREAMS[name]
        sc = scenario(preset, **over)
        tti0, iq, _ = gen_subframes(sc, nsf)
        x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])
        y = fft_convert(x, num, den)
        Y = np.fft.fft(y, axis=0)
        Y[np.abs(np.fft.fftfreq(len(y), 1.0 / rate)) > 0.5 * channel_hz] = 0.0
        y = np.fft.ifft(Y, axis=0)
        y = np.concatenate([y[len(y) - LEAD:], y, y[:TAIL]])
        y = y * carrier(len(y), f0, rate)[:, None]
        total = y if total is None else total + y
        cells.append((sc, opt, dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, max_subframes=nsf)))
    raw = total.astype(np.complex64)
    del total
    td = tempfile.mkdtemp(prefix="wide_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(td, "two.cf32")
    raw.tofile(path)
    say("wide_resample_probe --replay: tree %s, library %s; 61.44 MS/s cf32, 2 antennas, a 100-PRB cell at -9.9 MHz and a 25-PRB cell at +17 MHz, %d subframes per cell, "
        "%d bytes; built in %.0f s" % (tree_hash(), os.path.relpath(la.LIB_PATH, ROOT), nsf, os.path.getsize(path), time.time() - t))
    phich = {1: 0, 3: 1, 6: 2, 12: 3}

    def phys(jobs):
        out = []
        for sc, opt, _ in jobs:
            phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=100, pcapwriter=la.PcapWriter(None), **opt)
            assert phy.set_sampling(la.RATES_3GPP) and phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], phich[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
            phy.prepare_file()
            out.append(phy)
        return out

    def leg(jobs, way):
        from parity import gpu_records
        ps = phys(jobs)
        try:
            t0 = time.perf_counter()
            if way == "file":
                done = la.process_file_cells(path, rate, [(p, kw) for p, (_, _, kw) in zip(ps, jobs)])
            else:
                with la.Stream(rate, [(p, kw) for p, (_, _, kw) in zip(ps, jobs)], block_subframes=25) as st:
                    for pos in range(0, len(raw), 614400):
                        st.push(raw[pos:pos + 614400])
                    done = st.flush()
            dt = time.perf_counter() - t0
            return done, dt, [len(gpu_records(p)) for p in ps]
        finally:
            for p in ps:
                p.close()

    try:
        for rnd in range(rounds):
            for label, jobs in (("100 + 25 PRB", cells), ("100 PRB alone", cells[:1])):
                for way in ("file", "stream"):
                    done, dt, nrec = leg(jobs, way)
                    say("round %d  %-14s %-7s %s subframes, %6.0f cell-sf/s, %7.1f ms, records %s" % (rnd + 1, label, way, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3, nrec))
    finally:
        os.remove(path)
        os.rmdir(td)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--replay", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--subframes", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.rounds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.kernels:
        kernels(a.rounds or 6, say)
    if a.replay:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call
        replay(a.subframes, a.rounds or 3, say)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
