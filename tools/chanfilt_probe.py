#!/usr/bin/env python3
"""tools/chanfilt_probe.py - the channel filter in front of the resampler on the two-carrier recording of tools/cells_probe.py: what it costs and
whether the oracle's block digests hold with it (a measurement, no pass / fail).

The recording is cells_probe's: a cut of the cfg3 capture of bench.py on BOTH carriers (+-9.9 MHz) of a 61.44 MS/s file, cf32 and sc16, so both replays are
gated on the oracle's block digests of tests/golden/cfg3_stream_oracle.json.  Legs, interleaved round by round, each from cold Phys with the block buffers
reserved (lsn_phy_prepare_file), timed around the replay call(s) only:
  filter off / on  x  sequential (two process_file_rate calls) / one pass (one process_file_cells call)
Printed with every figure: cell-subframes per second and the number of digest blocks that differ from the oracle's.  Then, from a kernel trace run of its own
(a fresh child process under `rocprofv3 --kernel-trace` that replays the filtered one pass once per format): the time of k_chan_fir and of stage 2 per block.

  python tools/chanfilt_probe.py [--subframes 800] [--rounds 3] [--block 100] [--formats cf32,sc16] [--no-trace] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call
OFFSETS = (9.9e6, -9.9e6)


def _phys(la, sc, BLOCK, tti0, stop):
    out = []
    for _ in OFFSETS:
        w = la.PcapWriter(None)
        w.set_store(False)
        w.set_digest_blocks(BLOCK, tti0)
        phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=400, pcapwriter=w)
        assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
        assert phy.set_channel_filter(stop)
        phy.prepare_file()
        out.append((phy, w))
    return out


def _leg(la, sc, BLOCK, META, tti0, golden, path, kw, rate_in, stop, way):
    from resample_cases import LEAD
    ps = _phys(la, sc, BLOCK, tti0, stop)
    cell = [dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, update_meta_period=META) for f0 in OFFSETS]
    t0 = time.perf_counter()
    if way == "sequential":
        done = [ps[i][0].process_file_rate(path, rate_in, **dict(cell[i], **kw)) for i in (0, 1)]
    else:
        done = la.process_file_cells(path, rate_in, [(ps[i][0], cell[i]) for i in (0, 1)], **kw)
    dt = time.perf_counter() - t0
    bad = total = 0
    for phy, w in ps:
        blocks = w.block_digests()
        bad += sum(1 for j, (d, c) in enumerate(blocks) if ["%016x" % d, c] != list(golden[j]))
        total += len(blocks)
        phy.close()
    return done, dt, bad, total


def child(a):
    """one filtered one-pass replay per file, for the kernel trace"""
    import ltesniffer_amd as la
    from make_cfg3_golden import cfg3_stream
    sc, NSF, BLOCK, META = cfg3_stream()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")))["blocks"]
    for spec in a.child:
        path, fmt, scale = spec.split(",")
        _leg(la, sc, BLOCK, META, a.tti0, golden, path, dict(sample_format=int(fmt), sample_scale=float(scale)), 61.44e6, a.stop, "one pass")


def _col(row, *want):
    for k in row:
        if all(w in k.lower() for w in want):
            return k
    raise KeyError(want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every replay (two Phys hold their block buffers at once)")
    ap.add_argument("--formats", default="cf32,sc16")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="*", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tti0", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--stop", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.environ["LSN_FILE_BLOCK"] = str(a.block)
    if a.child is not None:
        return child(a)
    import numpy as np
    import ltesniffer_amd as la
    from ddc_cases import SPACING, wideband
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")))["blocks"]
    stop = la.cells_stopbands(list(OFFSETS), [sc["nof_prb"]] * 2, 61.44e6)[0]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    rate_in, f = wideband([(iq, f0, 1.0) for f0 in OFFSETS], 2, 1, 30.72e6, channel_hz=SPACING)
    del iq
    td = tempfile.mkdtemp(prefix="chanfilt_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    files = {}
    for fmt in a.formats.split(","):
        p = os.path.join(td, "two." + fmt)
        if fmt == "cf32":
            f.astype(np.complex64).tofile(p)
            files[fmt] = (p, dict(sample_format=la.FILE_CF32, sample_scale=0.0))
        else:
            peak = max(float(np.abs(f.real).max()), float(np.abs(f.imag).max()))
            scale = 2.0 ** np.ceil(np.log2(peak / 16384.0))
            np.round(np.stack([f.real, f.imag], axis=-1) / scale).astype(np.int16).tofile(p)
            files[fmt] = (p, dict(sample_format=la.FILE_SC16, sample_scale=float(scale)))
    del f
    d = la.channel_filter_design(rate_in, 15000.0 * (6 * sc["nof_prb"] + 1), stop)
    say("chanfilt_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, LSN_FILE_BLOCK %d, stopband %.3f MHz (L = %d, %d taps), library %s; built in %.0f s" %
        (rate_in / 1e6, nsf, a.block, stop / 1e6, d["L"], 2 * d["L"] + 1, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
    for k, (p, _) in files.items():
        with open(p, "rb", buffering=0) as fh:   # read once: the first read of freshly written page-cache pages is slow whoever reads them
            buf = bytearray(64 << 20)
            while fh.readinto(buf):
                pass
    try:
        for rnd in range(a.rounds):
            for fmt, (p, kw) in files.items():
                for way in ("sequential", "one pass"):
                    for label, s in (("filter off", 0.0), ("filter on", stop)):
                        done, dt, bad, total = _leg(la, sc, BLOCK, META, tti0, golden, p, kw, rate_in, s, way)
                        say("round %d  %-5s %-10s %-10s %s subframes, %.0f cell-sf/s, %.1f ms (%d of %d blocks differ from the oracle's)" %
                            (rnd + 1, fmt, way, label, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3, bad, total))
        if not a.no_trace:
            pd = tempfile.mkdtemp(prefix="chanfilt_prof_")
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", pd, "--", sys.executable, os.path.abspath(__file__), "--block", str(a.block),
                   "--tti0", str(tti0), "--stop", repr(stop), "--child"] + ["%s,%d,%r" % (p, kw["sample_format"], kw["sample_scale"]) for p, kw in files.values()]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            durs = {}
            for p in glob.glob(os.path.join(pd, "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(p)):
                    name = r[_col(r, "kernel_name")]
                    for k in ("k_chan_fir_cells<0>", "k_chan_fir_cells<1>", "k_chan_fir<", "k_resample<0, false>", "k_resample<"):
                        if k in name.replace("(int)", "").replace("(bool)", ""):
                            durs.setdefault(k, []).append(int(r[_col(r, "end_timestamp")]) - int(r[_col(r, "start_timestamp")]))
                            break
            shutil.rmtree(pd, ignore_errors=True)
            say("kernel trace of one filtered one-pass replay per format (%d subframes per cell; short last blocks included):" % nsf)
            for k, v in sorted(durs.items()):
                v.sort()
                say("  %-22s %3d launches, %8.1f us in all, median %7.1f us (%.1f - %.1f)" % (k, len(v), sum(v) / 1e3, v[len(v) // 2] / 1e3, v[0] / 1e3, v[-1] / 1e3))
    finally:
        for p, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
