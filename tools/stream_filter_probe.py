#!/usr/bin/env python3
"""tools/stream_filter_probe.py - what the channel filter costs a live stream: two cells of one 61.44 MS/s recording pushed as a stream with the filter off and on
(L = 88), tracked and untracked, against the file pass with and without the filter, all in ONE run on one build (a measurement, no pass / fail).

Recording and method are tools/stream_probe.py's: a cut of the cfg3 capture of bench.py on both carriers (+9.9 and -9.9 MHz) of a two-cell 61.44 MS/s recording, as
a cf32 and as an sc16 file; every leg from cold Phys with the block buffers reserved; the stream legs push the same bytes from ONE pinned host buffer in pieces of
1 ms (61 440 samples) and are timed from the first push to the end of the flush; rounds are interleaved and the summary is the median and the range of the rounds.
Legs per format and round:
  file / file+filter                         one process_file_cells call, the filter off / on (stopband_hz of cells_stopbands: 10.785 MHz, L = 88)
  stream blk B [+filter] [+track]            block_subframes B of --stream-blocks, the filter off / on, lsn_stream_track off / on (defaults, clock right)
The filter-off legs are the path of a stream before the filter existed: they belong next to profiles/stream.txt.  Printed with every figure: cell-subframes per
second (2 x subframes / wall time) and whether counts and block digests equal those of the same round's file pass with the same filter setting (an untracked
stream's must; a tracked one resamples at the steps its loop decides and need not).

Then, from a kernel-trace run of its own (a fresh child process under `rocprofv3 --kernel-trace` that runs, per format, one filtered stream with the first
--stream-blocks entry and one filtered file pass): the time of k_chan_fir_ring against k_chan_fir_cells, and of stage 2.

  python tools/stream_filter_probe.py [--subframes 800] [--rounds 3] [--block 100] [--stream-blocks 100,10] [--piece 61440] [--formats cf32,sc16] [--no-trace] [--out FILE]"""
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


def child(a):
    """per file: one filtered stream and one filtered file pass, for the kernel trace"""
    import numpy as np
    import ltesniffer_amd as la
    from make_cfg3_golden import cfg3_stream
    from resample_cases import LEAD
    sc, _, _, META = cfg3_stream()
    for spec in a.child:
        path, fmt, scale = spec.split(",")
        kw = dict(sample_format=int(fmt), sample_scale=float(scale))
        host = np.fromfile(path, dtype=np.complex64 if int(fmt) == la.FILE_CF32 else np.int16).reshape((-1, 2) if int(fmt) == la.FILE_CF32 else (-1, 2, 2))
        for way in ("stream", "file"):
            phys = []
            for _ in OFFSETS:
                w = la.PcapWriter(None)
                w.set_store(False)
                phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=400, pcapwriter=w)
                assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"]) and phy.set_channel_filter(a.stop)
                phy.prepare_file()
                phys.append(phy)
            cells = [(phys[i], dict(center_offset_hz=OFFSETS[i], start_tti=a.tti0, offset_time=LEAD, update_meta_period=META)) for i in (0, 1)]
            if way == "file":
                la.process_file_cells(path, 61.44e6, cells, **kw)
            else:
                with la.Stream(61.44e6, cells, block_subframes=a.trace_block, **kw) as st:
                    for pos in range(0, len(host), a.piece):
                        st.push(host[pos:pos + a.piece])
                    st.flush()
            for phy in phys:
                phy.close()


def _col(row, *want):
    for k in row:
        if all(w in k.lower() for w in want):
            return k
    raise KeyError(want)


OFFSETS = (9.9e6, -9.9e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every replay and stream (two Phys hold their block buffers at once)")
    ap.add_argument("--stream-blocks", default="100,10", help="block_subframes of the stream rows")
    ap.add_argument("--piece", type=int, default=61440, help="samples per push (61 440 = 1 ms)")
    ap.add_argument("--formats", default="cf32,sc16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", nargs="*", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tti0", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--stop", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--trace-block", type=int, default=100, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.environ["LSN_FILE_BLOCK"] = str(a.block)
    if a.child is not None:
        return child(a)
    import numpy as np
    import torch
    import ltesniffer_amd as la
    from ddc_cases import SPACING, wideband
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    from resample_cases import LEAD
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    offsets = OFFSETS
    sblocks = [int(v) for v in a.stream_blocks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    rate_in, f = wideband([(iq, f0, 1.0) for f0 in offsets], 2, 1, 30.72e6, channel_hz=SPACING)
    del iq
    stops = la.cells_stopbands(list(offsets), [sc["nof_prb"]] * 2, rate_in)
    half = [la.channel_filter_design(rate_in, 15000.0 * (6 * sc["nof_prb"] + 1), s)["L"] for s in stops]
    td = tempfile.mkdtemp(prefix="stream_filter_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    files = {}
    for fmt in a.formats.split(","):
        p = os.path.join(td, "two." + fmt)
        if fmt == "cf32":
            raw = f.astype(np.complex64)
            kw = dict(sample_format=la.FILE_CF32, sample_scale=0.0)
        else:
            peak = max(float(np.abs(f.real).max()), float(np.abs(f.imag).max()))
            scale = 2.0 ** np.ceil(np.log2(peak / 16384.0))
            raw = np.round(np.stack([f.real, f.imag], axis=-1) / scale).astype(np.int16)
            kw = dict(sample_format=la.FILE_SC16, sample_scale=float(scale))
        raw.tofile(p)
        pinned = torch.from_numpy(raw.view(np.float32 if fmt == "cf32" else np.int16).reshape(len(raw), -1)).pin_memory()   # what a radio driver's buffers are
        host = pinned.numpy().view(raw.dtype).reshape(raw.shape)
        files[fmt] = (p, kw, host, pinned)
        del raw
    del f
    say("stream_filter_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, LSN_FILE_BLOCK %d, pushes of %d samples from a "
        "pinned buffer, filter stopband %s Hz (L = %s), library %s; built in %.0f s" % (rate_in / 1e6, nsf, a.block, a.piece, "/".join("%.0f" % s for s in stops),
                                                                                       "/".join(str(h) for h in half), os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
    for k, (p, _, host, _) in files.items():
        say("  %-5s %d bytes, %d pushes" % (k, os.path.getsize(p), -(-len(host) // a.piece)))
        with open(p, "rb", buffering=0) as fh:   # read once: the first read of freshly written page-cache pages is slow whoever reads them
            buf = bytearray(64 << 20)
            while fh.readinto(buf):
                pass

    def phys():
        out = []
        for _ in offsets:
            w = la.PcapWriter(None)
            w.set_store(False)
            w.set_digest_blocks(BLOCK, tti0)
            phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=400, pcapwriter=w)
            assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
            out.append((phy, w))
        return out

    def leg(way, fmt, filt, track):
        p, kw, host, _ = files[fmt]
        ps = phys()
        for i, (phy, _) in enumerate(ps):      # the filter first: prepare_file then reserves the filter's intermediate with the block buffers
            assert phy.set_channel_filter(stops[i] if filt else 0.0)
            phy.prepare_file()
        cells = [(ps[i][0], dict(center_offset_hz=offsets[i], start_tti=tti0, offset_time=LEAD, update_meta_period=META)) for i in (0, 1)]
        ring = None
        if way == "file":
            t0 = time.perf_counter()
            done = la.process_file_cells(p, rate_in, cells, **kw)
            dt = time.perf_counter() - t0
        else:
            st = la.Stream(rate_in, cells, block_subframes=way, track=dict() if track else None, **kw)
            ring = st.status()["ring_samples"]
            t0 = time.perf_counter()
            for pos in range(0, len(host), a.piece):
                st.push(host[pos:pos + a.piece])
            done = st.flush()
            dt = time.perf_counter() - t0
            st.close()
        digests = []
        for phy, w in ps:
            digests.append(list(w.block_digests()))
            phy.close()
        return done, dt, digests, ring

    legs = [("file", False, False), ("file", True, False)] + [(b, filt, track) for b in sblocks for track in (False, True) for filt in (False, True)]
    rates = {}
    try:
        for rnd in range(a.rounds):
            for fmt in files:
                yard = {}
                for way, filt, track in legs:
                    done, dt, digests, ring = leg(way, fmt, filt, track)
                    if way == "file":
                        yard[filt] = (done, digests)
                    name = ("file" if way == "file" else "stream blk %d" % way) + ("+filter" if filt else "") + ("+track" if track else "")
                    rates.setdefault((fmt, name), []).append(sum(done) / dt)
                    say("round %d  %-5s %-28s %s subframes, %.0f cell-sf/s, %.1f ms%s (counts and digests %s the file pass's)" % (
                        rnd + 1, fmt, name, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3, "" if ring is None else ", ring %d samples" % ring,
                        "equal" if (done, digests) == yard[filt] else "DIFFER from"))
        for (fmt, name), v in rates.items():
            ref = statistics.median(rates[(fmt, "file+filter" if "+filter" in name else "file")])
            say("median of %d  %-5s %-28s %.0f cell-sf/s, range %.0f .. %.0f (%.2f of the file pass with the same filter setting)" % (
                len(v), fmt, name, statistics.median(v), min(v), max(v), statistics.median(v) / ref))
        say("lowest leg: %.0f cell-sf/s; two live cells need 1600" % min(min(v) for v in rates.values()))
        if not a.no_trace:
            pd = tempfile.mkdtemp(prefix="stream_filter_prof_")
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", pd, "--", sys.executable, os.path.abspath(__file__), "--block", str(a.block), "--piece", str(a.piece),
                   "--tti0", str(tti0), "--stop", repr(stops[0]), "--trace-block", str(sblocks[0]), "--child"] + ["%s,%d,%r" % (p, kw["sample_format"], kw["sample_scale"])
                                                                                                                 for p, kw, _, _ in files.values()]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
            durs = {}
            for p in glob.glob(os.path.join(pd, "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(p)):
                    name = r[_col(r, "kernel_name")].replace("(int)", "").replace("(bool)", "")
                    for k in ("k_chan_fir_ring<0>", "k_chan_fir_ring<1>", "k_chan_fir_cells<0>", "k_chan_fir_cells<1>", "k_chan_fir<", "k_resample_ring<", "k_resample<0, false>", "k_resample<"):
                        if k in name:
                            durs.setdefault(k, []).append(int(r[_col(r, "end_timestamp")]) - int(r[_col(r, "start_timestamp")]))
                            break
            shutil.rmtree(pd, ignore_errors=True)
            say("kernel trace of one filtered stream (blocks of %d) and one filtered file pass per format (%d subframes per cell; short last blocks included):" % (sblocks[0], nsf))
            for k, v in sorted(durs.items()):
                v.sort()
                say("  %-22s %3d launches, %8.1f us in all, median %7.1f us (%.1f - %.1f)" % (k, len(v), sum(v) / 1e3, v[len(v) // 2] / 1e3, v[0] / 1e3, v[-1] / 1e3))
    finally:
        for p, _, _, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
