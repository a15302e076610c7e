#!/usr/bin/env python3
"""tools/stream_probe.py - two cells of one 61.44 MS/s recording, pushed as a live stream against replayed as a file (a measurement, no pass / fail).

The recording is tools/cells_probe.py's: a cut of the cfg3 capture of bench.py on both carriers (+9.9 and -9.9 MHz) of a two-cell 61.44 MS/s recording, as a cf32 and
as an sc16 file.  Per format and round, each from cold Phys with the block buffers reserved (lsn_phy_prepare_file):
  (a) file    one process_file_cells call on the file (page cache), timed around the call: the yardstick
  (b) stream  the same bytes, read into ONE pinned host buffer beforehand, pushed through a Stream in pieces of 1 ms (61 440 samples) and flushed; timed from the
              first push to the end of the flush.  One row per --stream-blocks entry (block_subframes: how many subframes a cell collects before it is submitted)
Rounds are interleaved (file, stream, file, stream, ...); the summary is the median of the rounds.  Printed with every figure: cell-subframes per second (2 x
subframes / wall time) and whether the block digests of both cells equal those of the same round's file pass - they must be: the stream feeds every Phy the file
pass's samples, bit for bit.  How the recording compares with the oracle's block digests is cells_probe.py's business, not this probe's.

  python tools/stream_probe.py [--subframes 800] [--rounds 3] [--block 100] [--stream-blocks 100,10] [--piece 61440] [--formats cf32,sc16] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every replay and stream (two Phys hold their block buffers at once)")
    ap.add_argument("--stream-blocks", default="100,10", help="block_subframes of the stream rows")
    ap.add_argument("--piece", type=int, default=61440, help="samples per push (61 440 = 1 ms)")
    ap.add_argument("--formats", default="cf32,sc16")
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
    sblocks = [int(v) for v in a.stream_blocks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    rate_in, f = wideband([(iq, f0, 1.0) for f0 in offsets], 2, 1, 30.72e6, channel_hz=SPACING)
    del iq
    td = tempfile.mkdtemp(prefix="stream_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
    say("stream_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, LSN_FILE_BLOCK %d, pushes of %d samples from a pinned buffer, "
        "library %s; built in %.0f s" % (rate_in / 1e6, nsf, a.block, a.piece, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
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
            phy.prepare_file()
            out.append((phy, w))
        return out

    def leg(way, fmt):
        p, kw, host, _ = files[fmt]
        ps = phys()
        cells = [(ps[i][0], dict(center_offset_hz=offsets[i], start_tti=tti0, offset_time=LEAD, update_meta_period=META)) for i in (0, 1)]
        ring = None
        if way == "file":
            t0 = time.perf_counter()
            done = la.process_file_cells(p, rate_in, cells, **kw)
            dt = time.perf_counter() - t0
        else:
            st = la.Stream(rate_in, cells, block_subframes=way, **kw)
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

    rates = {}
    try:
        for rnd in range(a.rounds):
            for fmt in files:
                yard = None
                for way in ["file"] + sblocks:
                    done, dt, digests, ring = leg(way, fmt)
                    if way == "file":
                        yard = (done, digests)
                    name = "file" if way == "file" else "stream blk %d" % way
                    rates.setdefault((fmt, name), []).append(sum(done) / dt)
                    say("round %d  %-5s %-15s %s subframes, %.0f cell-sf/s, %.1f ms%s (counts and digests %s the file pass's)" % (
                        rnd + 1, fmt, name, "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3, "" if ring is None else ", ring %d samples" % ring,
                        "equal" if (done, digests) == yard else "DIFFER from"))
        for (fmt, name), v in rates.items():
            say("median of %d  %-5s %-15s %.0f cell-sf/s (%.2f of the file pass)" % (len(v), fmt, name, statistics.median(v), statistics.median(v) / statistics.median(rates[(fmt, "file")])))
    finally:
        for p, _, _, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
