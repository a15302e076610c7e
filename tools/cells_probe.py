#!/usr/bin/env python3
"""tools/cells_probe.py - two cells of one 61.44 MS/s recording: two passes over the file against one (a measurement, no pass / fail).

A cut of the cfg3 capture of bench.py (tools/make_cfg3_golden.py: 20 MHz, two antennas, 30.72 MS/s) is put on BOTH carriers of a two-cell recording the way
tests/ddc_cases.wideband builds one (whole-cut FFT conversion to 61.44 MS/s, each copy confined to its 19.8 MHz channel, moved to +9.9 and -9.9 MHz with an
integer phase, added) and written as a cf32 and as an sc16 file.  Both carriers carry the same cell, so BOTH replays are gated on the oracle's block digests of
tests/golden/cfg3_stream_oracle.json; to the file source they are two cells like any other two (two Phys, two plans, two tuning words).
Three ways, interleaved round by round, each from cold Phys with the block buffers reserved (lsn_phy_prepare_file), timed around the replay call(s) only:
  (a) sequential   two process_file_rate calls, one after the other: the way before lsn_file_process_cells, the yardstick
  (b) threads      the same two calls from two threads at once
  (c) one pass     one process_file_cells call
Printed with every figure: cell-subframes per second (2 x subframes / wall time), the number of digest blocks that differ from the oracle's, whether the block
digests of both cells equal those of the same round's sequential replay (the three ways must decode the same records whatever the recording does to them), and
the bytes of the file read and copied to the GPU per cell-subframe (a and b read every byte once per cell, c once).

  python tools/cells_probe.py [--subframes 800] [--rounds 2] [--block 100] [--formats cf32,sc16] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--block", type=int, default=100, help="LSN_FILE_BLOCK of every replay (two Phys hold their block buffers at once)")
    ap.add_argument("--formats", default="cf32,sc16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["LSN_FILE_BLOCK"] = str(a.block)
    import numpy as np
    import ltesniffer_amd as la
    from ddc_cases import SPACING, wideband
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    from resample_cases import LEAD
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")))["blocks"]
    offsets = (9.9e6, -9.9e6)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    rate_in, f = wideband([(iq, f0, 1.0) for f0 in offsets], 2, 1, 30.72e6, channel_hz=SPACING)
    del iq
    td = tempfile.mkdtemp(prefix="cells_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
    say("cells_probe: cfg3 capture on two carriers (+-9.9 MHz) of a %.2f MS/s recording, %d subframes per cell, 2 antennas, LSN_FILE_BLOCK %d, library %s; built in %.0f s" %
        (rate_in / 1e6, nsf, a.block, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
    for k, (p, _) in files.items():
        size = os.path.getsize(p)
        say("  %-5s %d bytes; read and copied per cell-subframe: sequential / threads %d, one pass %d" % (k, size, size // nsf, size // (2 * nsf)))
        with open(p, "rb", buffering=0) as fh:   # read once: the first read of freshly written page-cache pages is slow whoever reads them
            buf = bytearray(64 << 20)
            while fh.readinto(buf):
                pass

    yard = {}

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
        p, kw = files[fmt]
        ps = phys()
        done = [0, 0]

        def one(i):
            done[i] = ps[i][0].process_file_rate(p, rate_in, center_offset_hz=offsets[i], start_tti=tti0, offset_time=LEAD, update_meta_period=META, **kw)

        t0 = time.perf_counter()
        if way == "sequential":
            one(0)
            one(1)
        elif way == "threads":
            th = [threading.Thread(target=one, args=(i,)) for i in (0, 1)]
            for x in th:
                x.start()
            for x in th:
                x.join()
        else:
            done = la.process_file_cells(p, rate_in, [(ps[i][0], dict(center_offset_hz=offsets[i], start_tti=tti0, offset_time=LEAD, update_meta_period=META)) for i in (0, 1)], **kw)
        dt = time.perf_counter() - t0
        bad, total, digests = 0, 0, []
        for phy, w in ps:
            blocks = w.block_digests()
            digests.append(list(blocks))
            bad += sum(1 for j, (d, c) in enumerate(blocks) if ["%016x" % d, c] != list(golden[j]))
            total += len(blocks)
            phy.close()
        if way == "sequential":
            yard[fmt] = digests
        return "%s subframes, %.0f cell-sf/s, %.1f ms (%d of %d blocks differ from the oracle's; digests %s the sequential replay's)" % (
            "+".join(str(n) for n in done), sum(done) / dt, dt * 1e3, bad, total, "equal" if digests == yard[fmt] else "DIFFER from")

    try:
        for rnd in range(a.rounds):
            for fmt in files:
                for way in ("sequential", "threads", "one pass"):
                    say("round %d  %-5s %-10s %s" % (rnd + 1, fmt, way, leg(way, fmt)))
    finally:
        for p, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
