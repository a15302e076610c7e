#!/usr/bin/env python3
"""tools/resample_replay_probe.py - file replay through the polyphase resampler against the native-rate replay (a measurement, no pass / fail).

A cut of the cfg3 capture of bench.py (tools/make_cfg3_golden.py: 20 MHz, two antennas, 30.72 MS/s) is taken to 25 MS/s by zero-padding / truncating the
spectrum of the whole cut in float64 (tests/resample_cases.fft_convert; the cut continues periodically behind its end) and written as a cf32 and as an sc16
file.  Legs, interleaved round by round, each from a cold Phy with the block buffers reserved (lsn_phy_prepare_file):
  native cf32    lsn_phy_process_file on the 30.72 MS/s file (the baseline; LSN_LIB_PATH selects the build, e.g. the parent commit's library)
  25 MS/s cf32   lsn_phy_process_file_rate
  25 MS/s sc16   lsn_phy_process_file_rate, one LSB = 2^-13
Every pass is hashed in blocks of 200 subframes and compared with tests/golden/cfg3_stream_oracle.json (the oracle on the 30.72 MS/s cf32 capture); the
number of differing blocks is printed next to each figure.

  python tools/resample_replay_probe.py [--subframes 1000] [--rounds 3] [--legs native,cf32,sc16] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # host-program configuration of the HIP runtime, before its first call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="native,cf32,sc16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import ltesniffer_amd as la
    from make_cfg3_golden import cfg3_stream
    from parity import gen_capture
    from resample_cases import fft_convert
    sc, NSF, BLOCK, META = cfg3_stream()
    nsf = min(a.subframes, NSF) // BLOCK * BLOCK
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")))["blocks"]
    legs = a.legs.split(",")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.time()
    tti0, iq = gen_capture(sc, nsf)
    td = tempfile.mkdtemp(prefix="rs_replay_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    files = {}
    x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, sc["nof_rx"])   # [sample][antenna]
    if "native" in legs:
        files["native"] = (os.path.join(td, "native.cf32"), {})
        x.tofile(files["native"][0])
    if "cf32" in legs or "sc16" in legs:
        y = np.stack([fft_convert(x[:, r], 625, 768) for r in range(x.shape[1])], axis=1)
        y = np.concatenate([y, y[:4096]])
        rate = dict(sample_rate=25e6)
        if "cf32" in legs:
            files["cf32"] = (os.path.join(td, "r25.cf32"), rate)
            y.astype(np.complex64).tofile(files["cf32"][0])
        if "sc16" in legs:
            files["sc16"] = (os.path.join(td, "r25.sc16"), dict(rate, sample_format=la.FILE_SC16, sample_scale=2.0 ** -13))
            np.round(np.stack([y.real, y.imag], axis=-1) * 2.0 ** 13).astype(np.int16).tofile(files["sc16"][0])
        del y
    say("resample_replay_probe: cfg3 capture, %d of %d distinct subframes, 2 antennas, library %s; rendered and converted in %.0f s" %
        (nsf, NSF, os.path.relpath(la.LIB_PATH, ROOT), time.time() - t))
    for k, (p, _) in files.items():
        say("  %-7s %d bytes per subframe" % (k, os.path.getsize(p) // nsf))
        with open(p, "rb", buffering=0) as f:   # read once: the first read of freshly written page-cache pages is slow whoever reads them
            buf = bytearray(64 << 20)
            while f.readinto(buf):
                pass

    def leg(k):
        p, kw = files[k]
        w = la.PcapWriter(None)
        w.set_store(False)
        w.set_digest_blocks(BLOCK, tti0)
        phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=400, pcapwriter=w)
        assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
        phy.prepare_file()
        t0 = time.perf_counter()
        n = phy.process_file(p, start_tti=tti0, update_meta_period=META, **kw)
        dt = time.perf_counter() - t0
        blocks = w.block_digests()
        bad = sum(1 for j, (d, c) in enumerate(blocks) if ["%016x" % d, c] != list(golden[j]))
        phy.close()
        return "%d subframes, %.0f sf/s (%d of %d blocks differ)" % (n, n / dt, bad, len(blocks))

    try:
        for rnd in range(a.rounds):
            for k in legs:
                say("round %d  %-7s %s" % (rnd + 1, k, leg(k)))
    finally:
        for p, _ in files.values():
            os.remove(p)
        os.rmdir(td)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
