#!/usr/bin/env python3
"""tools/resample_probe.py - the polyphase resampler's kernel alone (a measurement, no pass / fail).

Workload (--child; started by this script in a fresh process under rocprofv3): a 20 MHz, two-antenna block of 400 output subframes.  Per round, in this order:
k_resample from 25 MS/s cf32, 25 MS/s sc16, 61.44 MS/s cf32, 61.44 MS/s sc16 (lsn_resample, input and output resident on the device), then k_file_unpack on a
native-rate file of the same 400 subframes, cf32 and sc16 (lsn_phy_process_file, LSN_FILE_BLOCK=400: one launch per pass) - the baseline, interleaved with the
resampler round by round.  The first round is a warm-up and is left out.

  python tools/resample_probe.py [--rounds 6] [--out FILE]          kernel durations from `rocprofv3 --kernel-trace`: median and range per leg, bytes moved
                                                                     (input span read once + output written) per second
  python tools/resample_probe.py --pmc [--out FILE]                 a counter run of its own (SQ busy cycles, VALU / LDS activity, LDS bank conflicts) per launch
  --offset HZ    center_offset_hz of the k_resample legs (|HZ| <= 3.485e6 for the 25 MS/s legs): the mixing instantiations.  Without it (0) the legs pass the
                 struct up to passband_hz, which a library from before the mixer accepts as well: LSN_LIB_PATH=<that build> runs the same legs on it (A/B)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSF, NANT, SFLEN, RATE_OUT, B = 400, 2, 30720, 30.72e6, 15e3 * 601
RS_LEGS = [(25e6, 0, "cf32"), (25e6, 1, "sc16"), (61.44e6, 0, "cf32"), (61.44e6, 1, "sc16")]
COUNTERS = ["SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_WAIT_INST_LDS", "SQ_INSTS_VALU", "SQ_INSTS_LDS"]


def _cfg(rate_in, fmt, offset):
    import ltesniffer_amd as la
    cfg = la._resample_cfg(NANT, rate_in, RATE_OUT, 0, 0.0, 0, 0, B, fmt, 1.0 / 8192)
    if offset != 0.0:
        cfg.center_offset_hz = offset
    else:
        cfg.struct_size = la.ResampleCfg.center_offset_hz.offset
    return cfg


def _span(rate_in, fmt, offset):
    import ltesniffer_amd as la
    sp = la.ResampleSpan()
    rc = la.lib().lsn_resample_span(C.byref(_cfg(rate_in, fmt, offset)), NSF * SFLEN, 0, C.byref(sp))
    assert rc == 0, rc
    return dict(in_hi=int(sp.in_hi), taps=int(sp.taps))


def child(rounds, offset):
    import numpy as np
    import torch
    import ltesniffer_amd as la
    L = la.lib()
    rng = np.random.default_rng(1)
    n_out = NSF * SFLEN
    out = torch.zeros((NANT, n_out, 2), dtype=torch.float32, device="cuda:0")
    legs = []
    for rate_in, fmt, _ in RS_LEGS:
        n_in = _span(rate_in, fmt, offset)["in_hi"]
        x = rng.standard_normal((n_in, NANT, 2)).astype(np.float32) if fmt == 0 else rng.integers(-8000, 8000, (n_in, NANT, 2)).astype(np.int16)
        legs.append((torch.from_numpy(x).to("cuda:0"), n_in, _cfg(rate_in, fmt, offset)))
    os.environ["LSN_FILE_BLOCK"] = str(NSF)
    td = tempfile.mkdtemp(prefix="rs_probe_")
    try:
        files = []
        for fmt, dt in ((0, np.float32), (1, np.int16)):
            p = os.path.join(td, "n%d" % fmt)
            (rng.standard_normal((n_out, NANT, 2)) * (1 if fmt == 0 else 3000)).astype(dt).tofile(p)
            files.append((p, fmt))
        phy = la.Phy(nof_rx_antennas=NANT, max_batch=400, pcapwriter=la.PcapWriter(None))
        assert phy.setCell(100, 2, 1)
        phy.prepare_file()
        for _ in range(rounds + 1):
            for x, n_in, cfg in legs:
                rc = L.lsn_resample(0, C.c_void_p(x.data_ptr()), 1, n_in, C.byref(cfg), C.c_void_p(out.data_ptr()), 1, n_out)
                assert rc == 0, rc
            for p, fmt in files:
                assert phy.process_file(p, sample_format=fmt, sample_scale=1.0 / 8192) == NSF
        phy.close()
    finally:
        shutil.rmtree(td, ignore_errors=True)


def _col(row, *want):
    for k in row:
        if all(w in k.lower() for w in want):
            return k
    raise KeyError(want)


def _run(prof_args, rounds, offset):
    td = tempfile.mkdtemp(prefix="rs_prof_")
    cmd = ["rocprofv3"] + prof_args + ["--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(rounds),
                                       "--offset", repr(offset)]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return td


def _kind(name):
    """k_resample<FMT> / k_file_unpack<FMT>: the first template argument (k_resample has a second one, the mixer, since center_offset_hz exists)"""
    m = re.search(r"(k_resample|k_file_unpack)<(\d)", name)
    return "%s<%s>" % m.groups() if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--offset", type=float, default=0.0)
    a = ap.parse_args()
    if a.child:
        return child(a.rounds, a.offset)
    import ltesniffer_amd as la
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n_out = NSF * SFLEN
    spans = {(r, f): _span(r, f, a.offset) for r, f, _ in RS_LEGS}
    if not a.pmc:
        td = _run(["--kernel-trace"], a.rounds, a.offset)
        seq = {}
        for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(p)):
                k = _kind(r[_col(r, "kernel_name")])
                if k:
                    seq.setdefault(k, []).append((int(r[_col(r, "start_timestamp")]), int(r[_col(r, "end_timestamp")])))
        shutil.rmtree(td, ignore_errors=True)
        say("resample_probe: 20 MHz, 2 antennas, %d output subframes per launch (%d outputs per antenna), %d timed rounds interleaved, warm-up round left out, center_offset_hz %g, library %s" %
            (NSF, n_out, a.rounds, a.offset, os.path.relpath(la.LIB_PATH, ROOT)))

        def report(label, durs, nbytes, extra=""):
            d = sorted(durs)
            med = d[len(d) // 2]
            say("  %-34s %7.1f us median (%.1f - %.1f, n = %d)  %6.2f TB/s of %d bytes per launch%s" % (label, med / 1e3, d[0] / 1e3, d[-1] / 1e3, len(d), nbytes / med / 1e3, nbytes, extra))

        for fmt in (0, 1):
            v = [e - s for s, e in sorted(seq.get("k_resample<%d>" % fmt, []))]
            per = [(25e6, v[0::2]), (61.44e6, v[1::2])]     # the order of the child's legs
            for rate, durs in per:
                sp = spans[(rate, fmt)]
                nb = sp["in_hi"] * NANT * (8 if fmt == 0 else 4) + n_out * NANT * 8
                report("k_resample %s from %.2f MS/s" % (("cf32", "sc16")[fmt], rate / 1e6), durs[1:], nb, ", %d taps" % sp["taps"])
            u = [e - s for s, e in sorted(seq.get("k_file_unpack<%d>" % fmt, []))]
            report("k_file_unpack %s (baseline)" % ("cf32", "sc16")[fmt], u[1:], n_out * NANT * ((8 if fmt == 0 else 4) + 8))
    else:
        td = _run(["--kernel-trace", "--pmc"] + COUNTERS, 2, a.offset)
        acc = {}   # (kernel, counter) -> {dispatch: value summed over the rows of the dispatch}
        for p in glob.glob(os.path.join(td, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(p)):
                k = _kind(r[_col(r, "kernel_name")])
                if k:
                    d = acc.setdefault((k, r[_col(r, "counter_name")]), {})
                    i = int(r[_col(r, "dispatch_id")])
                    d[i] = d.get(i, 0.0) + float(r[_col(r, "counter_value")])
        shutil.rmtree(td, ignore_errors=True)
        say("resample_probe --pmc: counters per launch, %d output subframes per launch" % NSF)
        for k in ("k_resample<0>", "k_resample<1>", "k_file_unpack<0>", "k_file_unpack<1>"):
            for label, pick in ((("from 25 MS/s", 0), ("from 61.44 MS/s", 1)) if "resample" in k else (("", None),)):
                vals = []
                for c in COUNTERS:
                    if (k, c) in acc:
                        ids = sorted(acc[k, c])
                        ids = ids if pick is None else ids[pick::2]     # the order of the child's legs
                        vals.append("%s %.3e" % (c.replace("SQ_", ""), sum(acc[k, c][i] for i in ids) / max(1, len(ids))))
                say("  %-18s %-16s " % (k, label) + "  ".join(vals))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
