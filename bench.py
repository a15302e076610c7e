#!/usr/bin/env python3
"""bench.py - subframes/s of the MI355X-native LTESniffer worker on BASELINE.json's metric config (configs[2] = "cfg3").

The stream (one definition, shared with tools/make_cfg3_golden.py): the cfg3 capture SURVEY.md 8(d) specifies - 20 000 DISTINCT synthetic
subframes, 150 RNTIs, a fresh RNTI by RAR every 200 subframes (the MCS-tracking database crosses its 250 entries and ages), TM2/3/4 up to
256QAM - replayed cyclically with the TTI advancing and all sequential state (RNTI histograms, MCS tables, meta formats) carried over; meta
formats update every 500 subframes.  A "step" is one pass of the hot path (OFDM -> chest -> PCFICH/PDCCH -> exhaustive Viterbi -> FALCON
search -> PDSCH demod -> rate de-matching -> turbo -> MAC PDUs into the MAC-LTE pcap writer) over the next --step-sf (20 000) subframes of
that stream.  IQ is in HBM before the timed region starts (`value`); the PCIe-inclusive rates - first H2D to last PDU, SURVEY 8(d) - are the
`first_h2d_to_last_pdu` legs of the same line.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--step-sf 20000] [--batch 400] [--dump-outputs DIR] [--full [--cpu-sample 1600]]

A plain run sets up, warms up, times the K steps, gates them on the cached oracle stream and prints the line.  --full adds what the headline
does not need, each outside the timed region: the live CPU oracle (cpu_baseline, and the head-of-stream check of ranks > 0), the
first-H2D-to-last-PDU legs and the other BASELINE configurations (--no-cpu / --no-legs leave parts of it out).  --dump-outputs DIR writes the
MAC-LTE records of the last timed step as .npy files (see dump_last_step).

Parity gate: `pcap_diff` describes the TIMED stream against the CPU ORACLE.  The oracle walked the first 100 000 subframes of the stream once
(one thread - its state is a sequential scan; 35 subframes/s) and its records were hashed per block of 200 subframes
(tests/golden/cfg3_stream_oracle.json, made by tools/make_cfg3_golden.py, keyed by the xxh3 of the capture bytes).  The pcap writer hashes
the records of the timed steps with the same block structure (lsn_pcap_set_digest_blocks); every block of the timed region must equal the
oracle's block of the same stream position, record count and digest.  The same check covers the warm-up (cold-state) steps and both passes
of every PCIe-inclusive leg.  On top (--full), the oracle runs live on the first --cpu-sample subframes (cpu_baseline) and must reproduce the
cached blocks on this host.

N > 1: `--gpus N` launches N ranks itself (python -m torch.distributed.run, one process per GPU, backend nccl = RCCL) unless it already
runs under one (RANK / WORLD_SIZE set, which is how the driver starts it).  Every rank replays its own synthetic cell (BASELINE
configs[4]: cells shard with no data-path exchange) -> weak scaling; value = all ranks' subframes / max-over-ranks time; rank 0's cell is
the gated one."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _maybe_spawn(argv):
    """--gpus N without a launcher: start N ranks (one per GPU) and relay rank 0's line"""
    n = 1
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            n = int(argv[i + 1])
        elif a.startswith("--gpus="):
            n = int(a.split("=", 1)[1])
    if n <= 1 or "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    sys.exit(subprocess.call(cmd, env=env))


_maybe_spawn(sys.argv[1:])

# HIP runtime configuration of the host program (read when the runtime initialises, i.e. before the first HIP call): the engine keeps 12 decode chains +
# 4 stage-A chains + copies in flight; on the runtime's default of 4 hardware queues they wait for each other's kernels (INTEGRATION.md section 2;
# measured in round 4: + 2 % with 16).  An exported value wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

_CPU_CTX = None


def _thread_cpu():
    """CPU seconds (user+system) of every thread of this process, keyed by (tid, name)"""
    out = {}
    tck = os.sysconf("SC_CLK_TCK")
    for tid in os.listdir("/proc/self/task"):
        try:
            st = open(f"/proc/self/task/{tid}/stat").read()
        except OSError:
            continue
        name = st[st.index("(") + 1:st.rindex(")")]
        f = st[st.rindex(")") + 2:].split()
        out[(int(tid), name)] = (int(f[11]) + int(f[12])) / tck
    return out


def _cpu_slice(k):
    sc, tti0, iq, gen, per, run_oracle = _CPU_CTX
    a = (k * per) % max(1, gen - per)
    run_oracle(sc, tti0 + a, iq[a:a + per], update_meta_period=500, taps=False)
    return 0


def _profile_json(key):
    """profiles/current.json names the rocprofv3 summaries of this tree (tools/gpu_profile.sh); None when absent OR when they were taken from
    another tree (current.json records the tree hash of the profiled sources)"""
    try:
        cur = json.load(open(os.path.join(ROOT, "profiles", "current.json")))
        if cur.get("tree_hash") != tree_hash():
            return None, None
        return json.load(open(os.path.join(ROOT, "profiles", cur[key]))), cur[key]
    except Exception:
        return None, None


def _profile_state():
    try:
        cur = json.load(open(os.path.join(ROOT, "profiles", "current.json")))
        return {"profiled_tree_hash": cur.get("tree_hash"), "this_tree_hash": tree_hash(), "match": cur.get("tree_hash") == tree_hash()}
    except Exception:
        return {"profiled_tree_hash": None, "this_tree_hash": tree_hash(), "match": False}


sys.path.insert(0, os.path.join(ROOT, "tools"))
from tree_hash import tree_hash  # noqa: E402  (hash of the product sources: profile summaries are only quoted for the tree they were taken from)


GOLDEN = os.path.join(ROOT, "tests", "golden", "cfg3_stream_oracle.json")


def _pcie_link(local):
    """negotiated host link of the GPU (sysfs): GT/s x lanes -> GB/s per direction before protocol overhead"""
    try:
        pr = torch.cuda.get_device_properties(local)
        bus = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        sp = open("/sys/bus/pci/devices/%s/current_link_speed" % bus).read().split()[0]
        wd = int(open("/sys/bus/pci/devices/%s/current_link_width" % bus).read())
        gts = float(sp)
        return {"GT_per_s": gts, "lanes": wd, "raw_GB_per_s": round(gts * wd / 8.0 * (128.0 / 130.0), 1),
                "measured_memcpy_GB_per_s": 57.5, "measured_by": "tools/ubench/h2d_bw.hip, profiles/r03_h2d_bw.txt"}
    except Exception:
        return None


def auto_step_sf(nsf, steps, warmup, cached, block=200):
    """--step-sf 0: the largest step (a divisor of the capture, a multiple of the digest block) whose whole run - warm-up and timed steps - lies inside the
    cached oracle stream, so that every timed block has an oracle block to be compared with"""
    fit = [s_ for s_ in (20000, 10000, 5000, 4000, 2000, 1000, 400, 200) if s_ % block == 0 and nsf % s_ == 0 and (steps + warmup) * s_ <= cached]
    return fit[0] if fit else block


def dump_last_step(out_dir, pcap_path, blocks, origin_tti, lo, hi, block=200, pdu_budget=8 << 20):
    """--dump-outputs: what a caller of the timed path receives from its last step - the MAC-LTE records of stream positions [lo, hi) (subframes
    since origin_tti, the first timed subframe) out of the pcap file the timed steps wrote (timestamps zero) - as out_dir/*.npy:
      records.npy          float32 [n, 6]: tti, rnti, direction, rnti_type, crc_ok, PDU length - every record of the step, in stream order
      pdu_sample.npy       float32: the PDU bytes of a fixed, seeded sample of those records (at most pdu_budget bytes), concatenated in record order
      pdu_sample_rows.npy  float64: the rows of records.npy the sample holds
      block_digests.npy    float64 [(hi - lo) / block, 3]: the pcap writer's digest of every 200-subframe block of the step (high and low 32 bits) and its
                           record count - covers every byte of every record"""
    import struct
    buf = np.fromfile(pcap_path, dtype=np.uint8)
    mv = memoryview(buf)
    offs, off, end = [], 24, buf.size  # 24-byte file header, then per record 16 bytes (ts, ts, length, length) + 19-byte MAC-LTE context + PDU
    while off + 35 <= end:
        offs.append(off)
        off += 16 + struct.unpack_from("<I", mv, off + 8)[0]
    o = np.array(offs, dtype=np.int64) + 16
    ln = buf[o[:, None] - 8 + np.arange(4)].copy().view(np.uint32)[:, 0].astype(np.int64) - 19
    fs = buf[o + 10].astype(np.int64) << 8 | buf[o + 11]
    tti = (fs >> 4) * 10 + (fs & 15)
    # stream position of every record: its TTI unwrapped from record to record, as the writer's block digests count them
    want = (tti - origin_tti) % 10240
    pos = np.cumsum(np.concatenate([[max(0, (int(want[0]) + 5120) % 10240 - 5120)], (np.diff(want) + 5120) % 10240 - 5120])) if want.size else want
    keep = (pos >= lo) & (pos < hi)
    o, ln = o[keep], ln[keep]
    rec = np.stack([tti[keep], buf[o + 4].astype(np.int64) << 8 | buf[o + 5], buf[o + 1], buf[o + 2], buf[o + 13], ln], axis=1).astype(np.float32)
    order = np.random.default_rng(0).permutation(len(o))
    rows = np.sort(order[:int(np.searchsorted(np.cumsum(ln[order]), pdu_budget, side="right"))])
    sample = np.concatenate([buf[o[r] + 19:o[r] + 19 + ln[r]] for r in rows]).astype(np.float32) if rows.size else np.zeros(0, np.float32)
    bd = np.zeros(((hi - lo) // block, 3), dtype=np.float64)
    for j, (d, c) in enumerate(blocks[lo // block:hi // block]):
        bd[j] = (d >> 32, d & 0xFFFFFFFF, c)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in (("records", rec), ("pdu_sample", sample), ("pdu_sample_rows", rows.astype(np.float64)), ("block_digests", bd)):
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "records": int(len(o)), "pdu_sample_records": int(rows.size), "bytes": int(rec.nbytes + sample.nbytes + 8 * rows.size + bd.nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-sf", type=int, default=0, help="subframes per step: a divisor of the capture length and a multiple of 200.  0 (default) = 20 000 (one pass of the "
                    "capture: the driver's 20 timed steps last 2 s; rounds 1-4 used 4 000, a timed region of 0.4 s of which pipeline fill / drain was 5 %%) when the cached "
                    "oracle stream covers (warmup + steps) x 20 000 subframes, otherwise the largest step the cache covers completely: the headline is never printed ungated "
                    "because the cache is shorter than the run")
    ap.add_argument("--nsf", type=int, default=0, help="distinct subframes of the capture (0 = the gated stream's 20 000); other values run ungated")
    ap.add_argument("--config", default="cfg3", help="scenario preset: cfg3 = 20 MHz, 150 RNTIs, TM3/TM4 up to 256QAM")
    ap.add_argument("--batch", type=int, default=400, help="subframes per pipeline chunk inside a submit (400-500 measured best on the 4 000-subframe steps: shorter fill / drain than 800, fewer launches than 200)")
    ap.add_argument("--cpu-sample", type=int, default=1600, help="--full: subframes the CPU oracle decodes live from cold state (rank 0): cpu_baseline + reproduction of the cached oracle blocks")
    ap.add_argument("--full", action="store_true", help="after the headline, also run the live CPU oracle (cpu_baseline, head of the stream of ranks > 0), the first-H2D-to-last-PDU "
                    "legs and the other BASELINE configurations; without it a run does only what the headline needs")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the live oracle leg (cpu_baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the MAC-LTE records of the last timed step to DIR/*.npy (rank 0; the timed steps then also write "
                    "their records to a pcap file on tmpfs, as the host_pinned_pcap_to_file leg does)")
    ap.add_argument("--shard", choices=("cells", "capture"), default="cells",
                    help="N > 1: 'cells' = one synthetic cell per rank (weak scaling, the default and what BASELINE configs[4] asks for); 'capture' = ONE capture "
                         "whose chunks go round-robin to the N GPUs (lsn_phy_create_multi on rank 0; the other ranks only hold their GPU) - strong scaling, "
                         "bounded by the sequential FALCON search on one host thread")
    ap.add_argument("--workload", default="", help="a downlink leg of tools/bench_legs.py (e.g. cfg3_at_16_dB_snr) as the TIMED stream instead of the headline capture - its capture, "
                    "its cached oracle stream, the same gate: how the second operating point is profiled (tools/gpu_profile.sh) with its own roofline figures; never the driver's line")
    ap.add_argument("--no-legs", action="store_true", help="--full without the PCIe-inclusive legs (host buffers, capture file, worker pool) and the other configs")
    ap.add_argument("--leg-batch", type=int, default=0, help="pipeline chunk of the first-H2D-to-last-PDU legs (0 = --batch)")
    ap.add_argument("--gen-threads", type=int, default=0, help="threads of the synthetic transmitter (0 = the CPUs this process may use, at most 32)")
    args = ap.parse_args()
    if not args.full:  # a plain run: the timed steps and their gate only
        args.no_cpu = args.no_legs = True

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("LSN_DIST_BACKEND", "nccl")  # nccl = RCCL on ROCm; "gloo" only to smoke-test N > 1 on a 1-GPU box
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
            local = local % max(1, torch.cuda.device_count())
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (the library has no CPU path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    # host threads and host buffers next to the GPU: pinned staging, the page-cache pages of the capture file and the caller's own arrays are
    # first touched by this process, and a far-socket source halves the PCIe rate (the engine pins its own threads the same way)
    try:
        pr = torch.cuda.get_device_properties(local)
        bus = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bus).read())
        if node >= 0:
            cpus = set()
            for tok in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
                a, _, b = tok.partition("-")
                cpus.update(range(int(a), int(b or a) + 1))
            cpus &= os.sched_getaffinity(0)
            if cpus:
                os.sched_setaffinity(0, cpus)
    except Exception:
        pass

    # N ranks share the host: a rank keeps ~3 cores busy with 8 decode threads (host.cores_busy_in_timed_region).  Under a CPU quota smaller
    # than that (cgroup cpu.max; the 1-GPU boxes of this pool give 16 cores) the CFS throttle stalls whole ranks, so the pipeline is narrowed
    # instead: fewer decode threads per rank (each costs ~0.3 core, search + front + commit + writer ~0.9).
    host_quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        host_quota = float(q) / float(per) if q != "max" else float(len(os.sched_getaffinity(0)))
    except Exception:
        host_quota = float(len(os.sched_getaffinity(0)))
    if world > 1 and "LSN_DECODE_THREADS" not in os.environ and host_quota / world < 3.4:
        os.environ["LSN_DECODE_THREADS"] = str(max(3, min(8, int((host_quota / world - 0.9) / 0.3))))

    import ltesniffer_amd as la
    from lsn_testlib import scenario
    from parity import gen_capture, run_oracle
    from ltesniffer_amd import dist as ld
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_cfg3_golden import BLOCK, META_PERIOD, NSF, capture_hash

    wl_leg = None
    if args.workload:
        import bench_legs as bl_
        wl_leg = bl_.LEGS[args.workload]
        assert wl_leg["kind"] == "dl" and world == 1, "--workload: a downlink leg on one GPU"
    gated_cfg = (args.config == "cfg3" and args.nsf in (0, NSF)) or wl_leg is not None
    nsf = wl_leg["nsf"] if wl_leg else (NSF if gated_cfg else max(BLOCK, (args.nsf or NSF) // BLOCK * BLOCK))
    step_sf_auto = None
    if args.step_sf <= 0:
        # every rank reads the same file, so every rank arrives at the same step
        args.step_sf = 20000
        try:
            cached = json.load(open(bl_.golden_path(args.workload) if wl_leg is not None else GOLDEN))["oracle_subframes"] if gated_cfg else 0
        except Exception:
            cached = 0
        if cached:
            args.step_sf = auto_step_sf(nsf, args.steps, args.warmup, cached, BLOCK)
            step_sf_auto = {"cached_oracle_subframes": cached, "chosen": args.step_sf,
                            "rule": "largest of 20000 / 10000 / 5000 / 4000 / 2000 / 1000 / 400 / 200 with (warmup + steps) x step <= cached oracle subframes"}
    S = max(BLOCK, min(args.step_sf, nsf) // BLOCK * BLOCK)
    while nsf % S:
        S -= BLOCK  # a step never straddles the wrap of the capture
    batch = min(args.batch or S, S)
    # the work queue (which cell each rank replays: SURVEY 8d config 5, one capture per GPU; rank 0 = the gated stream) lives on rank 0 and is
    # scattered - over RCCL / xGMI under the nccl backend: the path's only exchange step besides the timing reductions (BASELINE north_star)
    rdev_ = dev if world > 1 and dist.get_backend() == "nccl" else None
    work = ld.scatter_work([tuple(ld.rank_workload(args.config, r).values()) + (0, nsf) for r in range(world)] if rank == 0 else None, rdev_)
    sc = scenario(args.config, seed=work["seed"], cell_id=work["cell_id"]) if wl_leg is None else bl_.leg_scenario(args.workload)
    gen_threads = args.gen_threads or max(1, min(32, int(host_quota // max(1, world)) if host_quota else 8))
    # N ranks share the host's cores: a rank other than 0 (its cell is not the gated stream) renders fewer distinct subframes when it has few
    # transmitter threads - its work per step is unchanged, the block is replayed.  Captures are kept in /dev/shm between the back-to-back runs
    # of a scaling series (LSN_BENCH_NO_CACHE=1 switches that off).
    nsf_gen = nsf
    if rank > 0 and gen_threads < 6 and nsf % 5 == 0 and (nsf // 5) % S == 0:
        nsf_gen = nsf // 5
    t_gen = time.perf_counter()
    cache, iq = None, None
    if not os.environ.get("LSN_BENCH_NO_CACHE"):
        import hashlib
        key = hashlib.sha256((json.dumps(sc, sort_keys=True) + str(nsf_gen) + open(os.path.join(ROOT, "tools", "txgen", "txgen.cc")).read()).encode()).hexdigest()[:16]
        cache = "/dev/shm/lsn_bench_capture_%s.cf32" % key
        try:
            if os.path.getsize(cache) == nsf_gen * sc["nof_rx"] * 15 * {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}[sc["nof_prb"]] * 8:
                iq = np.fromfile(cache, dtype=np.complex64).reshape(nsf_gen, sc["nof_rx"], -1)
                tti0 = sc["start_tti"]
        except OSError:
            iq = None
    if iq is None:
        tti0, iq = gen_capture(sc, nsf_gen, threads=gen_threads)
        if cache:
            try:
                iq.tofile(cache + ".tmp%d" % os.getpid())
                os.replace(cache + ".tmp%d" % os.getpid(), cache)
            except OSError:
                pass
    if nsf_gen != nsf:
        iq = np.tile(iq, (nsf // nsf_gen, 1, 1))
    t_gen = time.perf_counter() - t_gen
    sf_bytes = iq[0].nbytes
    # the resident capture [nsf][rx][15*N] interleaved cf32 in HBM (9.8 GB at 20 MHz / 2 rx / 20 000 subframes), uploaded in slices
    d_iq = torch.empty((nsf,) + iq.shape[1:] + (2,), dtype=torch.float32, device=dev)
    for a in range(0, nsf, 2000):
        d_iq[a:a + 2000].copy_(torch.from_numpy(iq[a:a + 2000].view(np.float32).reshape(-1, iq.shape[1], iq.shape[2], 2)))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    golden, golden_note = None, None
    if rank == 0 and wl_leg is not None:
        golden, golden_note = bl_.load_golden(args.workload, iq, tti0)
    elif rank == 0 and gated_cfg:
        try:
            g = json.load(open(GOLDEN))
            chash, _ = capture_hash(iq)
            if g["capture_xxh3_64"] != chash:
                golden_note = "the capture rendered on this host (xxh3 %s) is not the one the cached oracle stream was made from (%s)" % (chash, g["capture_xxh3_64"])
            elif g["stream"]["block_subframes"] != BLOCK or g["stream"]["tti0"] != tti0 or g["stream"]["meta_period"] != META_PERIOD:
                golden_note = "cached oracle stream was made with another block / tti0 / meta period"
            else:
                golden = g
        except Exception as ex:
            golden_note = "no cached oracle stream: %s" % str(ex)[:120]

    def block_check(blocks, first_block, gold=None):
        """product blocks [(digest, nrec)] against the oracle's blocks from stream position first_block on -> (covered, mismatching blocks, record diff)"""
        gold = gold or golden
        if gold is None:
            return 0, None, None
        ob = gold["blocks"]
        n = max(0, min(len(blocks), len(ob) - first_block))
        bad, rd = 0, 0
        for j in range(n):
            d, c = blocks[j]
            if "%016x" % d != ob[first_block + j][0] or c != ob[first_block + j][1]:
                bad += 1
                rd += abs(c - ob[first_block + j][1])
        return n, bad, rd

    capture_mode = args.shard == "capture" and (world > 1 or os.environ.get("LSN_BENCH_DEVICES"))
    devices = None
    if capture_mode:
        devices = [int(x) for x in os.environ["LSN_BENCH_DEVICES"].split(",")] if os.environ.get("LSN_BENCH_DEVICES") else list(range(world))
    if capture_mode and rank != 0:  # the capture is driven by rank 0's process (one search thread, one record stream); this rank's GPU is one of its devices
        dist.barrier()
        dist.barrier()
        dist.destroy_process_group()
        return
    dump_pcap = None
    if args.dump_outputs and rank == 0:  # the records of the timed steps go to a file as well (the last step's are dumped after the run)
        import tempfile
        fd, dump_pcap = tempfile.mkstemp(prefix="lsn_bench_dump_", suffix=".pcap", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
        os.close(fd)
    pcap = la.PcapWriter(dump_pcap, wall_clock=False)  # native MAC-LTE writer, the reference's pcap-emit surface; the stream is digested per block, not kept
    pcap.set_store(False)
    pcap.set_digest_blocks(BLOCK, tti0)
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, device=local, pcapwriter=pcap, devices=devices, harq_mode=(wl_leg or {}).get("harq_mode", 0))
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
    stride = sf_bytes

    def submit_step(p, i):
        pos = (i * S) % nsf
        p.submit_device(d_iq.data_ptr() + pos * stride, S, (tti0 + i * S) % 10240, META_PERIOD, stream)  # LTESniffer_Core.cc:434: meta-format update every 500 subframes

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup):
        submit_step(phy, i)
    phy.wait()
    dt_warm = time.perf_counter() - t0
    pw = phy.perf()
    warm_blocks = pcap.block_digests()
    warm_records = pcap.nof_records()
    pcap.reset()
    pcap.set_digest_blocks(BLOCK, (tti0 + args.warmup * S) % 10240)  # blocks of the timed region count from its first subframe
    pcap.set_store(dump_pcap is not None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    import resource
    ru0 = resource.getrusage(resource.RUSAGE_SELF)
    thr0 = _thread_cpu()
    t0 = time.perf_counter()
    # the K steps are submitted back to back (lsn_phy_submit_device only queues; search / decode / commit / write of a step overlap the
    # next one's stage A) and completed by one lsn_phy_wait inside the timed region
    for i in range(args.steps):
        submit_step(phy, args.warmup + i)
    phy.wait()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if os.environ.get("LSN_BENCH_STAMP"):   # wall-clock stamps of the timed region: processes that share a GPU (tools/r6_session6.sh) show whether their regions overlapped
        print("[stamp] timed region %.3f .. %.3f (unix s)" % (time.time() - dt, time.time()), file=sys.stderr)
    ru1 = resource.getrusage(resource.RUSAGE_SELF)
    thr1 = _thread_cpu()
    p = phy.perf()
    timed_digest, timed_bytes = pcap.digest()
    timed_records = pcap.nof_records()
    timed_blocks = pcap.block_digests()
    host_cores_busy = ((ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)) / dt
    per_rank_cores = None
    if world > 1 and not capture_mode:
        rdev = dev if dist.get_backend() == "nccl" else None
        per_rank_cores = [v / 100.0 for v in ld.gather_flags(int(round(host_cores_busy * 100)), rdev)]  # host CPU each rank kept busy in ITS timed region
        dt, total = ld.reduce_max_sum(dt, args.steps * S, rdev)
        assert total == args.steps * S * world
    total_sf = args.steps * S * (1 if capture_mode else world)
    value = total_sf / dt
    # proof of what ran where: the collective backend torch.distributed really used, the world it saw, every rank's device (PCI bus id) - gathered over that backend
    pr_ = torch.cuda.get_device_properties(local)
    my_bus = (int(pr_.pci_domain_id) << 16) | (int(pr_.pci_bus_id) << 8) | int(pr_.pci_device_id)
    dist_echo = {"backend": None, "world_size": world, "devices_pci": ["%04x:%02x:%02x" % (my_bus >> 16, (my_bus >> 8) & 0xFF, my_bus & 0xFF)], "device_count_visible": torch.cuda.device_count()}
    if world > 1 and not capture_mode:
        rdev2 = dev if dist.get_backend() == "nccl" else None
        buses = ld.gather_flags(my_bus, rdev2)
        dist_echo.update({"backend": dist.get_backend() + (" (RCCL)" if dist.get_backend() == "nccl" else ""), "world_size": dist.get_world_size(),
                          "devices_pci": ["%04x:%02x:%02x" % (b >> 16, (b >> 8) & 0xFF, b & 0xFF) for b in buses], "distinct_devices": len(set(buses))})
    phy.close()
    dumped = None
    if dump_pcap is not None:
        pcap.close()  # flushes the file
        try:
            dumped = dump_last_step(args.dump_outputs, dump_pcap, timed_blocks, (tti0 + args.warmup * S) % 10240, (args.steps - 1) * S, args.steps * S, BLOCK)
        finally:
            os.remove(dump_pcap)

    def live_oracle_blocks(n):
        """the CPU oracle, live, over the first n subframes of THIS rank's capture from cold state -> (blocks [(digest, records)], seconds, records)"""
        ob = la.PcapWriter(None)
        ob.set_store(False)
        ob.set_digest_blocks(BLOCK, tti0)
        t = time.perf_counter()
        _, _, orecs = run_oracle(sc, tti0, iq[:n], update_meta_period=META_PERIOD, taps=False)
        dto = time.perf_counter() - t
        for r in orecs:  # the oracle's records through the product's block hash
            c = r["ctx"]
            fs = (c[10] << 8) | c[11]
            ob.write(dict(tti=(fs >> 4) * 10 + (fs & 15), rnti=(c[4] << 8) | c[5], direction=c[1], rnti_type=c[2], crc_ok=c[13]), r["pdu"])
        return ob.block_digests()[:n // BLOCK], dto, len(orecs)

    # ranks other than 0 replay cells of their own (no cached oracle stream): each checks the head of ITS cold-state stream - the first 400 subframes
    # of the warm-up - against the oracle run live on its host cores; the verdicts travel to rank 0 (round-4 review: "ranks > 0 are ungated")
    rank_flags = None
    if world > 1 and not capture_mode:
        flag = -1
        if rank > 0 and not args.no_cpu and args.warmup * S >= 2 * BLOCK:
            lb, _, _ = live_oracle_blocks(2 * BLOCK)
            flag = 1 if (len(lb) == 2 and warm_blocks[:2] == lb) else 0
        rank_flags = ld.gather_flags(flag, dev if dist.get_backend() == "nccl" else None)

    # ---------------------------------------------------------------- parity gate (rank 0): timed blocks == the oracle's blocks
    cpu, parity, pcap_diff = None, None, None
    if rank == 0:
        parity = {"reference": "CPU oracle (oracle/, scalar C restatement; unpinned against srsRAN soft values, DESIGN.md section 2), cached per 200-subframe block by tools/make_cfg3_golden.py",
                  "timed_subframes": args.steps * S, "timed_records": timed_records, "timed_bytes": timed_bytes, "timed_digest": "%016x" % timed_digest,
                  "block_subframes": BLOCK, "golden_note": golden_note}
        if rank_flags is not None:  # 1 = the rank's first 400 subframes equal the live oracle's, 0 = they differ, -1 = not checked (rank 0: gated on the cached stream)
            parity["other_ranks_head_equals_live_oracle"] = rank_flags[1:]
        if golden is not None:
            nb = args.steps * S // BLOCK
            cov, bad, rd = block_check(timed_blocks[:nb] + [(0, 0)] * max(0, nb - len(timed_blocks)), args.warmup * S // BLOCK)
            wcov, wbad, _ = block_check(warm_blocks[:args.warmup * S // BLOCK], 0)
            parity.update({"oracle_subframes": cov * BLOCK, "oracle_blocks_compared": cov, "oracle_blocks_mismatching": bad,
                           "oracle_stream_subframes_cached": golden["oracle_subframes"], "oracle_source_hash": golden.get("source_hash"),
                           "oracle_records_in_timed_region": sum(c for _, c in golden["blocks"][args.warmup * S // BLOCK:args.warmup * S // BLOCK + cov]),
                           "timed_equals_oracle": bool(cov == nb and bad == 0), "warmup_blocks_compared": wcov, "warmup_blocks_mismatching": wbad,
                           "distinct_subframes_in_timed_region": min(nsf, args.steps * S)})
            if cov == nb:
                pcap_diff = int(rd + (bad if rd == 0 else 0))
        ns = max(BLOCK, min(args.cpu_sample, nsf) // BLOCK * BLOCK)
        if not args.no_cpu:
            lb, dto, _ = live_oracle_blocks(ns)
            cpu = {"value": round(ns / dto, 2), "unit": "subframes/s", "cores": 1, "kind": "port",
                   "sample": "the first %d subframes of the same capture (cold RNTI state), scalar C oracle, 1 thread" % ns}
            if golden is not None:
                cov, bad, _ = block_check(lb, 0)
                parity["live_oracle_reproduces_cached_blocks"] = bool(cov == len(lb) and bad == 0)
            if args.warmup * S >= ns:  # ... and the product's cold-state blocks equal the LIVE oracle's, cache or not
                parity["warmup_equals_live_oracle_blocks"] = bool(warm_blocks[:len(lb)] == lb)
                if golden is None and pcap_diff is None:
                    parity["oracle_subframes"] = ns
                    parity["note"] = "no cached oracle stream for this capture: only the first %d warm-up subframes are oracle-checked; pcap_diff stays null" % ns
            if world == 1:
                # BASELINE.json configs[0] / BASELINE.md section 3: 10 MHz, one RNTI, TM1 QPSK, one CRS port, one rx antenna, CFO 300 Hz - the CPU path on this host's cores
                try:
                    sc1 = scenario("cfg1", seed=1)
                    n1 = 2000
                    t1, iq1 = gen_capture(sc1, n1, threads=gen_threads)
                    t = time.perf_counter()
                    _, _, r1 = run_oracle(sc1, t1, iq1, update_meta_period=META_PERIOD, taps=False)
                    dt1 = time.perf_counter() - t
                    cpu["configs0"] = {"value": round(n1 / dt1, 1), "unit": "subframes/s", "x_realtime": round(n1 / dt1 / 1000.0, 3), "cores": 1, "kind": "port", "records": len(r1),
                                       "sample": "BASELINE configs[0]: %d subframes of a synthetic 10 MHz capture (50 PRB, 1 port, 1 rx, one C-RNTI, TM1 QPSK, SIB1, CFO 300 Hz), scalar C oracle, 1 thread" % n1}
                    del iq1
                except Exception as ex:
                    cpu["configs0"] = {"error": str(ex)[:200]}
                # the same restatement on many cores: forked workers on independent 200-subframe slices, each with its own (cold) state - an
                # upper bound for a subframe-parallel CPU run of this code (the sequential RNTI state is not shared), informational only
                try:
                    import multiprocessing as mp
                    W = max(1, min(16, (os.cpu_count() or 2) // 2))
                    per = 200
                    global _CPU_CTX
                    _CPU_CTX = (sc, tti0, iq, nsf, per, run_oracle)
                    with mp.get_context("fork").Pool(W) as pool:
                        t = time.perf_counter()
                        pool.map(_cpu_slice, range(W))
                        dtp = time.perf_counter() - t
                    cpu["parallel"] = {"value": round(W * per / dtp, 1), "unit": "subframes/s", "cores": W,
                                       "sample": "%d forked workers x %d subframes, independent cold RNTI state each" % (W, per)}
                except Exception as ex:
                    cpu["parallel"] = {"error": str(ex)[:200]}

    # ---------------------------------------------------------------- first H2D -> last PDU: the capture starts in HOST memory
    # Never `value` (bench contract: inputs resident in HBM): the whole 20 000-subframe capture, three consecutive passes of the SAME stream
    # from a fresh engine - pass 1 from cold state, passes 2 and 3 with the tables learnt - each gated block by block on the oracle like the headline:
    # (a) host buffers (lsn_phy_process_host: PCIe copies overlapped with the pipeline), (b) a cf32 file in the page cache
    # (lsn_phy_process_file, the reference's file mode, LTESniffer_Core.cc:240-262,365), (c) the reference's own boundary: the worker pool
    # (getAvail / getBuffers / prepare / putPending / joinPending, LTESniffer_Core.cc:434-451) driven by tools/pool_driver.
    legs = None
    if rank == 0 and world == 1 and not args.no_legs:
        legs = {"pcie_link": _pcie_link(local)}

        def two_passes(name, make_phy, run_pass, extra=None, pcap_path=None, gold=None, sf_bytes=sf_bytes):
            lp = la.PcapWriter(pcap_path)   # pcap_path: the records go to a FILE like the reference's (PcapWriter.cc:75-118), digested on the way
            if pcap_path is None:
                lp.set_store(False)
            lphy = make_phy(lp)
            lphy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
            out = {}
            for k in range(3):
                lp.reset()
                lp.set_digest_blocks(BLOCK, (tti0 + k * nsf) % 10240)
                t = time.perf_counter()
                done = run_pass(lphy, (tti0 + k * nsf) % 10240)
                dtl = time.perf_counter() - t
                cov, bad, rd = block_check(lp.block_digests()[:done // BLOCK], k * nsf // BLOCK, gold)
                out["pass%d_%s" % (k + 1, "cold" if k == 0 else "warm")] = {   # (the third consecutive pass is the steady state: buffers grown, tables learnt)
                    "subframes_per_s": round(done / dtl, 1), "GB_per_s": round(done * sf_bytes / dtl / 1e9, 2), "x_realtime": round(done / dtl / 1000.0, 1),
                    "subframes": int(done), "records": lp.nof_records(), "oracle_blocks_compared": cov, "oracle_blocks_mismatching": bad,
                    "pcap_diff": (int(rd + (bad if rd == 0 else 0)) if cov == done // BLOCK and cov else None)}
            if extra:
                out.update(extra)
            lphy.close()
            if pcap_path is not None:
                lp.close()
                out["pcap_file_bytes"] = os.path.getsize(pcap_path)
                os.remove(pcap_path)
            legs[name] = out

        try:
            host = torch.from_numpy(iq).pin_memory()
            lbatch = args.leg_batch or batch
            legs["chunk_subframes"] = lbatch
            two_passes("host_pinned", lambda w: la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=lbatch, device=local, pcapwriter=w),
                       lambda ph, t: (ph.process_host(host.numpy(), t, META_PERIOD), nsf)[1])
            two_passes("host_pinned_pcap_to_file", lambda w: la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=lbatch, device=local, pcapwriter=w),
                       lambda ph, t: (ph.process_host(host.numpy(), t, META_PERIOD), nsf)[1],
                       {"note": "as host_pinned, the MAC-LTE records written to a pcap file on tmpfs (three passes in one file) instead of only digested"},
                       pcap_path="/dev/shm/lsn_bench_%d.pcap" % os.getpid())
            two_passes("host_pageable", lambda w: la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=lbatch, device=local, pcapwriter=w),
                       lambda ph, t: (ph.process_host(iq, t, META_PERIOD), nsf)[1], {"note": "registered in place (hipHostRegister) for the call"})
            # the reference's boundary: 1024 workers (1.5 GB pinned slab), chunks of up to 512 subframes; producer = 1 thread like LTESniffer_Core, then 4 copy threads
            import ctypes as C
            pd = C.CDLL(os.path.join(ROOT, "tools", "pool_driver", "_build", "libpool_driver.so"))
            pd.pool_drive.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
            for nthr in (1, 4):
                def drive(ph, t, nthr=nthr):
                    secs = C.c_double(0)
                    rc = pd.pool_drive(ph._h, host.numpy().ctypes.data, nsf, sc["nof_rx"], iq.shape[2], t, META_PERIOD, nthr, C.byref(secs))
                    assert rc == 0, "pool_drive failed: %d" % rc
                    return nsf
                two_passes("worker_pool_%d_producer_thread%s" % (nthr, "" if nthr == 1 else "s"),
                           lambda w: la.Phy(nof_rx_antennas=sc["nof_rx"], nof_workers=1024, max_batch=512, device=local, pcapwriter=w), drive,
                           {"nof_workers": 1024, "max_batch": 512, "driver": "tools/pool_driver (getAvail -> memcpy into getBuffers -> prepare -> putPending, joinPending)"})
            del host
            path = "/dev/shm/lsn_bench_capture_%d.cf32" % os.getpid()
            with open(path, "wb") as f:  # file mode: antennas interleaved per sample
                for a in range(0, nsf, 1000):
                    np.ascontiguousarray(np.transpose(iq[a:a + 1000], (0, 2, 1))).tofile(f)
            # The file is read once before the engine opens it: the FIRST read of freshly written page-cache pages is slow whoever reads them (every 393 MB
            # block took the twelve reader threads 13-16 ms = 26 GB/s in the first replay and 3.7-5 ms = 100 GB/s in the following ones, reserved and
            # pre-touched block buffers or not: profiles/r05_file_cold_probe_a.txt) - a property of a file written a moment ago, not of the file source.
            t_pre = time.perf_counter()
            with open(path, "rb", buffering=0) as f:
                buf = bytearray(64 << 20)
                while f.readinto(buf):
                    pass
            t_pre = time.perf_counter() - t_pre
            try:
                def file_phy(w):   # file mode is known at start-up (the reference parses -i first): the block buffers are reserved with the engine (lsn_phy_prepare_file)
                    ph = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=lbatch, device=local, pcapwriter=w)
                    ph.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
                    ph.prepare_file()
                    return ph
                two_passes("file_replay", file_phy,
                           lambda ph, t: ph.process_file(path, start_tti=t, update_meta_period=META_PERIOD),
                           {"storage": "tmpfs (/dev/shm) = page cache, read once after it was written (%.2f s, outside the timed passes); pread threads -> pinned blocks -> PCIe" % t_pre})
            finally:
                os.remove(path)
            # The same capture as a 16-bit recording (lsn_file_cfg_t.sample_format = LSN_FILE_SC16: int16 I/Q pairs, what the radio sends over its link;
            # an extension - the reference's file mode opens cf32 only): half the bytes per subframe cross PCIe, the GPU converts.  Gated on its OWN
            # oracle stream (tests/golden/cfg3_stream_sc16_oracle.json: the oracle walked the dequantised subframes, tools/make_cfg3_golden.py --sc16).
            try:
                from make_cfg3_golden import sc16_capture
                q16, lsb = sc16_capture(iq)
                g16, note16 = None, None
                try:
                    g16 = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg3_stream_sc16_oracle.json")))
                    if capture_hash(q16)[0] != g16["capture_xxh3_64"] or g16["stream"]["tti0"] != tti0 or g16["stream"]["block_subframes"] != BLOCK:
                        g16, note16 = None, "the 16-bit recording made on this host is not the one the cached oracle stream was made from"
                except Exception as ex:
                    g16, note16 = None, "no cached oracle stream: %s" % str(ex)[:120]
                path = "/dev/shm/lsn_bench_capture_%d.sc16" % os.getpid()
                with open(path, "wb") as f:
                    for a in range(0, nsf, 1000):
                        np.ascontiguousarray(np.transpose(q16[a:a + 1000], (0, 2, 1, 3))).tofile(f)
                # ... and in pinned host buffers (lsn_phy_process_host_int: what a radio driver delivers when asked not to convert), same stream, same gate
                hq = torch.from_numpy(q16).pin_memory()
                del q16
                two_passes("host_pinned_sc16", lambda w: la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=lbatch, device=local, pcapwriter=w),
                           lambda ph, t: (ph.process_host_int(hq.numpy(), t, META_PERIOD, sample_scale=lsb), nsf)[1],
                           {"sample_format": "int16 I/Q pairs in pinned host memory, one LSB = %g" % lsb, "bytes_per_subframe": sf_bytes // 2,
                            "oracle_stream": "tests/golden/cfg3_stream_sc16_oracle.json", "golden_note": note16},
                           gold=g16 or {"blocks": []}, sf_bytes=sf_bytes // 2)
                del hq
                with open(path, "rb", buffering=0) as f:
                    buf = bytearray(64 << 20)
                    while f.readinto(buf):
                        pass
                try:
                    two_passes("file_replay_sc16", file_phy,
                               lambda ph, t: ph.process_file(path, start_tti=t, update_meta_period=META_PERIOD, sample_format=la.FILE_SC16, sample_scale=lsb),
                               {"sample_format": "int16 I/Q pairs, one LSB = %g (a power of two: the conversion on the GPU is exact)" % lsb, "bytes_per_subframe": sf_bytes // 2,
                                "oracle_stream": "tests/golden/cfg3_stream_sc16_oracle.json (its own: the oracle on the dequantised subframes)", "golden_note": note16},
                               gold=g16 or {"blocks": []}, sf_bytes=sf_bytes // 2)
                finally:
                    os.remove(path)
            except Exception as ex:
                legs["file_replay_sc16"] = {"error": str(ex)[:300]}
        except Exception as ex:
            legs["error"] = str(ex)[:300]

    # ---------------------------------------------------------------- the other BASELINE.json configurations (tools/bench_legs.py: LEGS)
    # configs[1] (20 MHz, 32 RNTIs, TM2 64QAM), the same on four CRS ports, configs[2] at 16 dB, the same with HARQ soft combining, configs[3]
    # (UL_MODE, PUSCH at n + 4) - context numbers next to the headline, never `value`.  Since round 5 EVERY one of them is gated like the headline:
    # the oracle walked each leg's whole stream (cold pass + timed passes, state carried over) once, tests/golden/leg_<name>.json holds its
    # records hashed per 200-subframe block, and the leg prints oracle_blocks_compared / mismatching / pcap_diff for ALL its passes.
    if legs is not None and "error" not in legs:
        import bench_legs as bl
        only = os.environ.get("LSN_BENCH_LEGS")  # development: comma-separated subset
        for name, ld in bl.LEGS.items():
            if only is not None and name not in only.split(","):
                continue
            try:
                scl, tl, iql = bl.leg_capture(name, threads=gen_threads)
                gl, gnote = bl.load_golden(name, iql, tl)
                wl = la.PcapWriter(None)
                wl.set_store(False)
                wl.set_digest_blocks(bl.BLOCK, tl)
                nl, npass = ld["nsf"], ld["passes"]
                if ld["kind"] == "dl":
                    pl = la.Phy(nof_rx_antennas=scl["nof_rx"], max_batch=batch, device=local, pcapwriter=wl, harq_mode=ld.get("harq_mode", 0))
                    pl.setCell(scl["nof_prb"], scl["nof_ports"], scl["cell_id"])
                    dl_ = torch.empty((nl,) + iql.shape[1:] + (2,), dtype=torch.float32, device=dev)
                    for a_ in range(0, nl, 2000):
                        dl_[a_:a_ + 2000].copy_(torch.from_numpy(iql[a_:a_ + 2000].view(np.float32).reshape(-1, iql.shape[1], iql.shape[2], 2)))
                    torch.cuda.synchronize()
                    pl.process_device(dl_.data_ptr(), nl, tl % 10240, bl.META_PERIOD, stream)   # pass 1: cold state, untimed
                    t = time.perf_counter()
                    for r in range(1, npass):
                        pl.submit_device(dl_.data_ptr(), nl, (tl + r * nl) % 10240, bl.META_PERIOD, stream)
                    pl.wait()
                    dtl = time.perf_counter() - t
                    inp = "resident in HBM"
                    del dl_
                else:
                    hl = torch.from_numpy(iql).pin_memory()
                    pl = la.Phy(nof_rx_antennas=2, sniffer_mode=1, max_batch=200, device=local, pcapwriter=wl)
                    pl.setCell(scl["nof_prb"], scl["nof_ports"], scl["cell_id"])
                    pl.setUlConfig(ld["cyclic_shift"], ld["delta_ss"])
                    pl.process_host(hl.numpy(), tl % 10240, bl.META_PERIOD)
                    t = time.perf_counter()
                    for r in range(1, npass):
                        pl.process_host(hl.numpy(), (tl + r * nl) % 10240, bl.META_PERIOD)
                    dtl = time.perf_counter() - t
                    inp = "host buffers (two antenna streams), PCIe included"
                    del hl
                pfl = pl.perf()  # (counters of the last submit ... wait span = the timed passes; UL_MODE: the last pass)
                nb = npass * nl // bl.BLOCK
                blocks = wl.block_digests()[:nb]
                blocks += [(0x9E3779B97F4A7C15, 0)] * (nb - len(blocks))
                cov, bad, rd = bl.check_blocks(gl, blocks, 0)
                timed = (npass - 1) * nl
                counted = timed if ld["kind"] == "dl" else nl
                legs[name] = {"what": ld["what"], "subframes_per_s": round(timed / dtl, 1), "subframes": timed, "timed_s": round(dtl, 3), "records_all_passes": wl.nof_records(), "input": inp,
                              "turbo_iterations_per_subframe": round(pfl.nof_turbo_iterations / float(counted), 1), "tb_decodes_per_subframe": round(pfl.nof_tb_decodes / float(counted), 2),
                              "pdus_per_subframe": round(pfl.nof_pdus / float(counted), 2),
                              "oracle_subframes": cov * bl.BLOCK, "oracle_blocks_compared": cov, "oracle_blocks_mismatching": bad,
                              "pcap_diff": (int(rd + (bad if rd == 0 else 0)) if gl is not None and cov == nb else None), "golden_note": gnote}
                if ld.get("harq_mode"):   # retransmissions: batches run ahead of the commit walk / combined decodes taken from a batch / decoded alone inside the turn / batch results never asked for
                    legs[name]["harq_combines"] = dict(zip(("batches", "from_a_batch", "alone_in_the_commit_turn", "batch_results_unused"), [int(x) for x in pfl.nof_harq_combines]))
                    legs[name]["harq_commit_ms"] = {"scout": round(pfl.ms_harq[0], 1), "batches": round(pfl.ms_harq[1], 1), "flush": round(pfl.ms_harq[2], 1), "commit_turns_all": round(pfl.ms_commit, 1), "stage_c_all_threads": round(pfl.ms_stage_c, 1)}
                pl.close()
                del iql
            except Exception as ex:
                legs[name] = {"error": str(ex)[:300]}

    if rank == 0:
        kms = np.array(p.kernel_ms[:])
        klaunch = np.array(p.kernel_launches[:])
        per_thr = {}
        for k, v in thr1.items():
            per_thr[k[1]] = per_thr.get(k[1], 0.0) + (v - thr0.get(k, 0.0)) / dt
        busiest = {k: round(v, 2) for k, v in sorted(per_thr.items(), key=lambda kv: -kv[1])[:8] if v >= 0.01}
        if os.environ.get("LSN_BENCH_ALL_THREADS"):
            print("[threads] " + json.dumps({k: round(v, 3) for k, v in sorted(per_thr.items(), key=lambda kv: -kv[1]) if v >= 0.005}), file=sys.stderr)
        nk = len(la.KERNELS)
        dom = int(np.argmax(kms[:nk]))
        sf_rank = args.steps * S  # subframes this rank processed in the timed region
        # roofline of the dominant kernel (one of the two turbo-decoder variants).  Algorithmic bytes = what the decoder must move per code
        # block: its K + 12 packed soft words (4 B each, written by k_rm) in, payload bytes out.  Duration: HIP events on the launch stream,
        # i.e. the launch's own span while it shares the GPU with the kernels of the other streams (NOT an exclusive time); the rocprofv3
        # kernel trace of the same command (tools/gpu_profile.sh -> profiles/) gives the same average and the exclusive (union) time.
        k64, k128 = la.KERNELS.index("k_turbo<64>"), la.KERNELS.index("k_turbo<128>")
        kt = k128 if kms[k128] >= kms[k64] else k64
        kbytes = p.turbo128_algo_bytes if kt == k128 else p.turbo_algo_bytes - p.turbo128_algo_bytes
        ach = (kbytes / 1e9) / (kms[kt] / 1e3) if kms[kt] > 0 else 0.0
        traffic, traffic_src = None, None
        hj, hname = _profile_json("pmc_hbm")
        if hj and hj.get(la.KERNELS[kt]):
            e = hj[la.KERNELS[kt]]
            traffic = int(e["fetch_corrected_bytes_per_launch"] + e["write_bytes_per_launch"])
            traffic_src = "profiles/" + hname
        rp, rpname = _profile_json("kernel_trace")  # {kernel: {calls, avg_ms, exclusive_ms, ...}, _subframes, _wall_ms} of the driver's command
        rocprof = None
        bytes_per_sf = kbytes / max(1, sf_rank)
        if rp and rp.get(la.KERNELS[kt]):
            e = rp[la.KERNELS[kt]]
            hip_avg = kms[kt] / max(1, klaunch[kt])
            ex = e.get("exclusive_ms_per_subframe")
            rocprof = {"avg_launch_ms": e.get("avg_ms"), "launches": e.get("calls"), "exclusive_ms_per_subframe": ex,
                       # launches of one kernel overlap each other and the other kernels: launches x average span exceeds the step time.  The time that
                       # can be ATTRIBUTED to the kernel is the union of its launch intervals (exclusive time); the rate on that time:
                       "achieved_on_exclusive_time_GBps": round(bytes_per_sf / 1e9 / (ex / 1e3), 2) if ex else None,
                       "frac_on_exclusive_time": round(bytes_per_sf / 1e9 / (ex / 1e3) / 8000.0, 6) if ex else None,
                       "hip_event_over_rocprof_avg": round(hip_avg / e["avg_ms"], 3) if e.get("avg_ms") else None, "source": "profiles/" + rpname}
        valu, saturation = None, None
        vj, vname = _profile_json("pmc_sq")
        try:
            if vj and vj.get(la.KERNELS[kt]) and kms[kt] > 0:
                sub = float(vj["_subframes"])
                # peak: 1024 SIMDs x 2.4 GHz / 2 cycles per wave-instruction (SIMD-32, MI355X_MICROARCH.md) = 1228.8 G/s; the packed 16-bit and
                # 3-operand forms the two decoders are made of occupy the port for 4 cycles (profiles/r03_valu_peak_isa.txt): 614.4 G/s
                peak = float(vj.get("_peak_G_wave_insts_per_s", 1228.8))
                ins = vj[la.KERNELS[kt]]["SQ_INSTS_VALU"]["total"] / sub
                g = ins / (kms[kt] / sf_rank * 1e6)
                allk = sum(v["SQ_INSTS_VALU"]["total"] for k, v in vj.items() if not k.startswith("_") and "SQ_INSTS_VALU" in v and k.startswith("k_")) / sub
                valu = {"kernel_wave_insts_per_subframe": int(ins), "achieved_G_per_s": round(g, 1), "peak_G_per_s": peak, "frac": round(g / peak, 4),
                        "all_kernels_wave_insts_per_subframe": int(allk), "chip_G_per_s_at_this_rate": round(allk * value / world / 1e9, 1),
                        "chip_frac": round(allk * value / world / 1e9 / peak, 4), "chip_frac_of_4_cycle_class_peak": round(allk * value / world / 1e9 / (peak / 2.0), 4),
                        "source": "profiles/" + vname}
                # how full is the GPU?  The counter passes run every kernel ALONE (rocprofv3 serialises profiled dispatches): the sum of those stand-alone
                # launch times per subframe is what a one-kernel-at-a-time schedule would need; the pipelined engine needs 1 / value.  (A launch alone is
                # far from its instruction time - the 12-iteration tail of hopeless code blocks leaves the chip to a few workgroups - so the ratio says
                # how much of that idle time the overlap of 12 streams recovers, not how close the chip is to an instruction-issue bound.)
                alone = {}
                for k, v in vj.items():
                    if k.startswith("_") or "SQ_WAVES" not in v:
                        continue
                    alone[k] = v["SQ_WAVES"]["ns"] / sub / 1e3
                tot = sum(alone.values())
                saturation = {"sum_of_standalone_kernel_us_per_subframe": round(tot, 3), "pipelined_us_per_subframe": round(1e6 * world / value, 3),
                              "overlap_gain": round(tot / (1e6 * world / value), 2),
                              "standalone_us_per_subframe": {k: round(v, 3) for k, v in sorted(alone.items(), key=lambda kv: -kv[1])[:8]}, "source": "profiles/" + vname}
        except Exception:
            valu = None
        cold = None
        if args.warmup * S >= 2 * batch:
            cold = {"subframes_per_s": round(args.warmup * S / dt_warm, 1), "subframes": args.warmup * S, "records": warm_records,
                    "tb_decodes_per_subframe": round(pw.nof_tb_decodes / (args.warmup * S), 2), "turbo_iterations_per_subframe": round(pw.nof_turbo_iterations / (args.warmup * S), 1),
                    "note": "the warm-up steps: a fresh engine (empty RNTI histograms, no MCS-table knowledge), pipeline fill and drain included"}
        def leg_rate(name, which):
            return ((legs or {}).get(name) or {}).get(which, {}).get("subframes_per_s") if legs else None

        def leg_diffs(name):
            e = (legs or {}).get(name) or {}
            return [e.get(k, {}).get("pcap_diff") for k in ("pass1_cold", "pass2_warm", "pass3_warm")] if e else None
        h2d_cold, h2d_warm = leg_rate("host_pinned", "pass1_cold"), leg_rate("host_pinned", "pass3_warm")
        out = {
            "metric": "subframes/s (20 MHz, 150 RNTIs)", "value": round(value, 1), "unit": "subframes/s", "n_gpus": world if not capture_mode or world > 1 else len(devices),
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True, "scaling": "strong" if capture_mode else "weak", "vs_baseline": None, "dtype": "f32+int16", "data": "synthetic",
            # `value` follows the bench contract (the capture is resident in HBM when the timed region starts).  BASELINE.md section 3's clock - first H2D -> last PDU on the
            # host, PCIe included, fresh engine - is value_first_h2d_to_last_pdu (cold pass) / _warm (third pass); x_realtime is given on both clocks, by name
            "value_resident": round(value, 1), "x_realtime": round(value / 1000.0 / (1 if capture_mode else world), 2),
            "x_realtime_resident": round(value / 1000.0 / (1 if capture_mode else world), 2),
            "x_realtime_first_h2d_to_last_pdu": {"cold": round(h2d_cold / 1000.0, 1) if h2d_cold else None, "warm": round(h2d_warm / 1000.0, 1) if h2d_warm else None,
                                                 # the same capture held as int16 pairs (the radio's own sample format; an extension, lsn_phy_process_host_int): half the bytes
                                                 "cold_int16_samples": round(leg_rate("host_pinned_sc16", "pass1_cold") / 1000.0, 1) if leg_rate("host_pinned_sc16", "pass1_cold") else None,
                                                 "warm_int16_samples": round(leg_rate("host_pinned_sc16", "pass3_warm") / 1000.0, 1) if leg_rate("host_pinned_sc16", "pass3_warm") else None},
            "pcap_diff": pcap_diff,
            # BASELINE.md section 3 times "first H2D -> last PDU on host"; the bench contract wants inputs resident in HBM for `value`.  Both are here:
            # `value` = resident, `value_first_h2d_to_last_pdu` = the whole capture from pinned host memory through a FRESH engine (cold RNTI / MCS state, PCIe
            # included), the number to hold against BASELINE's >= 50 x real time
            "value_first_h2d_to_last_pdu": h2d_cold, "value_first_h2d_to_last_pdu_warm": h2d_warm,
            "parity_reference": "in-repo CPU oracle; its DSP is unpinned vs srsRAN (absent dependency); its search / grant / tracking logic is pinned on the reference's own compiled code (oracle/_ref, CPU suite)", "parity": parity,
            "config": {"workload": "%s: 20 MHz DL (100 PRB, 2 CRS ports, 2 rx), 150 active RNTIs + a fresh RNTI by RAR every 200 subframes, TM2/TM3/TM4 mix up to 256QAM, "
                                   "CFI 3, 8-14 DL + 3-6 UL DCIs per subframe (BASELINE.json configs[2], SURVEY 8d config 3)" % args.config
                       if args.config == "cfg3" and wl_leg is None else (args.workload + ": " + wl_leg["what"] if wl_leg else args.config),
                       "subframes_per_step": S, "subframes_per_step_auto": step_sf_auto, "distinct_subframes": nsf, "stream": "capture replayed cyclically, TTI and sequential state carried over",
                       "input": "resident in HBM", "steps_pipelined": True, "gpu_batch": batch, "cells": 1 if capture_mode else world, "capture_gen_s": round(t_gen, 1),
                       # (the driver keeps `config`: the other clock and the proof of what ran, in short)
                       "first_h2d_to_last_pdu_subframes_per_s": {"cold": h2d_cold, "warm": h2d_warm, "pcap_to_file_cold": leg_rate("host_pinned_pcap_to_file", "pass1_cold"),
                                                                 "pcap_to_file_warm": leg_rate("host_pinned_pcap_to_file", "pass3_warm")},
                       "pcap_diff": pcap_diff, "dist": dist_echo,
                       "parallelism": ("one capture, chunks round-robin over devices %s, shared sequential search" % devices) if capture_mode else "one cell per GPU, no collective"},
            "roofline": {"bound": "hbm", "kernel": la.KERNELS[kt], "achieved": round(ach, 2), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(ach / 8000.0, 6), "traffic": traffic, "traffic_source": traffic_src,
                         "avg_launch_ms": round(kms[kt] / max(1, klaunch[kt]), 4), "launches": int(klaunch[kt]),
                         "algo_bytes_per_launch": int(kbytes / max(1, klaunch[kt])), "timing": "HIP events on the launch streams inside the timed region (span of a launch that shares the GPU, not exclusive)",
                         # how many launches of this kernel are in flight on average (launches x mean span / timed region): the spans of concurrent launches
                         # stretch each other, so `frac` falls when the engine keeps more of them resident although the throughput rises
                         "mean_launches_in_flight": round(float(kms[kt]) / (dt * 1e3), 2),
                         "rocprof": rocprof, "dominant_by_time": la.KERNELS[dom], "valu": valu, "gpu_saturation": saturation, "profile": _profile_state()},
            "first_h2d_to_last_pdu": legs, "cold_state": cold, "cpu_baseline": cpu, "full": args.full, "dumped_outputs": dumped,
            "host": {"cpu_count": os.cpu_count(), "cpu_quota_cores": host_quota, "decode_threads": int(os.environ.get("LSN_DECODE_THREADS", "12")), "cores_busy_in_timed_region": round(host_cores_busy, 2), "cores_busy_per_rank": per_rank_cores,
                     "busiest_threads": busiest},
            "detail": {"pdus_per_subframe": round(p.nof_pdus / sf_rank, 3), "algo_bytes_per_subframe": int(p.algo_bytes / sf_rank),
                       "whole_path_GBps": round(p.algo_bytes * (1 if capture_mode else world) / 1e9 / dt, 2), "timed_region_s": round(dt, 3),
                       "per_6400_subframes": {k: round(getattr(p, k) * 6400.0 / sf_rank, 3) for k in
                                              ("nof_tb_decodes", "nof_cb_decodes", "nof_turbo_iterations", "nof_decode_jobs", "nof_decode_jobs_used", "nof_speculative_jobs", "nof_ondemand_decodes", "nof_candidate_misses", "ms_ondemand_commit", "ms_stage_a", "ms_search", "ms_search_core", "ms_rar", "ms_stage_c", "ms_commit", "ms_wait_front",
                                               "ms_wait_slot", "ms_drain")},
                       "decode_jobs_by_kind_per_6400": {"kinds": ["first attempt", "second table after failure", "second table speculative", "RA-RNTI ahead of search", "on demand"],
                                                        "jobs": [round(p.jobs_by_kind[k] * 6400.0 / sf_rank, 1) for k in range(5)], "jobs_unused": [round(p.jobs_unused_by_kind[k] * 6400.0 / sf_rank, 1) for k in range(5)],
                                                        "iterations": [round(p.iters_by_kind[k] * 6400.0 / sf_rank, 1) for k in range(5)], "iterations_unused": [round(p.iters_unused_by_kind[k] * 6400.0 / sf_rank, 1) for k in range(5)]},
                       # only a library built with -DLSN_TURBO_CYCLES fills these (tools/ab/): s_memtime ticks spent by the decoder's code blocks, per subframe
                       "turbo_clock_ticks_per_subframe": ({"load": round(p.turbo_cyc_rm / sf_rank, 1), "iterations": round(p.turbo_cyc_map / sf_rank, 1), "output": round(p.turbo_cyc_out / sf_rank, 1)}
                                                          if (p.turbo_cyc_rm or p.turbo_cyc_map) else None),
                       "table_hints_engine_total": {"used": int(p.nof_table_hints_used), "missed": int(p.nof_table_hints_missed)},
                       "ondemand_at_commit_per_6400": [round(p.nof_ondemand_commit[k] * 6400.0 / sf_rank, 2) for k in range(4)],
                       "kernel_ms_per_6400_subframes": {la.KERNELS[k]: round(kms[k] * 6400.0 / sf_rank, 4) for k in range(nk)},
                       "kernel_launches_per_step": {la.KERNELS[k]: round(float(klaunch[k]) / args.steps, 2) for k in range(nk)}},
        }
        # the last 1.5 kB of the line (what a tail keeps): every headline figure with its gate
        out["summary"] = {"value_resident": round(value, 1), "pcap_diff": pcap_diff, "timed_subframes": total_sf, "n_gpus": out["n_gpus"], "dist": dist_echo,
                          "first_h2d_to_last_pdu": {k: {"cold_warm_warm": [leg_rate(k, w) for w in ("pass1_cold", "pass2_warm", "pass3_warm")], "pcap_diff": leg_diffs(k)}
                                                    for k in ("host_pinned", "host_pinned_pcap_to_file", "host_pageable", "worker_pool_1_producer_thread", "worker_pool_4_producer_threads", "file_replay", "host_pinned_sc16", "file_replay_sc16")
                                                    if legs and k in legs},
                          "other_configs": {k: [v.get("subframes_per_s"), v.get("pcap_diff")] for k, v in (legs or {}).items() if isinstance(v, dict) and "what" in v},
                          "roofline_frac": out["roofline"]["frac"], "cpu_baseline": [cpu.get("value"), (cpu.get("configs0") or {}).get("value")] if cpu else None,
                          "host_cores_busy": round(host_cores_busy, 2)}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
