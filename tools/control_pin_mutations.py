#!/usr/bin/env python3
"""tools/control_pin_mutations.py - do the tests notice a misreading of the downlink control specifications that the transmitter and the oracle SHARE?
Each mutation is one such misreading, applied identically to tools/txgen/txgen.cc, to oracle/ and, where the constant lives there, to spec/lte_tables.h,
in scratch copies.  Two sets of CPU tests then run against the mutated libraries (a pytest plugin of this tool repoints tests/lsn_testlib at them):
  (a) the txgen loop-backs that touch the control region: tests/test_four_ports_oracle.py, tests/test_pbch_oracle.py, tests/test_extended_cp_oracle.py;
  (b) the spec-transmitter tests: tests/test_spec_control_oracle.py (tests/spec_downlink.py shares nothing with either side).
A loop-back passes a shared misreading by construction; (b) should fail on every one.  -> profiles/control_pin_mutations.txt"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX, PH, PB, PD, CV, FA, TB = "tools/txgen/txgen.cc", "oracle/o_phy.c", "oracle/o_pbch.c", "oracle/o_pdsch.c", "oracle/o_conv.c", "oracle/o_falcon.c", "spec/lte_tables.h"
REV16_CC = "[](uint32_t r) { uint32_t v = 0; for (int i = 0; i < 16; i++) v |= ((r >> i) & 1u) << (15 - i); return v; }(gr.rnti)"

# (what, [(file, old, new), ...]); every `old` occurs exactly once in its file
MUTATIONS = [
    ("PHICH REG offset floor(i n/3) read as floor(i (n+1)/3) (36.211 6.9.3)",
     [(TX, "(id + m + (i * na) / 3) % na", "(id + m + (i * (na + 1)) / 3) % na"),
      (PH, "((int)cell->id + mp + (i * navail) / 3) % navail", "((int)cell->id + mp + (i * (navail + 1)) / 3) % navail")]),
    ("PDCCH quadruplet cyclic shift by N_ID + 1 (36.211 6.8.5)",
     [(TX, "int q = perm[(mp + id) % M];", "int q = perm[(mp + id + 1) % M];"),
      (PH, "int q = perm[(mprime + (int)cell->id) % M];", "int q = perm[(mprime + (int)cell->id + 1) % M];")]),
    ("PCFICH k_bar from N_ID mod N_RB instead of mod 2 N_RB (36.211 6.7.4)",
     [(TX, "int kbar = 6 * (id % (2 * nprb));", "int kbar = 6 * (id % nprb);"),
      (PH, "int kbar = 6 * (int)(cell->id % (2u * (uint32_t)nprb));", "int kbar = 6 * (int)(cell->id % ((uint32_t)nprb));")]),
    ("PDCCH scrambling c_init with floor(ns/2) + 1 (36.211 6.8.2)",
     [(TX, "bits_t sc = gold(sf * 512u + id, (int)nbits);", "bits_t sc = gold((sf + 1) * 512u + id, (int)nbits);"),
      (PH, "o_gold(sf_idx * 512u + cell->id, c, (int)nbits);", "o_gold((sf_idx + 1u) * 512u + cell->id, c, (int)nbits);")]),
    ("DCI CRC RNTI mask in reversed bit order (x_rnti,0 = LSB; 36.212 5.3.3.2)",
     [(TX, "crc_attach(b, 0x11021, 16, gr.rnti);", "crc_attach(b, 0x11021, 16, " + REV16_CC + ");"),
      (CV, "uint16_t o_dci_decode(const float* llr, int E, int nof_bits, uint8_t* payload) { return o_dci_decode_off(llr, E, nof_bits, payload, 0); }",
       "uint16_t o_dci_decode(const float* llr, int E, int nof_bits, uint8_t* payload) { uint16_t r = o_dci_decode_off(llr, E, nof_bits, payload, 0), v = 0; "
       "for (int i = 0; i < 16; i++) v |= (uint16_t)(((r >> i) & 1u) << (15 - i)); return v; }")]),
    ("two entries of the convolutional sub-block permutation swapped (36.212 Table 5.1.4-2)",
     [(TB, "lsn_perm_cc[32] = {1,17,9,25,", "lsn_perm_cc[32] = {17,1,9,25,")]),
    ("SFBC: the sign of port 1 inverted (36.211 6.3.4.3)",
     [(TX, "p1[0] = -std::conj(x1) * s; p1[1] = std::conj(x0) * s;", "p1[0] = std::conj(x1) * s; p1[1] = -std::conj(x0) * s;"),
      (PH, "float t0r = a.r + b.r, t0i = a.i + b.i, t1r = d.r - c.r, t1i = d.i - c.i;", "float t0r = a.r - b.r, t0i = a.i - b.i, t1r = d.r + c.r, t1i = d.i + c.i;"),
      (PB, "float t0r = a.r + b.r, t0i = a.i + b.i, t1r = d.r - c.r, t1i = d.i - c.i;", "float t0r = a.r - b.r, t0i = a.i - b.i, t1r = d.r + c.r, t1i = d.i + c.i;"),
      (PD, "float t0r = a.r + b.r, t0i = a.i + b.i, t1r = d.r - cc.r, t1i = d.i - cc.i;", "float t0r = a.r - b.r, t0i = a.i - b.i, t1r = d.r + cc.r, t1i = d.i + cc.i;")]),
    ("PBCH four-port CRC mask inverted, 1010... instead of 0101... (36.212 Table 5.3.1.1-1)",
     [(TX, "(P == 2 ? 0xFFFFu : 0x5555u)", "(P == 2 ? 0xFFFFu : 0xAAAAu)"),
      (PB, "(mask == 0x5555 ? 4u : 0u)", "(mask == 0xAAAA ? 4u : 0u)")]),
    ("UE-specific search space: Y_k constant A = 39829 instead of 39827 (36.213 9.1.1)",
     [(TX, "Yk = (39827u * Yk) % 65537u;", "Yk = (39829u * Yk) % 65537u;"),
      (FA, "Yk = (39827u * Yk) % 65537u;", "Yk = (39829u * Yk) % 65537u;")]),
    ("PDCCH REG width: symbol 1 of a four-port cell read as 4-RE REGs (36.211 6.2.4)",
     [(TX, "int w = (l == 0 || (l == 1 && g->c.nof_ports == 4) || (l == 3 && g->c.cp)) ? 6 : 4;", "int w = (l == 0 || (l == 3 && g->c.cp)) ? 6 : 4;"),
      (PH, "return (l == 0 || (l == 1 && cell->nof_ports == 4) || (l == 3 && cell->cp)) ? 6 : 4;", "return (l == 0 || (l == 3 && cell->cp)) ? 6 : 4;")]),
]

PLUGIN = "control_pin_plugin"
LOOPBACK = ["tests/test_four_ports_oracle.py", "tests/test_pbch_oracle.py", "tests/test_extended_cp_oracle.py"]
SPEC = ["tests/test_spec_control_oracle.py"]


def _pytest(files, env):
    """-> (failed, passed) of one pytest run on the mutated libraries"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-p", PLUGIN, "-n", "8"] + files, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    tail = r.stdout.decode(errors="replace").strip().splitlines()[-1]
    got = {k: int(v) for v, k in re.findall(r"(\d+) (failed|passed|error)", tail)}
    return got.get("failed", 0) + got.get("error", 0), got.get("passed", 0)


def main():
    lines = ["shared misreadings of the control-region specifications, applied identically to txgen, the oracle and spec/lte_tables.h;",
             "(a) txgen loop-backs: " + ", ".join(LOOPBACK) + "    (b) " + ", ".join(SPEC), "",
             "%-2s  %-92s %-22s %s" % ("", "mutation", "(a) loop-backs", "(b) spec transmitter")]
    print("\n".join(lines), flush=True)
    for k, (what, edits) in enumerate(MUTATIONS):
        with tempfile.TemporaryDirectory() as tmp:
            for d in ("oracle", "spec", "tools/txgen"):
                shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, d), ignore=shutil.ignore_patterns("_build", "_ref"))
            for f, old, new in edits:
                p = os.path.join(tmp, f)
                src = open(p).read()
                assert src.count(old) == 1, (k, f, old, src.count(old))
                open(p, "w").write(src.replace(old, new))
            for d in ("oracle", "tools/txgen"):
                subprocess.check_call(["make", "-j8", "-C", os.path.join(tmp, d)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tools"), os.environ.get("PYTHONPATH", "")]),
                       LSN_MUTANT_ORACLE=os.path.join(tmp, "oracle", "_build", "liblsn_oracle.so"),
                       LSN_MUTANT_TXGEN=os.path.join(tmp, "tools", "txgen", "_build", "libtxgen.so"))
            a, b = _pytest(LOOPBACK, env), _pytest(SPEC, env)
        line = "%2d  %-92s %-22s %s" % (k, what, "%d of %d fail" % (a[0], sum(a)), ("%d of %d fail" % (b[0], sum(b))) + ("" if b[0] else "  <-- NOT NOTICED"))
        print(line, flush=True)
        lines.append(line)
    open(os.path.join(ROOT, "profiles", "control_pin_mutations.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
