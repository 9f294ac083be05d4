#!/usr/bin/env python3
"""`overlap -trim true` against `trim > file; overlap -input file`, both from this build, on one seeded input of BASELINE config 2's
shape: reads drawn from one genome, adapters planted at the ends of about half of them and in the centre of about one in a hundred.
The two forms run alternately in one call (one warm-up pair, then --pairs pairs); every run is listed with its per-stage marks
(DPH_PROFILE) and the medians are compared.  The intermediate file lies on tmpfs.  Prints one JSON document.

    python tools/overlap_trim_rate.py [--reads 100000] [--length 10000] [--k 13] [--pairs 5] [--out profiles/trim/overlap_trim.json]

Not a gate: profiles/trim/overlap_trim.json is one recorded run."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "downpore_amd", "bin", "downpore")
FRONT = os.path.join(ROOT, "tests", "golden", "trim", "adapters_front.fasta")
BACK = os.path.join(ROOT, "tests", "golden", "trim", "adapters_back.fasta")


def make_input(path, n, length, seed):
    """n reads of `length` bases from one genome (~ 10x coverage); returns (reads with end adapters, reads with a centre adapter)"""
    from tests import oracle_lib as O
    from tests import trim_cases as TC
    rng = np.random.default_rng(seed)
    bases, off = O.gen_reads(seed, max(100000, n * length // 10), n, length, 0.0, False)
    bases = bases.copy()
    fn, fs = TC.read_fasta(FRONT)
    bn, bs = TC.read_fasta(BACK)
    both = [x for x in fn if x in bn][:6]  # a few adapters dominate, as in a real run
    F = [np.frombuffer(fs[fn.index(x)].encode(), dtype=np.uint8) for x in both]
    B = [np.frombuffer(bs[bn.index(x)].encode(), dtype=np.uint8) for x in both]
    ends = centres = 0
    for i in range(n):
        r = bases[off[i]:off[i + 1]]
        a = int(rng.integers(0, len(both)))
        if i % 2 == 0:
            at = int(rng.integers(0, 60))
            r[at:at + len(F[a])] = F[a]
            at = len(r) - 150 + int(rng.integers(40, 90))
            r[at:at + len(B[a])] = B[a]
            ends += 1
        if i % 100 == 37:
            at = len(r) // 2
            r[at:at + len(F[a])] = F[a]
            centres += 1
    with open(path, "wb") as f:
        for i in range(n):
            f.write(b">r%07d\n" % i)
            f.write(bases[off[i]:off[i + 1]].tobytes())
            f.write(b"\n")
    return ends, centres


def marks(stderr):
    """the [cli] / [setup] stage marks of a DPH_PROFILE run, in ms, by name (repeated names add up)"""
    out = {}
    for m in re.finditer(r"^\[(cli|setup)\] (.+?)\s+([0-9.]+) ms$", stderr, flags=re.M):
        key = m.group(1) + ": " + m.group(2).strip()
        out[key] = round(out.get(key, 0.0) + float(m.group(3)), 2)
    return out


def kernel_times(d, cmd, env):
    """calls and time of the kernels the fused form adds, from a profiler run of the fused command alone"""
    import csv
    import glob
    os.makedirs(d, exist_ok=True)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fused", "--"] + cmd, env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
    if r.returncode != 0:
        return {"error": r.stderr.decode()[-500:]}
    out = {}

    def col(row, *words):  # (the column names differ between profiler versions: "Duration (Nsec)" / "TotalDurationNs")
        for key in row:
            if all(w in key.lower() for w in words):
                return float(row[key])
        raise KeyError("%s among %s" % (words, list(row)))

    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0]
            if name.startswith("void "):
                name = name[5:]
            if name in ("unpack_spans_kernel", "repack_spans_kernel", "span_offsets_kernel", "pack_kernel", "trim_edge_kernel", "trim_mid_kernel") or name.startswith("chunk_scan_kernel"):
                try:
                    out[name] = {"calls": int(col(row, "calls")), "total_ms": round(col(row, "duration") / 1e6, 4),
                                 "min_ms": round(col(row, "min") / 1e6, 4), "max_ms": round(col(row, "max") / 1e6, 4)}
                except KeyError as e:
                    out[name] = {"error": str(e)}
    return out


def run(cmd, env, stdout=None):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, stdout=stdout if stdout is not None else subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (" ".join(cmd[:3]), r.returncode, r.stderr.decode()[-1500:]))
    return wall, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--k", type=int, default=13)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--middle", type=int, default=1)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out", default="")
    ap.add_argument("--rocprof", default="", help="a directory: one more fused run under rocprofv3 --kernel-trace --stats, on its own, for the two kernels' times")
    a = ap.parse_args()
    env = dict(os.environ, DPH_PROFILE="1")
    env.pop("DP_TRIM_MIDDLE", None)
    if a.middle:
        env["DP_TRIM_MIDDLE"] = "1"
    d = tempfile.mkdtemp(prefix="overlap_trim_", dir=a.tmp if os.path.isdir(a.tmp) else None)
    src, mid = os.path.join(d, "reads.fasta"), os.path.join(d, "trimmed.fasta")
    t0 = time.time()
    n_ends, n_centres = make_input(src, a.reads, a.length, a.seed)
    doc = {"reads": a.reads, "length": a.length, "k": a.k, "middle": bool(a.middle), "reads_with_end_adapters": n_ends,
           "reads_with_a_centre_adapter": n_centres, "generate_s": round(time.time() - t0, 2), "input_bytes": os.path.getsize(src),
           "fused": [], "two_commands": []}
    ads = ["-front_adapters", FRONT, "-back_adapters", BACK]
    sha = {}
    try:
        for i in range(a.pairs + 1):
            wall, r = run([CLI, "overlap", "-input", src, "-trim", "true", "-k", str(a.k)] + ads, env)
            sha["fused"] = hashlib.sha256(r.stdout).hexdigest()
            fused = {"wall_s": round(wall, 4), "paf_bytes": len(r.stdout), "marks_ms": marks(r.stderr.decode())}
            with open(mid, "wb") as f:
                w1, r1 = run([CLI, "trim", "-input", src] + ads, env, stdout=f)
            w2, r2 = run([CLI, "overlap", "-input", mid, "-k", str(a.k)], env)
            sha["two_commands"] = hashlib.sha256(r2.stdout).hexdigest()
            two = {"wall_s": round(w1 + w2, 4), "trim_s": round(w1, 4), "overlap_s": round(w2, 4), "file_bytes": os.path.getsize(mid),
                   "marks_ms": marks(r2.stderr.decode())}
            if i:  # (the first pair warms the page cache, the driver and the block caches)
                doc["fused"].append(fused)
                doc["two_commands"].append(two)
        if a.rocprof:
            doc["kernels"] = kernel_times(a.rocprof, [CLI, "overlap", "-input", src, "-trim", "true", "-k", str(a.k)] + ads, env)
    finally:
        for p in (src, mid):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(d)
    doc["stdout_identical"] = sha["fused"] == sha["two_commands"]
    doc["median_fused_s"] = round(statistics.median(x["wall_s"] for x in doc["fused"]), 4)
    doc["median_two_commands_s"] = round(statistics.median(x["wall_s"] for x in doc["two_commands"]), 4)
    doc["fused_at_or_below_two_commands"] = doc["median_fused_s"] <= doc["median_two_commands_s"]
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
