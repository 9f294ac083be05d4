#!/usr/bin/env python3
"""map_reads(trim=...) - the trim in front of `map` on one upload - against the library's two steps
map_reads(ref, trim_reads(raw, ...).reads(min_length), ...), both from this build, on tools/overlap_trim_rate.py's seeded input (reads
drawn from one genome, adapters planted at the ends of about half of them and in the centre of about one in a hundred), mapped against
the genome they were drawn from.  The two forms run alternately in one call (one warm-up pair, then --pairs pairs), every run in a
process of its own under a time limit of its own; a run that fails or runs out of time ends the call, nothing is started after it.
Every run is listed with its stages - the fused run's from the library's [map setup] marks (DPH_PROFILE) - and the medians and ranges are
compared; the PAF of the two forms must be identical.  --parent-lib DIR: every pair gets a third run, the two steps with the two libraries of another build
(the parent commit's: make -C downpore_amd/csrc LIB=DIR hip host-lib in a checkout of it), so that the parent's own figure is measured in
the same call.  Prints one JSON document.

    python tools/map_trim_rate.py [--reads 100000] [--length 10000] [--k 11] [--pairs 5] [--out profiles/trim/map_trim.json]
                                  [--rocprof DIR] [--parent-lib DIR]

Not a gate: profiles/trim/map_trim.json is one recorded run."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRONT = os.path.join(ROOT, "tests", "golden", "trim", "adapters_front.fasta")
BACK = os.path.join(ROOT, "tests", "golden", "trim", "adapters_back.fasta")
MIN_LENGTH = 500


def child(a):
    """one run of one form; prints its JSON line"""
    from downpore_amd import trim as T
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    t = [time.perf_counter()]

    def lap():
        t.append(time.perf_counter())
        return round(t[-1] - t[-2], 4)

    front, back = Reads(fasta=FRONT, min_len=0, himem=False), Reads(fasta=BACK, min_len=0, himem=False)
    ref = Reads(fasta=a.ref, min_len=0, himem=False)
    raw = Reads(fasta=a.input, min_len=50, himem=False)
    out = {"read_input_s": lap()}
    kw = dict(k=6, middle=bool(a.middle))
    if a.child == "fused":
        paf, err, st = map_reads(ref, raw, trim=dict(front=front, back=back, **kw), k=a.k, min_length=MIN_LENGTH)
        out["map_reads_s"] = lap()
        trimmed = st["trim"].reads(MIN_LENGTH, himem=False)
        out["trim_bytes_up"] = st["trim"].stats["bytes_up"]
    else:
        res = T.trim_reads(raw, front, back, **kw)
        out["trim_reads_s"] = lap()
        out["trim_write_s"] = round(res.stats["t_write_s"], 4)
        out["trim_bytes_up"] = res.stats["bytes_up"]
        trimmed = res.reads(MIN_LENGTH, himem=False)
        out["trimmed_read_set_s"] = lap()
        paf, err, st = map_reads(ref, trimmed, k=a.k, min_length=MIN_LENGTH)
        out["map_reads_s"] = lap()
    out["wall_s"] = round(t[-1] - t[0], 4)
    out["run_s"] = round(out["wall_s"] - out["read_input_s"], 4)  # without reading the files, which both forms do alike
    out.update(paf_sha256=hashlib.sha256(paf.encode()).hexdigest(), paf_lines=paf.count("\n"), trimmed_reads=len(trimmed),
               trimmed_bases=int(trimmed.total_bases()), raw_bases=int(raw.total_bases()),
               map_setup_s=round(st["t_setup_s"], 4), map_loop_s=round(st["t_scan_s"] + st["t_chain_s"] + st["t_host_s"], 4))
    print(json.dumps(out))


def marks(stderr):
    """the [map setup] marks of a DPH_PROFILE run, in ms, by name (repeated names add up)"""
    out = {}
    for m in re.finditer(r"^\[map setup\] (.+?)\s+([0-9.]+) ms$", stderr, flags=re.M):
        out[m.group(1).strip()] = round(out.get(m.group(1).strip(), 0.0) + float(m.group(2)), 2)
    return out


def run_child(form, a, paths, env, limit, prefix=()):
    # the limit is `timeout`'s, in front of everything: it puts the command into a process group of its own and signals the whole group,
    # so the run itself ends also where a profiler stands between this process and it (-k: killed if the first signal does not end it)
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", form, "--input", paths[0],
                                                              "--ref", paths[1], "--k", str(a.k), "--middle", str(a.middle)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit + 60)
    if r.returncode != 0:
        raise SystemExit("the %s run failed (%d); nothing more is started: %s" % (form, r.returncode, r.stderr.decode()[-1500:]))
    doc = json.loads(r.stdout.decode().strip().splitlines()[-1])
    doc["marks_ms"] = marks(r.stderr.decode())
    return doc


def kernel_times(d, a, paths, env, limit):
    """calls and time of the kernels of the fused form, from one profiler run of it alone (kernel trace only, no counters)"""
    import csv
    import glob
    os.makedirs(d, exist_ok=True)
    doc = run_child("fused", a, paths, env, limit, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fused", "--"])
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
            if name in ("repack_spans_rc_kernel", "place_packed_kernel", "unpack_spans_kernel", "span_offsets_kernel", "trim_edge_kernel",
                        "trim_mid_kernel") or name.startswith("chunk_scan_kernel"):
                try:
                    out[name] = {"calls": int(col(row, "calls")), "total_ms": round(col(row, "duration") / 1e6, 4),
                                 "min_ms": round(col(row, "min") / 1e6, 4), "max_ms": round(col(row, "max") / 1e6, 4)}
                except KeyError as e:
                    out[name] = {"error": str(e)}
    k = out.get("repack_spans_rc_kernel")
    if k and "total_ms" in k and k["total_ms"] > 0:
        # per base of a paired read: 0.25 bytes read, 0.5 written (both strands); the unpaired reference and join chunks are left out
        traffic = 0.75 * doc["trimmed_bases"]
        k["bytes_of_paired_reads"] = int(traffic)
        k["share_of_8_TB_per_s"] = round(traffic / (k["total_ms"] * 1e-3) / 8e12, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--middle", type=int, default=1)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--limit", type=int, default=240, help="seconds one run may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--rocprof", default="", help="a directory: one more fused run under rocprofv3 --kernel-trace --stats, on its own, for the kernels' times")
    ap.add_argument("--parent-lib", default="", help="a directory with libdownpore_hip.so and libdownpore_host.so of the parent commit's build: a third run per pair, the two steps with it")
    ap.add_argument("--child", default="", choices=["", "fused", "two_steps"])
    ap.add_argument("--input", default="")
    ap.add_argument("--ref", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    from overlap_trim_rate import make_input
    from tests import oracle_lib as O
    env = dict(os.environ, DPH_PROFILE="1")
    env.pop("DP_LIB_DIR", None)
    env.pop("DPH_HOST_LIB", None)
    d = tempfile.mkdtemp(prefix="map_trim_", dir=a.tmp if os.path.isdir(a.tmp) else None)
    paths = (os.path.join(d, "reads.fasta"), os.path.join(d, "ref.fasta"))
    t0 = time.time()
    n_ends, n_centres = make_input(paths[0], a.reads, a.length, a.seed)
    genome = max(100000, a.reads * a.length // 10)
    with open(paths[1], "wb") as f:
        f.write(b">genome\n" + bytes(O.gen_genome(a.seed, genome)) + b"\n")
    doc = {"reads": a.reads, "length": a.length, "genome": genome, "k": a.k, "middle": bool(a.middle), "min_length": MIN_LENGTH,
           "reads_with_end_adapters": n_ends, "reads_with_a_centre_adapter": n_centres, "generate_s": round(time.time() - t0, 2),
           "input_bytes": os.path.getsize(paths[0]), "fused": [], "two_steps": [], "two_steps_parent_build": []}
    try:
        for i in range(a.pairs + 1):
            fused = run_child("fused", a, paths, env, a.limit)
            two = run_child("two_steps", a, paths, env, a.limit)
            if a.parent_lib:
                old = run_child("two_steps", a, paths, dict(env, DP_LIB_DIR=os.path.abspath(a.parent_lib)), a.limit)
                assert old["paf_sha256"] == two["paf_sha256"], "the parent build's two steps print different PAF"
                if i:
                    doc["two_steps_parent_build"].append(old)
            assert fused["paf_sha256"] == two["paf_sha256"] and fused["paf_lines"] > 0, "the two forms print different PAF"
            if i:  # (the first pair warms the page cache, the driver and the block caches)
                doc["fused"].append(fused)
                doc["two_steps"].append(two)
        if a.rocprof:
            doc["kernels"] = kernel_times(a.rocprof, a, paths, env, 2 * a.limit)
    finally:
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(d)
    doc["paf_identical"] = True
    for form in ("fused", "two_steps") + (("two_steps_parent_build",) if a.parent_lib else ()):
        for key in ("wall_s", "run_s"):
            v = [x[key] for x in doc[form]]
            doc["%s_%s" % (form, key)] = {"median": round(statistics.median(v), 4), "min": min(v), "max": max(v)}
    names = sorted(set(n for x in doc["fused"] for n in x["marks_ms"]))
    doc["fused_marks_ms"] = {n: {"median": round(statistics.median(x["marks_ms"].get(n, 0.0) for x in doc["fused"]), 2),
                                 "min": min(x["marks_ms"].get(n, 0.0) for x in doc["fused"]),
                                 "max": max(x["marks_ms"].get(n, 0.0) for x in doc["fused"])} for n in names}
    doc["fused_at_or_below_two_steps"] = doc["fused_run_s"]["median"] <= doc["two_steps_run_s"]["median"]
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
