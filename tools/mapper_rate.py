#!/usr/bin/env python3
"""What a Mapper saves: N batches through one downpore_amd.mapping.Mapper against N map_reads calls on the same batches, alternating in
one process (two distinct read sets taking turns), medians after the first as bench.py takes them.  Every batch's PAF and stderr text
through the mapper must be map_reads' (the run stops otherwise).  Prints one JSON line; --out writes it to a file too.

  --config 3      BASELINE config 3, the bench's `map` leg: 50 000 reads x 8 kb (10 % error), 4.6 Mb circular reference, k = 11
  --config share  the 375 Mb share of config 5 with 1 000 reads x 15 kb (10 % error), k = 13

--parent DIR: also map_reads alone, in processes of their own, alternating between this tree and the tree at DIR (a build of the parent
commit) --reps times on this box: boxes differ by 10 %, so only such an alternation says whether map_reads itself got slower."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"3": dict(genome=4600000, reads=50000, read_len=8000, error=0.1, seed=3, k=11),
           "share": dict(genome=375000000, reads=1000, read_len=15000, error=0.1, seed=5, k=13)}


def inputs(c):
    from tools.synth import gen_genome, gen_reads
    from downpore_amd.overlap import Reads
    genome = np.frombuffer(gen_genome(c["seed"], c["genome"]), dtype=np.uint8)
    goff = np.array([0, c["genome"]], dtype=np.int64)
    bases, off = gen_reads(c["seed"], c["genome"], 2 * c["reads"], c["read_len"], c["error"], False)
    n = c["reads"]
    sets = [Reads(bases[off[0]:off[n]], off[:n + 1] - off[0], min_len=500, himem=False),
            Reads(bases[off[n]:off[2 * n]], off[n:] - off[n], min_len=500, himem=False)]
    return Reads(genome, goff, min_len=0, himem=False), sets


def med_after_first(v):
    w = v[1:] if len(v) > 1 else v
    return statistics.median(w)


def oneshot_only(c, n):
    """worker of --parent: n map_reads calls in this process's tree, wall seconds of each"""
    from downpore_amd.mapping import map_reads
    ref, sets = inputs(c)
    walls = []
    for i in range(n):
        t0 = time.perf_counter()
        paf, err, st = map_reads(ref, sets[i % 2], circular=True, k=c["k"])
        walls.append(time.perf_counter() - t0)
    print(json.dumps({"walls": walls, "lines": paf.count("\n")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="3", choices=sorted(CONFIGS))
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--oneshot-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, os.getcwd() if a.oneshot_worker else ROOT)
    c = CONFIGS[a.config]
    if a.oneshot_worker:
        return oneshot_only(c, a.batches)
    from downpore_amd.mapping import Mapper, map_reads
    ref, sets = inputs(c)
    t0 = time.perf_counter()
    m = Mapper(ref, circular=True, k=c["k"])
    t_open = time.perf_counter() - t0
    rows = []
    for i in range(a.batches):
        reads = sets[i % 2]
        t0 = time.perf_counter()
        mp = m.map(reads)
        t1 = time.perf_counter()
        op = map_reads(ref, reads, circular=True, k=c["k"])
        t2 = time.perf_counter()
        if mp[0] != op[0] or mp[1] != op[1]:
            sys.exit("batch %d: the mapper's text differs from map_reads'" % i)
        rows.append({"mapper_wall_s": t1 - t0, "oneshot_wall_s": t2 - t1, "mapper_setup_s": mp[2]["t_setup_s"], "oneshot_setup_s": op[2]["t_setup_s"],
                     "paf_lines": mp[0].count("\n")})
    m.close()
    mw, ow = med_after_first([r["mapper_wall_s"] for r in rows]), med_after_first([r["oneshot_wall_s"] for r in rows])
    ms, os_ = med_after_first([r["mapper_setup_s"] for r in rows]), med_after_first([r["oneshot_setup_s"] for r in rows])
    out = {"workload": "map, config %s: batches of %d reads x %d bp (error %.2f) against a %d bp circular reference, k=%d" %
                       (a.config, c["reads"], c["read_len"], c["error"], c["genome"], c["k"]),
           "batches": a.batches, "mapper_open_s": t_open, "medians_after_the_first": {
               "mapper_batch_wall_s": mw, "oneshot_wall_s": ow, "saved_s": ow - mw, "mapper_reads_per_s": c["reads"] / mw, "oneshot_reads_per_s": c["reads"] / ow,
               "oneshot_setup_s": os_, "mapper_batch_setup_s": ms, "expected_saving_s": os_ - ms, "shortfall_s": (os_ - ms) - (ow - mw)},
           "text_identical": True, "rows": rows}
    if a.parent:
        res = {"parent": [], "this": []}
        for _ in range(a.reps):
            for label, d in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", a.config, "--batches", str(a.batches), "--oneshot-worker"], cwd=d,
                                   capture_output=True, text=True, timeout=1500)
                if p.returncode != 0:
                    sys.exit("%s: %s" % (label, p.stderr[-2000:]))
                res[label].append(json.loads(p.stdout.strip().splitlines()[-1])["walls"])
        med = {k: [med_after_first(w) for w in v] for k, v in res.items()}
        out["map_reads_against_parent"] = {"medians_after_the_first_per_process_s": med, "median_of_them_s": {k: statistics.median(v) for k, v in med.items()},
                                           "spread_of_the_parents_own_s": max(med["parent"]) - min(med["parent"]), "walls_s": res}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
