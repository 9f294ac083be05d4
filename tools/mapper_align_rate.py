#!/usr/bin/env python3
"""What the NM and cg tags of Mapper.map_aligned cost a batch.  In one process, on one open mapper, every batch is mapped both ways,
one after the other - m.map(reads), then m.map_aligned(reads) - over two read sets taking turns.  Medians after the first batch, as
bench.py takes them.  The aligned text without its tags must be the plain text (the run stops otherwise).  Prints one JSON line; --out
writes it to a file too.

  --config 3      BASELINE config 3, the bench's `map` leg: 50 000 reads x 8 kb (10 % error), 4.6 Mb circular reference, k = 11
  --config share  the 375 Mb share of config 5 with 1 000 reads x 15 kb (10 % error), k = 13

--reads N maps N reads per batch instead of the configuration's (the JSON says so)."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"3": dict(genome=4600000, reads=50000, read_len=8000, error=0.1, seed=3, k=11),
           "share": dict(genome=375000000, reads=1000, read_len=15000, error=0.1, seed=5, k=13)}
MIN_LENGTH = 500
TAGS = re.compile(r"\tNM:i:\d+\tcg:Z:[0-9MID]+$", flags=re.M)


def med_after_first(v):
    w = v[1:] if len(v) > 1 else v
    return statistics.median(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="3", choices=sorted(CONFIGS))
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--max-edits", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    c = dict(CONFIGS[a.config])
    if a.reads:
        c["reads"] = a.reads
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    from tools.synth import gen_genome, gen_reads
    genome = np.frombuffer(gen_genome(c["seed"], c["genome"]), dtype=np.uint8)
    bases, off = gen_reads(c["seed"], c["genome"], 2 * c["reads"], c["read_len"], c["error"], False)
    n = c["reads"]
    sets = [Reads(np.array(bases[off[b * n]:off[(b + 1) * n]]), (off[b * n:(b + 1) * n + 1] - off[b * n]).astype(np.int64), min_len=MIN_LENGTH,
                  himem=False) for b in range(2)]
    ref = Reads(genome, np.array([0, c["genome"]], dtype=np.int64), min_len=0, himem=False)
    t0 = time.perf_counter()
    m = Mapper(ref, circular=True, k=c["k"], min_length=MIN_LENGTH)
    t_open = time.perf_counter() - t0
    rows = []
    for i in range(a.batches):
        reads = sets[i % 2]
        t0 = time.perf_counter()
        plain = m.map(reads)
        t1 = time.perf_counter()
        al = m.map_aligned(reads, max_edits=a.max_edits)
        t2 = time.perf_counter()
        if TAGS.sub("", al[0]) != plain[0] or al[1] != plain[1]:
            sys.exit("batch %d: the aligned text without its tags differs from the plain text" % i)
        s = al[2]["align"]
        rows.append(dict(map_wall_s=t1 - t0, map_aligned_wall_s=t2 - t1, align_kernel_s=1e-6 * s["kernel_us"], **s))
    m.close()
    med = {k: med_after_first([r[k] for r in rows]) for k in ("map_wall_s", "map_aligned_wall_s", "align_kernel_s", "cells", "traceback_bytes")}
    med["dp_cells_per_s"] = med["cells"] / med["align_kernel_s"] if med["align_kernel_s"] > 0 else None
    med["kernel_share_of_the_aligned_batch"] = med["align_kernel_s"] / med["map_aligned_wall_s"]
    out = {"workload": "map against map_aligned, config %s: batches of %d reads x %d bp (error %.2f) against a %d bp circular reference, k=%d, max_edits=%d" %
                       (a.config, c["reads"], c["read_len"], c["error"], c["genome"], c["k"], a.max_edits),
           "batches": a.batches, "mapper_open_s": t_open, "medians_after_the_first": med, "text_identical_without_tags": True, "rows": rows}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
