#!/usr/bin/env python3
"""What Mapper.map(raw, trim=...) saves a caller with a stream of raw, adapter-carrying batches against one reference.  In one process,
on one open mapper, every batch is run three ways, one after the other (two distinct raw read sets taking turns):

  (a) fused     m.map(raw, trim=...)                                   one upload, trim and cut on the device's copy
  (b) two_step  trim_reads(raw, ...) then m.map(res.reads(min_length))  what a caller could do before: the bases cross the link twice
  (c) oneshot   map_reads(ref, raw, trim=...)                           the reference set-up paid for every batch

Medians after the first batch, as bench.py takes them.  The three must agree on the PAF, and (a) and (c) on the stderr text (the run
stops otherwise).  The raw read sets are made outside the timed calls (a trim writes its flags into the set it ran on, so every call
gets a set of its own).  Prints one JSON line; --out writes it to a file too.

  --config 3      BASELINE config 3, the bench's `map` leg: 50 000 reads x 8 kb (10 % error), 4.6 Mb circular reference, k = 11
  --config share  the 375 Mb share of config 5 with 1 000 reads x 15 kb (10 % error), k = 13

Adapters (tests/golden/trim) are planted on three reads of four: both ends, the front alone, and one in the middle of every eighth."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"3": dict(genome=4600000, reads=50000, read_len=8000, error=0.1, seed=3, k=11),
           "share": dict(genome=375000000, reads=1000, read_len=15000, error=0.1, seed=5, k=13)}
MIN_LENGTH = 500
ADAPTERS = os.path.join(ROOT, "tests", "golden", "trim")


def fasta_seqs(path):
    return [ln.strip().encode() for ln in open(path) if ln.strip() and not ln.startswith(">")]


def raw_arrays(c):
    """two raw batches as (bases, offsets): synthetic reads with adapters planted"""
    from tools.synth import gen_genome, gen_reads
    genome = np.frombuffer(gen_genome(c["seed"], c["genome"]), dtype=np.uint8)
    bases, off = gen_reads(c["seed"], c["genome"], 2 * c["reads"], c["read_len"], c["error"], False)
    front = [np.frombuffer(s, dtype=np.uint8) for s in fasta_seqs(os.path.join(ADAPTERS, "adapters_front.fasta"))]
    back = [np.frombuffer(s, dtype=np.uint8) for s in fasta_seqs(os.path.join(ADAPTERS, "adapters_back.fasta"))]
    n = c["reads"]
    out = []
    for b in range(2):
        parts, lens = [], []
        for i in range(b * n, (b + 1) * n):
            r = bases[off[i]:off[i + 1]]
            if i % 8 == 3 and len(r) > 4000:
                h = len(r) // 2
                p = [r[:h], front[0], r[h:]]
            elif i % 4 == 0:
                p = [front[0], r, back[0]]
            elif i % 4 == 1:
                p = [front[0], r]
            else:
                p = [r]
            parts += p
            lens.append(sum(len(x) for x in p))
        out.append((np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)))
    return (genome, np.array([0, c["genome"]], dtype=np.int64)), out


def med_after_first(v):
    w = v[1:] if len(v) > 1 else v
    return statistics.median(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="3", choices=sorted(CONFIGS))
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--edges-only", action="store_true", help="the edge stage alone (default: with the middle stage)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    c = CONFIGS[a.config]
    from downpore_amd.mapping import Mapper, map_reads
    from downpore_amd.overlap import Reads
    from downpore_amd.trim import trim_reads
    (g, goff), raws = raw_arrays(c)
    ref = Reads(g, goff, min_len=0, himem=False)
    front = Reads(fasta=os.path.join(ADAPTERS, "adapters_front.fasta"), min_len=0, himem=False)
    back = Reads(fasta=os.path.join(ADAPTERS, "adapters_back.fasta"), min_len=0, himem=False)
    tkw = dict(k=6, middle=not a.edges_only)

    def raw(i):
        return Reads(raws[i % 2][0], raws[i % 2][1], min_len=50, himem=False)

    t0 = time.perf_counter()
    m = Mapper(ref, circular=True, k=c["k"], min_length=MIN_LENGTH)
    t_open = time.perf_counter() - t0
    rows = []
    for i in range(a.batches):
        ra, rb, rc = raw(i), raw(i), raw(i)
        t0 = time.perf_counter()
        fa = m.map(ra, trim=dict(front=front, back=back, **tkw))
        t1 = time.perf_counter()
        res = trim_reads(rb, front, back, **tkw)
        t1b = time.perf_counter()
        tb = m.map(res.reads(MIN_LENGTH, himem=False))
        t2 = time.perf_counter()
        oc = map_reads(ref, rc, circular=True, k=c["k"], min_length=MIN_LENGTH, trim=dict(front=front, back=back, **tkw))
        t3 = time.perf_counter()
        if fa[0] != oc[0] or fa[1] != oc[1]:
            sys.exit("batch %d: the mapper's text differs from map_reads(trim=...)'s" % i)
        if fa[0] != tb[0]:
            sys.exit("batch %d: the fused batch's PAF differs from the two steps'" % i)
        rows.append({"fused_wall_s": t1 - t0, "two_step_wall_s": t2 - t1, "two_step_trim_s": t1b - t1, "oneshot_wall_s": t3 - t2,
                     "fused_setup_s": fa[2]["t_setup_s"], "oneshot_setup_s": oc[2]["t_setup_s"], "paf_lines": fa[0].count("\n"),
                     "raw_bases": int(raws[i % 2][1][-1]), "trim_bytes_up": fa[2]["trim"].stats["bytes_up"]})
        res.close()
    m.close()
    med = {k: med_after_first([r[k] for r in rows]) for k in ("fused_wall_s", "two_step_wall_s", "two_step_trim_s", "oneshot_wall_s", "fused_setup_s", "oneshot_setup_s")}
    out = {"workload": "trim + map, config %s: raw batches of %d reads x %d bp (error %.2f, adapters planted) against a %d bp circular reference, k=%d, %s" %
                       (a.config, c["reads"], c["read_len"], c["error"], c["genome"], c["k"], "edge stage only" if a.edges_only else "edge and middle stage"),
           "batches": a.batches, "mapper_open_s": t_open, "medians_after_the_first": dict(
               med, fused_saves_against_two_step_s=med["two_step_wall_s"] - med["fused_wall_s"],
               fused_saves_against_oneshot_s=med["oneshot_wall_s"] - med["fused_wall_s"], fused_reads_per_s=c["reads"] / med["fused_wall_s"],
               two_step_reads_per_s=c["reads"] / med["two_step_wall_s"], oneshot_reads_per_s=c["reads"] / med["oneshot_wall_s"]),
           "text_identical": True, "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
