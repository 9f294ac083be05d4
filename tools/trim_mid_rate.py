#!/usr/bin/env python3
"""Rate of `trim`'s middle stage: synthetic reads, about one in a hundred a chimera with a front adapter in its middle, through
trim_reads(middle=True) on the GPU, stage by stage, and a sample of the same reads through the C++ model
(tests/native/trim_mid_model.cpp) on one core as the CPU yardstick.  Prints one JSON line.

    python tools/trim_mid_rate.py [--reads 100000] [--length 10000] [--model-reads 2000] [--no-model]

Not a gate."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--model-reads", type=int, default=2000)
    ap.add_argument("--front", default=os.path.join(ROOT, "tests", "golden", "trim", "adapters_front.fasta"))
    ap.add_argument("--back", default=os.path.join(ROOT, "tests", "golden", "trim", "adapters_back.fasta"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    import trim_rate
    from downpore_amd import trim as T
    from downpore_amd.overlap import Reads
    from tests import trim_cases as TC
    bases, off = trim_rate.make_reads(a.reads, a.length, a.front, a.back)
    rng = np.random.default_rng(2)
    fs = [np.frombuffer(s.encode(), dtype=np.uint8) for s in TC.read_fasta(a.front)[1]]
    b2 = bases.reshape(a.reads, a.length)
    chimeras = rng.choice(a.reads, size=max(1, a.reads // 100), replace=False)
    for i in chimeras:  # one of the few adapters make_reads plants at the ends, so that determination keeps it
        ad = fs[int(rng.integers(0, 8)) % len(fs)]
        at = int(rng.integers(a.length // 4, 3 * a.length // 4))
        b2[i, at:at + len(ad)] = ad
    F, B = Reads(fasta=a.front, min_len=0, himem=False), Reads(fasta=a.back, min_len=0, himem=False)
    out = {"reads": a.reads, "length": a.length, "chimeras": int(len(chimeras))}
    for label, determine in (("determine_on", True), ("determine_off", False)):
        reads = Reads(bases, off, min_len=50, himem=False)
        t0 = time.time()
        res = T.trim_reads(reads, F, B, determine_adapters=determine, middle=True, device=a.device)
        wall = time.time() - t0
        s = res.stats
        out[label] = {"wall_s": round(wall, 3), "front_adapters": int(s["front_adapters"]), "splits": int(len(res.splits)),
                      **{key: (round(s[key], 3) if key.endswith("_ms") else int(s[key])) for key in T.TRIM_MID_STAT_FIELDS},
                      "kernel_us_per_pair": round(1e3 * s["mid_kernel_ms"] / max(s["mid_pairs"], 1), 3)}
        res.close()
    if not a.no_model:
        from tests import trim_mid_model as MM
        n = min(a.model_reads, a.reads)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sample.fasta")
            with open(path, "wb") as f:
                for i in range(n):
                    f.write(b">r%07d\n" % i + b2[i].tobytes() + b"\n")
            MM.load()
            t0 = time.time()
            m = MM.run(path, a.front, a.back, determine_adapters=False)
            t_model = time.time() - t0
            out["model_one_core_determine_off"] = {"reads": n, "wall_s": round(t_model, 3), "candidate_pairs": m.counters["candidate_pairs"],
                                                   "us_per_pair": round(1e6 * t_model / max(m.counters["candidate_pairs"], 1), 3),
                                                   "note": "whole model run (edge + middle) on the first reads of the same input"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
