#!/usr/bin/env python3
"""Rate of the `trim` edge stage: synthetic reads with planted adapters through the product on the GPU, stage by stage, and the
same read ends through the C++ model (tests/native/trim_model.cpp) on one core as the CPU yardstick.  Prints one JSON line.

    python tools/trim_rate.py [--reads 100000] [--length 10000] [--front F.fasta --back B.fasta] [--no-model]

Not a gate: profiles/trim/edge_rate.json is one recorded run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_reads(n, length, front, back, seed=1):
    """n reads of `length` bases cut from a random pool; three in four carry a front and a back adapter (a tenth of them with
    5 % substitutions) inside their first / last 150 bases."""
    from tests import trim_cases as TC
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(TC.random_bases(seed, 32 << 20).encode(), dtype=np.uint8)
    bases = np.empty(n * length, dtype=np.uint8)
    starts = rng.integers(0, len(pool) - length, size=n)
    fs = [np.frombuffer(s.encode(), dtype=np.uint8) for s in TC.read_fasta(front)[1]]
    bs = [np.frombuffer(s.encode(), dtype=np.uint8) for s in TC.read_fasta(back)[1]]
    pick = rng.integers(0, 8, size=n)  # a few adapters dominate, as in a real run
    for i in range(n):
        r = bases[i * length:(i + 1) * length]
        r[:] = pool[starts[i]:starts[i] + length]
        if i % 4 == 3:
            continue
        for ad, at in ((fs[pick[i] % len(fs)], int(rng.integers(0, 60))), (bs[pick[i] % len(bs)], length - 150 + int(rng.integers(40, 90)))):
            a = ad.copy()
            if i % 10 == 0:
                m = rng.random(len(a)) < 0.05
                a[m] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(m.sum()))]
            r[at:at + len(a)] = a
    off = np.arange(n + 1, dtype=np.int64) * length
    return bases, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--front", default=os.path.join(ROOT, "tests", "golden", "trim", "adapters_front.fasta"))
    ap.add_argument("--back", default=os.path.join(ROOT, "tests", "golden", "trim", "adapters_back.fasta"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    from downpore_amd import trim as T
    from downpore_amd.overlap import Reads
    t0 = time.time()
    bases, off = make_reads(a.reads, a.length, a.front, a.back)
    t_gen = time.time() - t0
    reads = Reads(bases, off, min_len=50, himem=False)
    F, B = Reads(fasta=a.front, min_len=0, himem=False), Reads(fasta=a.back, min_len=0, himem=False)
    H = T._host()
    out = {"reads": a.reads, "length": a.length, "ends": 2 * a.reads, "generate_s": round(t_gen, 3)}
    for label, determine in (("determine_off", False), ("determine_on", True)):
        p = T._params(6, 10000, 90, 5, True, False, determine, 1)
        t0 = time.time()
        h = H.dph_trim_run(reads.h, F.h, B.h, p.ctypes.data, len(p), a.device)
        wall = time.time() - t0
        if not h:
            raise SystemExit("dph_trim_run: " + H.dph_last_error(None).decode())
        st = np.zeros(16, dtype=np.float64)
        H.dph_trim_stats(h, st.ctypes.data)
        n = C.c_int64(0)
        H.dph_trim_output(h, C.byref(n))
        H.dph_trim_free(h)
        s = dict(zip(T.TRIM_STAT_FIELDS, st.tolist()))
        ends = 2 * s["seen"]
        run = {"wall_s": round(wall, 4), "end_extraction_s": round(s["t_extract_s"], 4), "upload_ms": round(s["upload_ms"], 3),
               "kernel_ms": round(s["kernel_ms"], 3), "download_ms": round(s["download_ms"], 3), "host_apply_s": round(s["t_apply_s"], 4),
               "write_s": round(s["t_write_s"], 4), "determine_s": round(s["t_determine_s"], 4),
               "determine_kernel_ms": round(s["determine_kernel_ms"], 3), "adapters": int(s["front_adapters"] + s["back_adapters"]),
               "output_bytes": int(n.value), "bytes_up_per_end": s["bytes_up"] / max(ends, 1), "bytes_down_per_end": s["bytes_down"] / max(ends, 1),
               "kernel_ns_per_end": round(1e6 * s["kernel_ms"] / max(ends, 1), 2),
               "kernel_gb_per_s": round((s["bytes_up"] + s["bytes_down"]) / max(s["kernel_ms"], 1e-9) / 1e6, 3)}
        out[label] = run
    if not a.no_model:
        # the same ends on one core: reads made of their two ends alone are read sets with exactly these ends
        import tempfile
        from tests import trim_model as M
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "ends.fasta")
            b2 = bases.reshape(a.reads, a.length)
            with open(path, "wb") as f:
                for i in range(a.reads):
                    f.write(b">r%07d\n" % i + b2[i, :150].tobytes() + b2[i, -150:].tobytes() + b"\n")
            M.load()
            t0 = time.time()
            m = M.run(path, a.front, a.back, determine_adapters=False)
            t_model = time.time() - t0
            out["model_one_core"] = {"wall_s": round(t_model, 3), "ns_per_end": round(1e9 * t_model / max(len(m.recs), 1), 1),
                                     "ends": int(len(m.recs)), "note": "whole model run on 300-base reads: parse, match, apply, write"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
