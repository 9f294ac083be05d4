"""Inputs of the `trim` tests: a seeded generator of reads with the fixture adapters and barcodes planted at their ends (random
bases from tools/libdpsynth.so), FASTA / FASTQ writers, and the classes a read or a read end falls into on the model's output."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trim")
FRONT = os.path.join(GOLDEN, "adapters_front.fasta")
BACK = os.path.join(GOLDEN, "adapters_back.fasta")
EDGE = 150

CLASSES = ["found_front", "found_back", "best_is_barcode", "ambiguous", "pair_mismatch", "ignored", "trimmed_without_found",
           "no_prefilter_pass", "skipped_short"]


def read_fasta(path):
    names, seqs = [], []
    for ln in open(path):
        ln = ln.rstrip("\n")
        if ln.startswith(">"):
            names.append(ln[1:].strip())
        elif ln:
            seqs.append(ln)
    return names, seqs


def write_fasta(path, names, seqs, quals=None):
    with open(path, "w") as f:
        for i, (n, s) in enumerate(zip(names, seqs)):
            if quals is None:
                f.write(">%s\n%s\n" % (n, s))
            else:
                f.write("@%s\n%s\n+\n%s\n" % (n, s, quals[i]))


def random_bases(seed, n):
    so = C.CDLL(os.path.join(ROOT, "tools", "libdpsynth.so"))
    so.dps_genome.argtypes = [C.c_uint64, C.c_int64, C.c_char_p]
    buf = C.create_string_buffer(n + 1)
    so.dps_genome(seed, n, buf)
    return buf.raw[:n].decode()


def mutate(rng, s, rate):
    """Substitutions and indels at `rate` per base, a third each."""
    if rate <= 0:
        return s
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append("ACGT"[rng.integers(4)])          # substitution (may repeat the base)
        elif r < 2 * rate / 3:
            continue                                      # deletion
        elif r < rate:
            out.append(c)
            out.append("ACGT"[rng.integers(4)])          # insertion
        else:
            out.append(c)
    return "".join(out)


def plant(read, at, what):
    at = max(0, min(at, len(read) - len(what)))
    return read[:at] + what + read[at + len(what):]


def generate(seed, n_reads, fastq=False):
    """-> names, seqs, quals (or None), truth: per read a dict of what was planted (front / back = (adapter name, offset from the
    read's start / offset of the adapter's start inside the last 150 bases, error rate))."""
    rng = np.random.default_rng(seed)
    fn, fs = read_fasta(FRONT)
    bn, bs = read_fasta(BACK)
    # planted from a small pool, so that adapter determination keeps every class alive: two plain adapters and four barcodes that
    # exist on both sides under the same name
    both = [n for n in fn if n in bn]
    plain = [n for n in both if not n.startswith("Barcode")][:2]
    bars = [n for n in both if n.startswith("Barcode")][:4]
    F = dict(zip(fn, fs))
    B = dict(zip(bn, bs))
    pool = random_bases(seed, 4_000_000)
    at = [0]

    def take(n):
        if at[0] + n > len(pool):
            at[0] = 0
        s = pool[at[0]:at[0] + n]
        at[0] += n
        return s

    names, seqs, truth = [], [], []
    kinds = ["none", "front0", "back0", "both5", "both15", "straddle", "two_barcodes", "mismatch", "tiny_both", "short", "pair", "deep",
             "front0", "back0", "lowcomplex"]
    for i in range(n_reads):
        kind = kinds[i % len(kinds)]
        r = rng.random()
        length = int(rng.integers(300, 1500)) if r < 0.9 else int(rng.integers(1500, 20001))
        if kind == "short":
            length = int(rng.integers(60, 200))
        if kind == "tiny_both":
            length = int(rng.integers(150, 211)) if i % 2 else int(rng.integers(200, 261))
        read = take(length)
        if kind == "lowcomplex":  # homopolymer and dinucleotide-repeat ends: too few distinct k-mers to pass any adapter's gate
            read = "A" * 160 + read[160:-160] + "AC" * 80
        t = dict(kind=kind, front=None, back=None)
        err = {"both5": 0.05, "both15": 0.15}.get(kind, 0.0)

        def put_front(name, off, e=0.0):
            nonlocal read
            read = plant(read, off, mutate(rng, F[name], e))
            t["front"] = (name, off, e)

        def put_back(name, off_in_edge, e=0.0):
            nonlocal read
            read = plant(read, len(read) - EDGE + off_in_edge, mutate(rng, B[name], e))
            t["back"] = (name, off_in_edge, e)

        if length >= EDGE + 50 or kind == "tiny_both":
            if kind in ("front0", "both5", "both15"):
                put_front(plain[i % 2] if i % 3 else bars[i % 4], int(rng.integers(0, 60)), err)
            if kind in ("back0", "both5", "both15"):
                put_back(plain[i % 2] if i % 3 else bars[i % 4], int(rng.integers(60, 110)), err)
            if kind == "straddle":
                name = plain[i % 2]
                put_front(name, EDGE - len(F[name]) // 2)
                put_back(name, -(len(B[name]) // 2))
            if kind in ("two_barcodes", "deep"):
                put_front(bars[0], 5)
                read = plant(read, 70, F[bars[1]])
                t["front2"] = (bars[1], 70, 0.0)
                if kind == "deep":
                    put_back(plain[0], 10)
            if kind == "mismatch":
                put_front(bars[i % 4], int(rng.integers(0, 40)))
                put_back(bars[(i + 1) % 4], int(rng.integers(70, 110)))
            if kind == "pair":
                put_front(bars[i % 4], int(rng.integers(0, 40)))
                put_back(bars[i % 4], int(rng.integers(70, 110)))
            if kind == "tiny_both" and length >= 200:
                put_front(plain[0], 95)
                put_back(plain[0], 15)
        names.append("read%05d_%s" % (i, kind))
        seqs.append(read[:length])
        truth.append(t)
    quals = None
    if fastq:
        quals = ["".join(chr(33 + int(q)) for q in rng.integers(2, 41, size=len(s))) for s in seqs]
    return names, seqs, quals, truth


def ends_of(seqs):
    """uint8 [eligible reads, 2, 150] ASCII and the eligible read ids (reads of 200 bases and more)."""
    ids = [i for i, s in enumerate(seqs) if len(s) >= EDGE + 50]
    e = np.zeros((len(ids), 2, EDGE), dtype=np.uint8)
    for j, i in enumerate(ids):
        e[j, 0] = np.frombuffer(seqs[i][:EDGE].encode(), dtype=np.uint8)
        e[j, 1] = np.frombuffer(seqs[i][-EDGE:].encode(), dtype=np.uint8)
    return e, np.array(ids, dtype=np.int64)


def prefilter_passes(model, ends, k):
    """bool [ends]: some adapter of the end's side passes findMatches' gate (hits*10/size >= 2 || hits >= 3), computed from the
    model's index (k-mer -> seed table and adapter segments) with numpy alone."""
    ks = model.kmer_seed
    n_seeds = int(ks.max()) + 1
    nA = len(model.seg_off) - 1
    A = np.zeros((nA, n_seeds), dtype=np.float32)
    for a in range(nA):
        A[a, model.segs[model.seg_off[a] + 1:model.seg_off[a + 1]:2]] = 1
    size = A.sum(axis=1)
    n_front = sum(1 for s, _, _ in model.adapters if s == "F")
    flat = ends.reshape(-1, EDGE)
    c = (((flat >> 1) ^ ((flat & 4) >> 2)) & 3).astype(np.int64)
    km = np.zeros((len(flat), EDGE - k + 1), dtype=np.int64)
    for j in range(k):
        km = (km << 2) | c[:, j:j + EDGE - k + 1]
    sid = ks[km]
    E = np.zeros((len(flat), n_seeds + 1), dtype=np.float32)
    np.put_along_axis(E, np.where(sid < 0, n_seeds, sid), 1, axis=1)
    hits = E[:, :n_seeds] @ A.T
    gate = ((hits * 10) // np.maximum(size, 1) >= 2) | (hits >= 3)
    side = np.arange(len(flat)) % 2
    gate[side == 0, n_front:] = False
    gate[side == 1, :n_front] = False
    return gate.any(axis=1)


def end_classes(model, ends, k):
    """Counts of read ENDS per class on a model run without determination and without require_pairs (kernel-level set)."""
    r = model.recs
    found = (r[:, 2] == 1) & (r[:, 4] == 0)
    side = np.arange(len(r)) % 2
    bar = np.array([n.startswith("Barcode") for _, n, _ in model.adapters])
    n_front = sum(1 for s, _, _ in model.adapters if s == "F")
    best_global = r[:, 3] + side * n_front
    pairs = model.pairs
    fp = np.where(found[0::2], pairs[best_global[0::2]], -1)
    bp = np.where(found[1::2], pairs[best_global[1::2]], -1)
    t = model.table[model.eligible]
    return {
        "found_front": int(found[0::2].sum()),
        "found_back": int(found[1::2].sum()),
        "best_is_barcode": int((found & bar[best_global]).sum()),
        "ambiguous": int((r[:, 4] == 1).sum()),
        "pair_mismatch": int((fp != bp).sum()),
        "ignored": int((t[:, 2] == 1).sum()),
        "trimmed_without_found": int(((t[:, 3] < 0) & (t[:, 0] > 0)).sum()),
        "no_prefilter_pass": int((~prefilter_passes(model, ends, k)).sum()),
        "skipped_short": int(len(model.table) - len(model.eligible)),
    }


def read_classes(model, model_pairs, seqs):
    """Counts of READS per class for an end-to-end set: model = a run with the flags under test, model_pairs = the same input with
    require_pairs on (a mismatch shows as a read whose two ends each found an adapter while the table names none)."""
    t = model.table[model.eligible]
    r = model.recs
    found = (r[:, 2] == 1) & (r[:, 4] == 0)
    bar = np.array([n.startswith("Barcode") for _, n, _ in model.adapters])
    n_front = sum(1 for s, _, _ in model.adapters if s == "F")
    tp = model_pairs.table[model_pairs.eligible]
    rp = model_pairs.recs
    foundp = (rp[:, 2] == 1) & (rp[:, 4] == 0)
    e, _ = ends_of(seqs)
    npass = ~prefilter_passes(model, e, int(round(np.log(len(model.kmer_seed)) / np.log(4))))
    return {
        "found_front": int((t[:, 3] >= 0).sum()),
        "found_back": int((t[:, 4] >= 0).sum()),
        "best_is_barcode": int(((t[:, 3] >= 0) & bar[np.maximum(t[:, 3], 0)]).sum()) if n_front else 0,
        "ambiguous": int(((r[0::2, 4] == 1) | (r[1::2, 4] == 1)).sum()),
        "pair_mismatch": int(((foundp[0::2] | foundp[1::2]) & (tp[:, 3] < 0) & (tp[:, 4] < 0)).sum()),
        "ignored": int((t[:, 2] == 1).sum()),
        "trimmed_without_found": int(((t[:, 3] < 0) & (t[:, 0] > 0)).sum()),
        "no_prefilter_pass": int((npass[0::2] & npass[1::2]).sum()),
        "skipped_short": int(len(model.table) - len(model.eligible)),
    }
