"""Inputs of the tests of `trim`'s middle stage: a seeded generator of reads with fixture adapters planted in their middles (and at
their ends, through trim_cases' adapters), and the class the MODEL put every read in."""
import numpy as np

from tests import trim_cases as TC

FRONT, BACK = TC.FRONT, TC.BACK
CLASSES = ["split", "front_crop", "tail_crop", "widened_split", "shifted_split", "ignored_by_crop", "straddle_two_chunks",
           "back_adapter_untouched", "err0", "err5", "err15", "no_chunk", "homopolymer_dropped", "dinucleotide", "three_chunks"]

KINDS = ["split", "front_crop", "tail_crop", "widened", "shifted", "ignored_crop", "straddle", "back_mid", "split5", "split15", "no_chunk",
         "homopolymer", "dinucleotide", "long3", "plain"]


def generate(seed, n_reads, fastq=False, chunk_size=5000):
    """-> names, seqs, quals (or None), truth: per read a dict(kind, planted=[(adapter name, offset, error rate)])."""
    rng = np.random.default_rng(seed)
    fn, fs = TC.read_fasta(FRONT)
    bn, bs = TC.read_fasta(BACK)
    F, B = dict(zip(fn, fs)), dict(zip(bn, bs))
    both = [n for n in fn if n in bn]
    plain = [n for n in both if not n.startswith("Barcode")][:2]
    bars = [n for n in both if n.startswith("Barcode")][:4]
    back_only = [n for n in bn if B[n] not in fs][:1] or [bn[0]]
    ga_adapter = [n for n in fn if "GAGAGA" in F[n]][0]
    pool = TC.random_bases(seed + 77, 6_000_000)
    at = [0]

    def take(n):
        if at[0] + n > len(pool):
            at[0] = 0
        s = pool[at[0]:at[0] + n]
        at[0] += n
        return s

    names, seqs, truth = [], [], []
    for i in range(n_reads):
        kind = KINDS[i % len(KINDS)]
        length = int(rng.integers(2500, 4500))
        if kind == "no_chunk":
            length = int(rng.integers(210, 400))
        if kind in ("long3", "straddle"):
            length = int(3 * chunk_size + rng.integers(200, 1500))
        if kind == "homopolymer":
            length = int(2 * chunk_size + rng.integers(500, 900))
        read = take(length)
        t = dict(kind=kind, planted=[])
        name = plain[i % 2] if i % 3 else bars[i % 4]

        def put(adapter, off, e=0.0, table=F):
            nonlocal read
            read = TC.plant(read, off, TC.mutate(rng, table[adapter], e))
            t["planted"].append((adapter, off, e))

        # every third read also carries an adapter at its front end, so that the edge stage leaves a non-zero front trim and
        # adapter determination keeps every adapter planted below
        if i % 3 == 0 and kind not in ("no_chunk", "straddle"):
            put((plain + bars)[(i // 3) % 6], int(rng.integers(0, 40)))
        mid = length // 2
        if kind == "split":
            put(name, mid)
        elif kind == "split5":
            put(name, mid, 0.05)
        elif kind == "split15":
            put(name, mid, 0.15)
        elif kind == "front_crop":
            put(name, int(rng.integers(200, 420)))
        elif kind == "tail_crop":
            put(name, length - int(rng.integers(330, 520)))
        elif kind == "widened":
            put(plain[0], mid)
            put(plain[1], mid + len(F[plain[0]]) + 40)
        elif kind == "shifted":  # a split, then a front crop by a later adapter of the list
            order = sorted([plain[0], plain[1]], key=fn.index)
            put(order[0], mid)
            put(order[1], int(rng.integers(220, 400)))
        elif kind == "ignored_crop":  # a front crop that leaves less than 500 bases: a short read with the adapter near its end
            length = int(rng.integers(700, 900))
            read = take(length)
            t["planted"] = []
            put(name, int(rng.integers(330, 420)))
        elif kind == "straddle":  # inside the 100 bases two chunks share
            put(name, 150 + (chunk_size - 100) + 20)
        elif kind == "back_mid":
            put(back_only[0], mid, 0.0, B)
        elif kind == "homopolymer":  # a first chunk without a single adapter k-mer
            read = read[:150] + "A" * chunk_size + read[150 + chunk_size:]
        elif kind == "dinucleotide":  # a (GA)n centre with, in its middle, the fixture front adapter that holds GAGAGA: the chunk is a
            # candidate of that adapter, and at k = 5 both of the repeat's k-mers are its seeds, so the reduced chunk keeps thousands
            read = read[:300] + "GA" * ((length - 600) // 2) + read[300 + 2 * ((length - 600) // 2):]
            put(ga_adapter, mid)
        elif kind == "long3":
            put(name, int(1.5 * chunk_size))
        names.append("read%05d_%s" % (i, kind))
        seqs.append(read[:length])
        truth.append(t)
    quals = None
    if fastq:
        quals = ["".join(chr(33 + int(q)) for q in rng.integers(2, 41, size=len(s))) for s in seqs]
    return names, seqs, quals, truth


def model_classes(model, edge_table, truth):
    """Counts of reads per class, read off the MODEL's run (`model`: trim_mid_model.Result, edge_table: the table of an edge-only
    model run on the same input)."""
    plan, recs, splits = model.plan, model.recs, model.splits
    n = len(model.table)
    chunks_of = np.bincount(plan[:, 0], minlength=n) if len(plan) else np.zeros(n, dtype=np.int64)
    read_of_rec = plan[recs[:, 1], 0] if len(recs) else np.zeros(0, dtype=np.int64)
    rec_reads = set(read_of_rec.tolist())
    split_reads = set(splits[:, 0].tolist()) if len(splits) else set()
    front_grew = set(np.nonzero(model.table[:, 0] > edge_table[:, 0])[0].tolist())
    back_grew = set(np.nonzero(model.table[:, 1] > edge_table[:, 1])[0].tolist())
    newly_ignored = set(np.nonzero((model.table[:, 2] == 1) & (edge_table[:, 2] == 0))[0].tolist())
    recs_per_read = np.bincount(read_of_rec, minlength=n) if len(recs) else np.zeros(n, dtype=np.int64)
    chunks_with_rec = {}
    for r, c in zip(read_of_rec.tolist(), recs[:, 1].tolist() if len(recs) else []):
        chunks_with_rec.setdefault(r, set()).add(c)

    def kind(r):
        return truth[r]["kind"]

    def err_class(e):
        return sum(1 for r in rec_reads if any(abs(x[2] - e) < 1e-9 for x in truth[r]["planted"][-1:]) and kind(r) in ("split", "split5", "split15"))

    return {
        "split": len(split_reads),
        "front_crop": len(front_grew),
        "tail_crop": len(back_grew),
        "widened_split": sum(1 for r in split_reads if recs_per_read[r] >= 2 and kind(r) == "widened"),
        "shifted_split": sum(1 for r in split_reads if r in front_grew),
        "ignored_by_crop": len(newly_ignored - split_reads),
        "straddle_two_chunks": sum(1 for r, cs in chunks_with_rec.items() if len(cs) >= 2),
        "back_adapter_untouched": sum(1 for r in range(n) if kind(r) == "back_mid" and r not in rec_reads and edge_table[r, 2] == 0),
        "err0": err_class(0.0),
        "err5": err_class(0.05),
        "err15": sum(1 for r in range(n) if kind(r) == "split15"),
        "no_chunk": int(((chunks_of == 0) & (edge_table[:, 2] == 0)).sum()),
        "homopolymer_dropped": int(((plan[:, 5] == 0) & (plan[:, 4] < 4)).sum()) if len(plan) else 0,
        "dinucleotide": sum(1 for r in range(n) if kind(r) == "dinucleotide" and chunks_of[r] > 0),
        "three_chunks": int((chunks_of >= 3).sum()),
    }
