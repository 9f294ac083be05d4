"""Inputs of the `map -all_sequences` tests and what is known about them without any mapper: where every read was drawn from."""
import numpy as np

from tests import oracle_lib as O

#: the reference of the multi-sequence cases
LENGTHS = [120001,  # ordinary sequence
           4999,    # no regular chunk (<= chunk_size / 2)
           61003,   # len % 4 = 3
           900,     # below query_size: no join chunk, with its stderr line
           30,      # no seed window (<= seed_rate)
           52000,   # len % 4 = 0
           12000]   # a copy of bases 20 000 - 32 000 of the first sequence
COPY = (20000, 32000)
NAMES = ["r%07d" % i for i in range(len(LENGTHS))]
SEED = 21
TOLERANCE = 150  # bases a chain's end may lie from where the truth puts it: indel drift of a 6 kb read at 5 % errors (sd ~12) + stray seeds


def reference(seed=SEED):
    """(bases, off): six i.i.d. sequences (one stream: tools/synth.cpp's genome of this seed, cut) and the planted copy"""
    g6 = int(sum(LENGTHS[:-1]))
    g = np.frombuffer(O.gen_genome(seed, g6), dtype=np.uint8)
    bases = np.concatenate([g, g[COPY[0]:COPY[1]]])
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return bases, off


def short_reads(seed, G, e):
    """the 40 reads <= 2 * query_size that tests/test_gpu_map.py's _case(short_reads=True) appends"""
    b, o = O.gen_reads(seed, G, 40, 1400, e, True)
    cut = [1200, 1600, 1996, 2000, 900, 1333]
    parts = []
    for i in range(40):
        ln = min(int(o[i + 1] - o[i]), cut[i % len(cut)])
        parts.append(b[o[i]:o[i] + ln])
    return parts


def multi_case(seed=SEED):
    """The GPU suite's multi-sequence input: the reference above, 300 reads of about 6 kb (variable length, 5 % errors) drawn from the
    concatenation of the first six sequences - some span a boundary - and the 40 short reads.  Returns ref_bases, ref_off, bases,
    off, truth; truth[i] = (start in the concatenation, strand) of the template of read i, None for the short reads (cut from
    templates whose length the generator does not tell)."""
    from tools.synth import gen_reads_truth
    ref_bases, ref_off = reference(seed)
    g6 = int(ref_off[-2])
    b, o, starts, strands = gen_reads_truth(seed, g6, 300, 6000, 0.05, True)
    parts = short_reads(seed, g6, 0.05)
    bases = np.concatenate([b] + parts)
    off = np.concatenate([o, o[-1] + np.cumsum([len(p) for p in parts])]).astype(np.int64)
    truth = [(int(s), int(r)) for s, r in zip(starts, strands)] + [None] * len(parts)
    return ref_bases, ref_off, bases, off, truth


def witness_reads(seed, ref_bases, ref_off, n, length, e, chunk_size=10000):
    """n reads of `length` template bases, each wholly inside one sequence and at least chunk_size from its ends, with errors at
    rate e (half substitutions, a quarter insertions, a quarter deletions).  Returns bases, off, truth [(sequence, start, strand)]."""
    rng = np.random.default_rng(seed)
    room = np.array([max(0, int(ref_off[c + 1] - ref_off[c]) - 2 * chunk_size - length + 1) for c in range(len(ref_off) - 1)])
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    code = np.zeros(256, dtype=np.uint8)
    code[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts, truth = [], []
    for _ in range(n):
        c = int(rng.choice(len(room), p=room / room.sum()))
        start = chunk_size + int(rng.integers(0, room[c]))
        strand = int(rng.integers(0, 2))
        t = code[ref_bases[ref_off[c] + start:ref_off[c] + start + length]]
        if strand:
            t = comp[t[::-1]]
        if e > 0:
            err = rng.random(length) < e
            kind = rng.random(length)
            sub = err & (kind < 0.5)
            ins = err & (kind >= 0.5) & (kind < 0.75)
            dele = err & (kind >= 0.75)
            t = np.where(sub, (t + rng.integers(1, 4, length)) & 3, t).astype(np.uint8)
            reps = np.ones(length, dtype=np.int64) + ins - dele
            out = np.repeat(t, reps)
            first = np.cumsum(reps) - reps  # an inserted base comes before its template base
            out[first[ins]] = rng.integers(0, 4, int(ins.sum()))
            t = out
        parts.append(letters[t])
        truth.append((c, start, strand))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts), off, truth


def parse(paf):
    """[(read index, query length, query start, query end, strand, target index, target length, start, end)] of a PAF"""
    rows = []
    for ln in paf.splitlines():
        f = ln.split("\t")
        rows.append((int(f[0][1:]), int(f[1]), int(f[2]), int(f[3]), f[4], NAMES.index(f[5]), int(f[6]), int(f[7]), int(f[8])))
    return rows


def touches_copy(c, a, b):
    """does [a, b) of sequence c lie on the planted copy or on its original?"""
    return c == len(LENGTHS) - 1 or (c == 0 and a < COPY[1] + TOLERANCE and b > COPY[0] - TOLERANCE)


def pieces(ref_off, start, tlen, strand):
    """{sequence: (first, last, a, b)} - the read coordinates [first, last) (template bases) of the part of a read drawn from each
    sequence and that part's place [a, b) on the sequence, for a template [start, start + tlen) of the concatenation"""
    out = {}
    for c in range(len(ref_off) - 1):
        a, b = max(start, int(ref_off[c])), min(start + tlen, int(ref_off[c + 1]))
        if a < b:
            out[c] = ((start + tlen - b, start + tlen - a) if strand else (a - start, b - start)) + (a - int(ref_off[c]), b - int(ref_off[c]))
    return out


def check_lines(paf, ref_off, truth, read_len, query_size=1000):
    """What holds for every PAF line of a read whose template is known, whatever the mapper's text: the target is a sequence the read
    was drawn from, the query interval lies on the part of the read drawn from that target, and the target interval lies where that
    part was drawn from.  Exempt: reads that touch the planted copy or its original (two right answers), and from the last condition
    parts within query_size of an end of their sequence (a chain found in the circular join chunk gets the reference's join-chunk
    arithmetic: an End before the sequence's start when it does not cross the join).  The template's length is taken to be the
    read's: insertions and deletions are equally likely, their difference over 6 kb at 5 % has a standard deviation of 12 bases,
    which TOLERANCE holds many times.  Returns the number of lines whose target interval was checked."""
    lens = np.diff(ref_off)
    checked = 0
    for r, qlen, qs, qe, strand, t, tl, s, e in parse(paf):
        assert tl == lens[t] and qlen == read_len[r] and 0 <= qs < qe <= qlen
        if truth[r] is None:
            continue
        start, rev = truth[r]
        pc = pieces(ref_off, start, int(read_len[r]), rev)
        if any(touches_copy(c, v[2], v[3]) for c, v in pc.items()):
            continue
        assert t in pc, "read %d drawn from %s has a line on %s" % (r, sorted(pc), NAMES[t])
        first, last, a, b = pc[t]
        assert qs >= first - TOLERANCE and qe <= last + TOLERANCE, "read %d: query %d-%d on %s, drawn from it: %d-%d" % (r, qs, qe, NAMES[t], first, last)
        if a >= query_size and b <= tl - query_size:
            assert a - TOLERANCE <= s < e <= b + TOLERANCE, "read %d: %d-%d on %s of %d bases, drawn from %d-%d" % (r, s, e, NAMES[t], tl, a, b)
            checked += 1
    return checked
