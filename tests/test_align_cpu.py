"""The alignment rule of DESIGN.md 4.9 without a GPU: the model (tests/native/align_model.cpp: full matrix, canonical walk) against
hand-worked pairs, against a brute-force enumeration of every alignment of short strings, and against two deliberate mutations of the
walk; then the Python surface and the header / export entries of the feature."""
import inspect
import os
import random
import re

import pytest

from tests import align_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (query, target, NM, CIGAR).  The first four are the rule's worked examples; the rest were walked by hand from (m, n):
# M if the diagonal explains the cell, else I if the cell above does, else D.
HAND = [
    ("AAA", "AAAA", 1, "1D3M"),        # gaps go to the left end
    ("AAAA", "AAA", 1, "1I3M"),
    ("ACGT", "AGT", 1, "1M1I2M"),
    ("AC", "CA", 2, "2M"),             # two mismatches tie with a gap pair: M wins
    ("A", "A", 0, "1M"),               # m = n = 1
    ("A", "C", 1, "1M"),
    ("A", "AAAA", 3, "3D1M"),          # m = 1: the one base matches the LAST target base, the gap leads
    ("AAAA", "A", 3, "3I1M"),          # n = 1
    ("ACG", "ACGT", 1, "3M1D"),        # a trailing gap where nothing else explains the last column
    ("ACGT", "ACG", 1, "3M1I"),
    ("CGT", "ACGT", 1, "1D3M"),        # a leading gap
    ("ACA", "CAC", 2, "1D2M1I"),       # at (3, 3) only I explains the cell; at (0, 1) only D is left
    ("ACAA", "CACA", 2, "1D2M1I1M"),
    ("AAT", "ATA", 2, "3M"),           # mismatch-versus-gap tie at (3, 3) and (2, 2): M both times
    ("AAAAA", "AAA", 2, "2I3M"),       # homopolymer: both gaps at the left end
    ("CAAT", "CAAAT", 1, "1M1D3M"),    # ... at the left end of the run, not of the string
    ("CAAAT", "CAAT", 1, "1M1I3M"),
    ("ACCT", "ACT", 1, "1M1I2M"),
]


def test_hand_worked_pairs():
    assert len(HAND) >= 12
    for q, t, nm, cigar in HAND:
        assert A.align(q, t) == (nm, cigar), (q, t)
        assert A.consumed(cigar) == (len(q), len(t))


def _all_alignments(q, t):
    """every path from (0, 0) to (m, n) as (cost, merged CIGAR): M costs a mismatch, I and D cost 1"""
    out = []

    def go(i, j, cost, ops):
        if i == len(q) and j == len(t):
            out.append((cost, "".join("%d%s" % (len(m.group(0)), m.group(0)[0]) for m in re.finditer(r"M+|I+|D+", ops))))
            return
        if i < len(q) and j < len(t):
            go(i + 1, j + 1, cost + (q[i] != t[j]), ops + "M")
        if i < len(q):
            go(i + 1, j, cost + 1, ops + "I")
        if j < len(t):
            go(i, j + 1, cost + 1, ops + "D")

    go(0, 0, 0, "")
    return out


def _short_pairs():
    words = [""]
    for n in range(1, 5):
        words += ["".join(w) for w in __import__("itertools").product("AC", repeat=n)]
    words = [w for w in words if w]
    pairs = [(q, t) for q in words for t in words if len(q) + len(t) <= 6]
    rng = random.Random(20260117)
    for _ in range(40):
        pairs.append(("".join(rng.choice("ACGT") for _ in range(rng.randint(5, 6))), "".join(rng.choice("ACG") for _ in range(rng.randint(4, 6)))))
    return pairs


def test_model_against_brute_force_enumeration():
    """NM is the cheapest of ALL alignments, and the canonical CIGAR is one of the cheapest ones."""
    pairs = _short_pairs()
    assert len(pairs) > 300 and max(len(q) for q, _ in pairs) == 6
    for q, t in pairs:
        every = _all_alignments(q, t)
        best = min(c for c, _ in every)
        nm, cigar = A.align(q, t)
        assert nm == best, (q, t)
        assert cigar in {s for c, s in every if c == best}, (q, t, cigar)
        assert A.consumed(cigar) == (len(q), len(t))


@pytest.mark.parametrize("mutation", [A.PREFER_I_OVER_M, A.D_BEFORE_I])
def test_the_hand_cases_catch_a_mutated_walk(mutation):
    """both wrong walks still give NM and an optimal alignment - only the canonical choice tells them apart, and the hand cases do"""
    wrong = [(q, t) for q, t, nm, cigar in HAND if A.align(q, t, mutation) != (nm, cigar)]
    assert wrong, "no hand-worked pair notices mutation %d" % mutation
    for q, t, nm, _ in HAND:
        assert A.align(q, t, mutation)[0] == nm


def test_model_on_a_larger_pair_is_consistent():
    rng = random.Random(5)
    t = "".join(rng.choice("ACGT") for _ in range(3000))
    q = list(t)
    for _ in range(300):
        p = rng.randrange(len(q))
        r = rng.random()
        if r < 0.4:
            q[p] = rng.choice("ACGT")
        elif r < 0.7:
            del q[p]
        else:
            q.insert(p, rng.choice("ACGT"))
    q = "".join(q)
    nm, cigar = A.align(q, t)
    assert 0 < nm <= 300 and A.consumed(cigar) == (len(q), len(t))
    # the CIGAR's own cost is NM: mismatches under its M runs plus its gap lengths
    i = j = cost = 0
    for ln, op in re.findall(r"(\d+)([MID])", cigar):
        ln = int(ln)
        if op == "M":
            cost += sum(1 for x in range(ln) if q[i + x] != t[j + x])
            i, j = i + ln, j + ln
        elif op == "I":
            cost, i = cost + ln, i + ln
        else:
            cost, j = cost + ln, j + ln
    assert cost == nm


# ---- the Python surface, the headers and the exports

def test_python_surface():
    from downpore_amd import mapping as M
    from downpore_amd.hip import DpError
    assert list(inspect.signature(M.Mapper.map_aligned).parameters) == ["self", "reads", "trim", "max_edits"]
    assert inspect.signature(M.Mapper.map_aligned).parameters["max_edits"].default == 4096
    sig = inspect.signature(M.map_reads_aligned)
    assert list(sig.parameters)[:2] == ["ref", "reads"] and sig.parameters["max_edits"].default == 4096 and sig.parameters["trim"].default is None
    assert list(sig.parameters)[:-1] == list(inspect.signature(M.map_reads).parameters)
    doc = M.map_reads_aligned.__doc__
    assert "DP_MAP_SHARDS" in doc and "map_ascii_upload" in doc and "not available" in doc
    # what the existing tests pin stays
    assert list(inspect.signature(M.Mapper.map).parameters) == ["self", "reads", "trim"]
    assert len(M.MAP_STAT_FIELDS) == 13
    assert M.MAP_ALIGN_FIELDS == ["lines", "aligned", "over_max_edits", "out_of_range", "cells", "band_doublings", "kernel_us", "traceback_bytes"]
    m = object.__new__(M.Mapper)  # (no device here: the refusals come before any library call)
    m.h = None
    for bad in (0, 40000, True, 1.5):
        with pytest.raises(DpError, match="max_edits"):
            m.map_aligned(None, max_edits=bad)
    with pytest.raises(DpError, match="closed"):
        m.map_aligned(None, max_edits=50)


def _strip(txt):
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_and_exports():
    hip_h = _strip(open(os.path.join(ROOT, "include", "downpore_hip.h")).read())
    host_h = _strip(open(os.path.join(ROOT, "include", "downpore_host.h")).read())
    assert re.search(r"\bdp_align_spans\s*\(\s*dp_ctx\s*\*\s*ctx\s*,\s*const\s+dp_align_item\s*\*\s*items\s*,\s*uint32_t\s+n\s*,\s*uint32_t\s+max_edits\s*,\s*int\s+circular\s*,"
                     r"\s*dp_align_batch\s*\*\s*out\s*\)", hip_h)
    for name in ("dp_align_item", "dp_align_rec", "dp_align_batch"):
        assert re.search(r"\}\s*%s\s*;" % name, hip_h), name
    m = re.search(r"\bdph_mapper_map_align\s*\(([^)]*)\)", host_h)
    assert m and len(m.group(1).split(",")) == 9
    assert re.search(r"\bdph_map_align_info\s*\(\s*void\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*out\s*,\s*int\s+cap\s*\)", host_h)
    assert "#define DPH_MAP_STATS 13" in host_h
    import downpore_amd.hip as h
    from downpore_amd.overlap import load_host
    assert "dp_align_spans" in h.SYMBOLS and hasattr(h.load_library(), "dp_align_spans")
    H = load_host()
    assert hasattr(H, "dph_mapper_map_align") and hasattr(H, "dph_map_align_info")
    assert h.ALIGN_ITEM.itemsize == 24 and h.ALIGN_REC.itemsize == 16
    go = open(os.path.join(ROOT, "integration", "gpuhost", "chost.go")).read()
    assert re.search(r"^func \(m \*Mapper\) MapAlign\(", go, flags=re.M) and "C.dph_mapper_map_align(" in go and "C.dph_map_align_info(" in go
