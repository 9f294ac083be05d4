"""dp_align_spans held to the model of the rule (tests/native/align_model.cpp: full matrix, canonical walk), pair by pair, on crafted
pairs cut from one uploaded read set.  The model reads the bases the device holds (dp_reads_packed), so NM and the CIGAR must be equal
to the letter.  One upload and a handful of calls serve every test; the expected values are computed once."""
import numpy as np
import pytest

from tests import align_model as A

pytestmark = pytest.mark.gpu

LENS = [1, 2, 63, 64, 65, 255, 256, 257]
APART = [0, 1, 63, 64, 65, 300]
OFFSETS = [0, 1, 2, 3, 63, 64, 65]  # every residue mod 4, and either side of the 16-byte (64-base) mark behind a read's start


def _rand(rng, n):
    return rng.integers(0, 4, int(n)).astype(np.uint8)


def _mutate(rng, t, rate):
    """substitutions, insertions and deletions mixed, about `rate` of the bases"""
    out = []
    for b in t:
        r = rng.random()
        if r < rate / 3:
            out.append((int(b) + 1 + int(rng.integers(0, 3))) % 4)
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out.append(int(b))
            out.append(int(rng.integers(0, 4)))
        else:
            out.append(int(b))
    return np.array(out, dtype=np.uint8)


def _fit(rng, q, m):
    return q[:m] if len(q) >= m else np.concatenate([q, _rand(rng, m - len(q))])


class Cases:
    """reads (as codes) and items by group name"""

    def __init__(self):
        self.reads, self.groups = [], {}

    def add(self, group, q, t, q_off=0, t_off=0, rng=None, t_whole=None):
        rng = rng or np.random.default_rng(len(self.reads))
        qr = np.concatenate([_rand(rng, q_off), q, _rand(rng, 3)])
        tr = t_whole if t_whole is not None else np.concatenate([_rand(rng, t_off), t, _rand(rng, 5)])
        self.reads += [qr, tr]
        n = len(self.reads)
        self.groups.setdefault(group, []).append((n - 2, q_off, len(q), n - 1, t_off, len(t)))


def _build():
    rng = np.random.default_rng(20260117)
    c = Cases()
    for base in LENS:  # lengths around the wave and the 16-base word, m = n and m, n apart, either one the longer
        for d in APART:
            for m, n in {(base, base + d), (base + d, base)}:
                t = _rand(rng, n)
                c.add("lengths", _fit(rng, _mutate(rng, t, 0.1), m), t, rng=rng)
    for qo in OFFSETS:
        for to in OFFSETS:
            t = _rand(rng, 75)
            c.add("offsets", _fit(rng, _mutate(rng, t, 0.08), 70), t, q_off=qo, t_off=to, rng=rng)
    same = _rand(rng, 300)
    c.add("identical", same, same.copy(), q_off=5, t_off=2, rng=rng)
    c.add("disjoint", np.zeros(100, dtype=np.uint8), np.ones(130, dtype=np.uint8), rng=rng)  # poly-A against poly-C
    c.add("disjoint", np.zeros(130, dtype=np.uint8), np.ones(100, dtype=np.uint8), rng=rng)
    for rate in (0.0, 0.05, 0.15, 0.30):
        for _ in range(125):
            t = _rand(rng, rng.integers(50, 601))
            q = _mutate(rng, t, rate)
            q = q if 50 <= len(q) <= 600 else _fit(rng, q, min(600, max(50, len(q))))
            c.add("random", q, t, q_off=int(rng.integers(0, 9)), t_off=int(rng.integers(0, 9)), rng=rng)
    t = _rand(rng, 12000)
    c.add("long", _mutate(rng, t, 0.12), t, q_off=1, t_off=3, rng=rng)
    # the optimal path drifts 200 diagonals to one side and back: 200 bases cut out at 500, 200 foreign ones put in at 1500
    t = _rand(rng, 2000)
    q = np.concatenate([t[:500], t[700:1700], _rand(rng, 200), t[1700:]])
    assert len(q) == 2000
    c.add("drift", q, t, rng=rng)
    # NM exactly 50 and 51: substitutions seven bases apart in a random target
    t = _rand(rng, 400)
    for k in (50, 51):
        q = t.copy()
        q[3:3 + 7 * k:7] = (q[3:3 + 7 * k:7] + 1) % 4
        c.add("cap", q, t, q_off=2, rng=rng)
    # a circular target of 500 bases: wrapping after one base, before the last base, and starting at the read's length
    ring = _rand(rng, 500)
    for t_off, n in ((499, 120), (500 - 119, 120), (500, 90), (250, 500)):
        tt = np.concatenate([ring, ring])[t_off:t_off + n]
        c.add("circular", _mutate(rng, tt, 0.1), tt, q_off=1, t_off=t_off, rng=rng, t_whole=ring)
    # no shared base at a size whose band outgrows the LDS tier (more than 128 diagonals per lane)
    c.add("wide", np.zeros(5000, dtype=np.uint8), np.ones(4800, dtype=np.uint8), rng=rng)
    return c


def _unpack(packed, n):
    b = np.asarray(packed, dtype=np.uint8)
    codes = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)
    return codes[:n]


@pytest.fixture(scope="module")
def world():
    import downpore_amd
    cases = _build()
    ctx = downpore_amd.Context(0)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in cases.reads])]).astype(np.int64)
    ctx.upload_reads(np.concatenate([letters[r] for r in cases.reads]), off)
    held = [_unpack(ctx.packed_read(r), len(cases.reads[r])) for r in range(len(cases.reads))]  # the codes the device holds
    for r, h in enumerate(held):
        assert np.array_equal(h, cases.reads[r]), r
    want = {}
    for g, items in cases.groups.items():
        want[g] = []
        for (qr, qo, m, tr, to, n) in items:
            tt = np.concatenate([held[tr], held[tr]])[to:to + n] if g == "circular" else held[tr][to:to + n]
            want[g].append(A.align(held[qr][qo:qo + m], tt))
    yield dict(ctx=ctx, cases=cases, want=want)
    ctx.close()


def _check(got, want, what, max_edits=None):
    assert len(got["nm"]) == len(want)
    for x, (nm, cigar) in enumerate(want):
        if max_edits is not None and nm > max_edits:
            assert got["nm"][x] == -1 and got["cigar"][x] == "", (what, x)
        else:
            assert (int(got["nm"][x]), got["cigar"][x]) == (nm, cigar), (what, x, nm)


def test_crafted_pairs_in_one_call_and_again(world):
    """lengths, offsets, identical strings, no shared base, the random pairs and the 12 kb pair in ONE call; then the same call again on
    the same context, which must find no stale buffer"""
    names = ["lengths", "offsets", "identical", "disjoint", "random", "long"]
    items = [it for g in names for it in world["cases"].groups[g]]
    want = [w for g in names for w in world["want"][g]]
    assert len(world["cases"].groups["random"]) == 500 and len(items) > 600
    first = world["ctx"].align_spans(items)
    _check(first, want, "first call")
    assert first["cells"] > 0 and first["tb_bytes"] > 0
    again = world["ctx"].align_spans(items)
    _check(again, want, "second call")
    assert (again["cells"], again["tb_bytes"], again["doublings"]) == (first["cells"], first["tb_bytes"], first["doublings"])
    w = world["want"]
    assert w["identical"] == [(0, "300M")]
    assert [nm for nm, _ in w["disjoint"]] == [130, 130]  # NM = max(m, n)
    assert 1000 < w["long"][0][0] < 1600


def test_drift_pair_forces_two_band_doublings(world):
    (nm, cigar), = world["want"]["drift"]
    import re
    diag = far = 0
    for ln, op in re.findall(r"(\d+)([MID])", cigar):
        diag += int(ln) if op == "D" else -int(ln) if op == "I" else 0
        far = max(far, diag)
    assert 256 < nm <= 400 and far == 200 and diag == 0  # out to diagonal 200 and back: more than |m - n| + 2 x 128 edits
    got = world["ctx"].align_spans(world["cases"].groups["drift"])
    _check(got, world["want"]["drift"], "drift")
    assert got["doublings"] == 2  # 64 -> 128 -> 256: a build that starts wide does not pass by accident


def test_nm_at_the_cap_and_one_above(world):
    assert [nm for nm, _ in world["want"]["cap"]] == [50, 51]
    got = world["ctx"].align_spans(world["cases"].groups["cap"], max_edits=50)
    _check(got, world["want"]["cap"], "cap", max_edits=50)
    assert list(got["nm"]) == [50, -1]


def test_circular_targets(world):
    got = world["ctx"].align_spans(world["cases"].groups["circular"], circular=True)
    _check(got, world["want"]["circular"], "circular")
    # the same items on a linear call lie outside their reads
    from downpore_amd.hip import DpError
    with pytest.raises(DpError):
        world["ctx"].align_spans(world["cases"].groups["circular"][:1], circular=False)


def test_band_beyond_the_lds_tier(world):
    assert world["want"]["wide"] == [(5000, "200I4800M")]
    got = world["ctx"].align_spans(world["cases"].groups["wide"], max_edits=32768)
    _check(got, world["want"]["wide"], "wide")
    assert got["doublings"] == 6  # 64 -> 4096: 8193 diagonals, 132 per lane
    # with the default cap the lengths' difference and the band prove NM > 4096 without reaching that width
    assert list(world["ctx"].align_spans(world["cases"].groups["wide"])["nm"]) == [-1]


def test_arguments_over_the_limits_are_refused(world):
    from downpore_amd.hip import DpError
    ctx, reads = world["ctx"], world["cases"].reads
    good = world["cases"].groups["identical"][0]
    qr, qo, m, tr, to, n = good
    bad = [(len(reads), 0, 1, tr, 0, 1), (qr, 0, 1, len(reads), 0, 1), (qr, 0, 0, tr, 0, 1), (qr, 0, 1, tr, 0, 0),
           (qr, len(reads[qr]) - 1, 2, tr, 0, 1), (qr, 0, 1, tr, len(reads[tr]) - 1, 2), (qr, 0, (1 << 20) + 1, tr, 0, 1), (qr, 0, 1, tr, 0, (1 << 20) + 1)]
    for it in bad:
        with pytest.raises(DpError, match="dp_align_spans"):
            ctx.align_spans([good, it])
    for circ_bad in [(qr, 0, 1, tr, len(reads[tr]) + 1, 1), (qr, 0, 1, tr, 0, len(reads[tr]) + 1)]:
        with pytest.raises(DpError, match="dp_align_spans"):
            ctx.align_spans([circ_bad], circular=True)
    for cap in (0, 32769):
        with pytest.raises(DpError, match="max_edits"):
            ctx.align_spans([good], max_edits=cap)
    assert ctx.align_spans(np.zeros((0, 6), dtype=np.uint32))["nm"].size == 0
    _check(ctx.align_spans([good]), world["want"]["identical"], "after the refusals")  # the context is as usable as before
