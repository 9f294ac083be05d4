"""The chaining stage of dp_find_overlaps (dp_overlap.hip: chain_walk_kernel, chain_spec_kernel, chain_resolve_kernel, chain_pair's four
paths) pair by pair against the oracle, on the crafted cases of tests/chain_cases.py - one on either side of every capacity that picks
a path (tests/test_chain_cases_cpu.py proves, without a GPU, that each case is where its name says).

Per case: candidates, records (query, target, offsets, MatchA, MatchB) and target anchors are the oracle's; under the default settings
the path every pair took (DP_DEBUG=chain_paths) is the one the capacity table predicts from the oracle's profiles; every other setting
of the stage gives the same records.  A case in which the reference would panic must fail with DP_ERR_CAPACITY and exactly the
reference's reason, and leave the context usable.  Everything is integer-exact.
"""
import os
import re

import numpy as np
import pytest

from tests import chain_cases as CC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

#: every setting of the stage a case runs under; None = the left-on-device route
SETTINGS = [
    ("passes0", {"DP_CHAIN_PASSES": "0"}), ("passes1", {"DP_CHAIN_PASSES": "1"}), ("passes3", {"DP_CHAIN_PASSES": "3"}),
    ("tier2", {"DP_CHAIN_TIER": "2"}), ("tier3", {"DP_CHAIN_TIER": "3"}), ("perfect0", {"DP_CHAIN_PERFECT": "0"}),
    ("pack1", {"DP_CHAIN_PACK": "1"}), ("no_prestage", {"DP_TUNE": "no_query_prestage=1"}), ("on_device", None),
]
KEYS = ("query", "target", "off", "match_a", "match_b")


@pytest.fixture()
def ctx():
    from downpore_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def load_index(ctx, c):
    """the device index of exactly the case's sequences (as _device_index of test_hand_known_answers.py: the kernels see seed ids only)"""
    ctx.upload_reads(np.frombuffer(b"ACGT" * 30, dtype=np.uint8), np.array([0, 120], dtype=np.int64))
    kmers = np.arange(c.n_seed_ids, dtype=np.uint32)
    if c.n_seed_ids * 37 + 5 < 4 ** c.k:
        kmers = kmers * 37 + 5
    ctx.round_begin(c.k, kmers)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in c.index])]).astype(np.uint64)
    ctx.import_segments(np.concatenate([np.asarray(s, dtype=np.int32) for s in c.index]))
    ctx.index_build(offs[:-1], np.array([len(s) // 2 for s in c.index], dtype=np.uint32))


def find(ctx, c, queries=None, env=None, **kw):
    qs = c.queries if queries is None else queries
    q = np.concatenate([np.asarray(s, dtype=np.int32) for s in qs])
    qoff = np.concatenate([[0], np.cumsum([len(s) for s in qs])]).astype(np.uint64)
    with _Env(env or {}):
        return ctx.find_overlaps(q, qoff, c.hf, c.k, c.max_length, **kw)


def check_records(c, want, out, what):
    for key in KEYS:
        assert np.array_equal(np.asarray(out[key]).astype(np.int64), want[key]), (c.name, what, key)
    assert [tuple(int(x) for x in r) for r in out["target_anchor"]] == CC.anchors(c, want), (c.name, what, "target_anchor")


def capacity_bits(ctx, c, queries=None, env=None):
    """the call must fail with DP_ERR_CAPACITY: -> the reason bits of its message"""
    from downpore_amd.hip import DpError
    with pytest.raises(DpError) as e:
        find(ctx, c, queries, env=env)
    m = re.search(r"error (-?\d+): overlap chaining hit a reference capacity limit \(bits (\d+):", str(e.value))
    assert m, str(e.value)
    assert int(m.group(1)) == _err_capacity()
    return int(m.group(2))


def _err_capacity():
    hdr = open(os.path.join(O.ROOT, "include", "downpore_hip.h")).read()
    return int(re.search(r"DP_ERR_CAPACITY\s*=\s*(-?\d+)", hdr).group(1))


@pytest.mark.parametrize("name", [n for n in CC.CASE_NAMES if n not in CC.ERROR_CASES])
def test_case_records_and_paths(ctx, name):
    c, want = CC.case(name), CC.oracle(name)
    load_index(ctx, c)
    out = find(ctx, c, env={"DP_DEBUG": "chain_paths"}, want_candidates=True)
    assert np.array_equal(out["cand_off"].astype(np.int64), want["cand_off"]) and np.array_equal(out["cand"].astype(np.int64), want["cand"])
    check_records(c, want, out, "default")
    # the path of every pair
    got = ctx.chain_paths()
    assert got["error_bits"] == 0 and got["attempts"] == 1
    predicted = CC.predict_paths(name, got["passes"])
    paths = {(int(q), int(t)): int(p) for q, t, p in zip(got["query"], got["target"], got["path"])}
    assert sorted(paths) == sorted(predicted)
    wrong = {k: (hex(paths[k]), hex(predicted[k])) for k in paths if paths[k] != predicted[k]}
    assert not wrong, (name, "pairs on another path than the capacities predict {(query, target): (device, predicted)}", wrong)
    # without the hook: the same records
    plain = find(ctx, c)
    check_records(c, want, plain, "no hook")
    for label, env in SETTINGS:
        if env is None:
            find(ctx, c, on_device=True)
            o = ctx.fetch_overlaps()
        else:
            o = find(ctx, c, env=env)
        check_records(c, want, o, label)


def test_hook_off_means_no_paths(ctx):
    from downpore_amd.hip import DpError
    c = CC.case("perfect")
    load_index(ctx, c)
    find(ctx, c)
    with pytest.raises(DpError):
        ctx.chain_paths()


@pytest.mark.parametrize("name", sorted(CC.ERROR_CASES))
def test_reference_limit_is_reported_and_the_context_lives(ctx, name):
    c, want = CC.case(name), CC.oracle(name)
    assert want["limit"] == CC.ERROR_CASES[name]
    load_index(ctx, c)
    settings = [("default", {})] + [(l, e) for l, e in SETTINGS if e is not None]
    for label, env in settings:
        assert capacity_bits(ctx, c, env=env) == want["limit"], (name, label)
    # the next call on the same context, with an ordinary case
    c2, want2 = CC.case("ratchet_stale"), CC.oracle("ratchet_stale")
    load_index(ctx, c2)
    check_records(c2, want2, find(ctx, c2), "after " + name)


def test_grown_buffers_repeat_the_stage(ctx):
    """On a fresh context the scratch columns hold 2^18 ints; the many-candidates case nine times over needs more: the stage reports its
    totals, is repeated with larger buffers and gives the same records."""
    c, want = CC.case("many_grow"), CC.oracle("many_grow")
    load_index(ctx, c)
    out = find(ctx, c, env={"DP_DEBUG": "chain_paths"}, want_candidates=True)
    got = ctx.chain_paths()
    print("attempts %d, pairs %d of %d held" % (got["attempts"], len(got["path"]), got["pair_cap"]))
    assert got["attempts"] > 1, "the first guess held: pair buffers %d" % got["pair_cap"]
    assert np.array_equal(out["cand"].astype(np.int64), want["cand"])
    check_records(c, want, out, "grown")
    again = find(ctx, c, env={"DP_DEBUG": "chain_paths"})  # (the buffers are large enough now)
    assert ctx.chain_paths()["attempts"] == 1
    check_records(c, want, again, "second call")


@pytest.mark.parametrize("hf", CC.SWEEP_HIT_FRACTIONS)
def test_seeded_sweep(ctx, hf):
    """300 random repetitive pairs, one call for those the oracle finishes; each of the others is a call of its own that must fail with
    the oracle's reason"""
    name = "sweep_%g" % hf
    c = CC.case(name)
    load_index(ctx, c)
    each = [O.find_overlaps_segments(c.index, [q], c.n_seed_ids, c.hf, c.k, c.max_length) for q in c.queries]
    good = [i for i, r in enumerate(each) if r["limit"] == 0]
    assert len(good) >= 250
    want = O.find_overlaps_segments(c.index, [c.queries[i] for i in good], c.n_seed_ids, c.hf, c.k, c.max_length)
    assert want["limit"] == 0
    out = find(ctx, c, [c.queries[i] for i in good], want_candidates=True)
    assert np.array_equal(out["cand"].astype(np.int64), want["cand"])
    check_records(c, want, out, "finishing pairs")
    for label, env in SETTINGS:
        if env is not None and label in ("passes0", "tier2", "tier3", "perfect0"):
            check_records(c, want, find(ctx, c, [c.queries[i] for i in good], env=env), label)
    for i, r in enumerate(each):
        if r["limit"]:
            assert capacity_bits(ctx, c, [c.queries[i]]) == r["limit"], (name, "query", i)
