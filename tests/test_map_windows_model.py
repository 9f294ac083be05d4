"""The plain model of performMapping's device part (tests/map_model.py) against the oracle's own performMapping, call by call:
the model is what the GPU tests hold dp_map_windows against where no reads exist (the crafted relaunch cases of
tests/map_crafted.py), so it has to be right wherever the oracle can say what right is.  No GPU.  About 30 s, most of it the
oracle's k = 13 value table (twice: the traced and the plain run)."""
import json
import os

import numpy as np
import pytest

from tests import map_crafted as MC
from tests import map_model as MM
from tests import oracle_lib as O

_STATS = {}


def _index_of(run):
    isegs, ioff = run.trace("indexedSegments")
    return MM.Index([isegs[ioff[i]:ioff[i + 1]] for i in range(len(ioff) - 1)], len(run.trace("seedKmers")))


@pytest.mark.parametrize("name", sorted(MC.TRACED))
def test_model_equals_oracle_trace(name):
    """Candidates of both strands and every chain (strand, chunk, MatchA, MatchB, append order) of every traced performMapping call;
    the traced run prints the PAF of the plain one."""
    run = MC.traced_run(name)
    ref, reads, k = MC.traced_inputs(name)
    paf, err = O.map_run(ref, reads, circular=True, k=k)
    assert run.paf == paf and run.err == err
    assert run.n_calls == run.calls_made > 0
    ix = _index_of(run)
    drops = chains_total = 0
    for c in range(run.n_calls):
        tc = run.call(c)
        d = {}
        cf, cr, chains = ix.perform(tc["fwdSegments"], tc["rcSegments"], tc["lengths"][0], tc["lengths"][1], k, d)
        assert cf == tc["candidates"].tolist(), (name, c)
        assert cr == tc["rcCandidates"].tolist(), (name, c)
        assert chains == MC.traced_chains(tc), (name, c)
        drops += len(d["ratchet_drops"]) > 0
        chains_total += len(chains)
    print("%s: %d calls, %d chains, %d calls in which a ratchet drops a later candidate" % (name, run.n_calls, chains_total, drops))
    _STATS[name] = (run.n_calls, drops)


def test_traced_inputs_cover_enough_calls_and_a_ratchet_drop():
    """At least 300 traced calls in all, and at least one call in which a chain's ratchet drops a later candidate whose prefilter
    count reaches the window's own threshold (what separates a ratchet that works from one that does not)."""
    for name in sorted(MC.TRACED):
        if name not in _STATS:
            test_model_equals_oracle_trace(name)
    assert sum(n for n, _ in _STATS.values()) >= 300, _STATS
    assert sum(d for _, d in _STATS.values()) >= 1, _STATS


def test_model_reproduces_hand_case_extend_chain_skip():
    h = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand", "extend_chain_skip.json")))
    ix = MM.Index([h["target_segments"]] + h["decoy_segments"], 64)
    cf, cr, chains = ix.perform(h["query_segments"], [h["window_len"]], h["window_len"], h["window_len"], h["k"])
    assert cf == [0] and cr == []
    assert chains == [(0, 0, m["match_a"], m["match_b"]) for m in h["expect"]]


@pytest.mark.parametrize("case", ["big", "records", "ints"])
def test_model_on_crafted_cases(case):
    """The crafted relaunch inputs: the model is deterministic on them (two evaluations on two indexes agree array for array),
    they reach what they are built to reach (a chain longer than 256; more than 65 536 chains within 2 097 152 ints; more than
    2 097 152 ints within 65 536 chains - in the whole index and in the forward pass of the first shard alone), and the
    ratchet-sensitive pair behaves as described: t0's short chain, t1's long one, t3's chain at a count equal to the raised
    threshold, t2 dropped by the forward chain's ratchet."""
    c = MC.build(case)
    outs = []
    for _ in range(2):
        ix = MM.Index(c["chunks"], c["n_seeds"])
        outs.append(MM.map_windows(ix, c["w_segs"], c["w_off"], c["w_len"], c["k"]))
    a, b = outs
    for key in ("window", "target", "off", "match_a", "match_b"):
        assert np.array_equal(a[key], b[key]), key
    assert a["cands"] == b["cands"] and a["distinct"] == c["distinct"]
    lens = np.diff(a["off"])
    first = (a["target"] < c["split"]) & (a["window"] % 2 == 0)  # the first shard's forward pass
    for n_chains, n_ints in ((len(lens), int(lens.sum())), (int(first.sum()), int(lens[first].sum()))):
        if case == "big":
            assert lens.max() > 256
        elif case == "records":
            assert n_chains > 65536 and n_ints <= 2097152
        else:
            assert n_ints > 2097152 and n_chains <= 65536
    sp = c["sensitive_pair"]
    wo, ws = c["w_off"], c["w_segs"]
    d = {}
    cf, cr, chains = ix.perform(ws[int(wo[2 * sp]):int(wo[2 * sp + 1])], ws[int(wo[2 * sp + 1]):int(wo[2 * sp + 2])], c["w_len"][2 * sp],
                                c["w_len"][2 * sp + 1], c["k"], d)
    assert cf == [MC.T0, MC.T1, MC.T3] and cr == [MC.T2]
    assert [(s, t, len(x)) for s, t, x, _ in chains] == [(0, MC.T0, 10), (0, MC.T1, 40), (0, MC.T3, 32)]
    assert d["ratchet_drops"] == [(1, MC.T2)] and d["thr"] == [32, 32]
