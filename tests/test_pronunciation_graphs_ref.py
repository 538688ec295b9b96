"""CPU: the definition of a transcript's graph with pronunciation alternatives (include/tdnnf_hip.h "PRONUNCIATION GRAPHS";
tests/pronunciation_graphs_ref.py states it in numpy).
  (a) for transcripts whose every position has one alternative of one unit its arrays are exactly those of tests/transcript_graphs_ref.py,
      in both contexts;
  (b) the accepting loop-free paths of small graphs, enumerated: the (alternative chosen or "skipped") tuples are exactly the product over the
      positions, each once; a path's pdfs are the entry pdfs by the true left context; its weight is the float64 sum of its terms to 1e-6;
  (c) the arcs are ordered by (source, destination), no pair twice, and an arc's label is the entry number of its destination."""
import itertools

import numpy as np
import pytest

from tests import pronunciation_graphs_ref as ref
from tests import transcript_graphs_ref as slots_ref


@pytest.fixture(scope="module")
def synth(pkg):
    return pkg.synth


def small_transcripts(synth):
    """at most 4 positions, 3 alternatives, 3 units"""
    out = [t for t in ref.edge_batch() if len(t[0]) <= 4]
    return out + synth.make_pronunciation_transcripts(60, ref.U, positions=(1, 4), alternatives=(1, 3), units=(1, 3), optional_rate=0.45, seed=7)


@pytest.mark.parametrize("context", [0, 1])
def test_single_alternative_single_unit_transcripts_are_slot_transcripts(synth, context):
    cases = 0
    for trial in range(150):
        us = synth.make_unit_set(5, context=context, seed=trial, distinct=trial % 2 == 0)
        (units, opt), = synth.make_transcripts(1, 5, slots=(1, 9), optional_rate=float([0.0, 0.3, 0.6][trial % 3]), seed=1000 + trial)
        got, want = ref.pronunciation_graph(us, ref.as_slots(units, opt)), slots_ref.transcript_graph(us, units, opt)
        for key, w in want.items():
            g = np.asarray(got[key])
            assert g.dtype == np.asarray(w).dtype and g.tobytes() == np.asarray(w).tobytes(), (trial, key, units, opt)
        # an alt_logprob of a lone alternative is not a term of any weight
        lone = ref.pronunciation_graph(us, (*ref.as_slots(units, opt), [[-3.0]] * len(units)))
        assert lone["logprob"].tobytes() == want["logprob"].tobytes()
        cases += 1
    assert cases == 150


def loop_free_paths(g):
    """every accepting path that takes no self-loop, as its list of arcs"""
    by_src = {}
    for a in range(len(g["src"])):
        if g["src"][a] != g["dst"][a]:
            by_src.setdefault(int(g["src"][a]), []).append(a)
    out = []

    def walk(s, arcs):
        if np.isfinite(g["final"][s]):
            out.append(list(arcs))
        for a in by_src.get(s, ()):
            walk(int(g["dst"][a]), arcs + [a])

    start, = np.flatnonzero(np.isfinite(g["init"]))
    assert start == 0 and g["init"][0] == 0
    walk(0, [])
    return out


@pytest.mark.parametrize("context", [0, 1])
def test_loop_free_paths_are_the_product_of_the_alternatives(synth, context):
    us = ref.unit_set(synth, context)
    entry = np.asarray(us["entry_pdf"])
    pdf_of = lambda left, u: int(entry[left + 1, u] if context else entry[u])
    leave, take, skip = np.asarray(us["leave_logprob"], np.float64), float(us["take_logprob"]), float(us["skip_logprob"])
    total = 0
    for t in small_transcripts(synth):
        positions, opt, logp = ref.normalise(t)
        g = ref.pronunciation_graph(us, t)
        of_entry = {e: pa for pa, e in ref.entry_numbers(positions).items()}
        seen = []
        for arcs in loop_free_paths(g):
            walk = [of_entry[int(g["label"][a])] for a in arcs]
            # whole alternatives, positions increasing
            chosen, k = {}, 0
            while k < len(walk):
                p, a, j = walk[k]
                L = len(positions[p][a])
                assert j == 0 and walk[k:k + L] == [(p, a, i) for i in range(L)] and (not chosen or p > max(chosen)), (t, walk)
                chosen[p] = a
                k += L
            key = tuple(chosen.get(p, "skipped") for p in range(len(positions)))
            seen.append(key)
            # the pdfs by the true left context, the weight as the float64 sum of its terms
            pdfs, w, left = [], 0.0, -1
            for p in range(len(positions)):
                if p not in chosen:
                    w += skip
                    continue
                w += (take if opt[p] else 0.0) + (float(logp[p][chosen[p]]) if len(positions[p]) >= 2 else 0.0)
                for u in positions[p][chosen[p]]:
                    pdfs.append(pdf_of(left, u))
                    w += leave[u]
                    left = u
            assert [int(g["pdf"][a]) for a in arcs] == pdfs, (t, key)
            have = float(np.sum(g["logprob"][arcs].astype(np.float64))) + float(g["final"][g["dst"][arcs[-1]]])
            assert abs(have - w) <= 1e-6, (t, key, have, w)
        want = list(itertools.product(*[list(range(len(pos))) + (["skipped"] if o else []) for pos, o in zip(positions, opt)]))
        assert len(seen) == len(set(seen)) and set(seen) == set(want) and len(seen) == len(want), (t, len(seen), len(want))
        total += len(seen)
    assert total > 500, total  # (the enumeration did not run dry: some eight paths a transcript)


@pytest.mark.parametrize("context", [0, 1])
def test_arc_order_pairs_and_labels(synth, context):
    us = ref.unit_set(synth, context, distinct=False)
    for t in ref.edge_batch() + [ref.long_transcript(), ref.heavy_transcript()] + synth.make_pronunciation_transcripts(20, ref.U, seed=4):
        positions, _, _ = ref.normalise(t)
        g = ref.pronunciation_graph(us, t)
        pairs = list(zip(g["src"].tolist(), g["dst"].tolist()))
        assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
        number = ref.entry_numbers(positions)
        assert [int(x) for x in g["label"]] == [number[g["states"][d][0]] for d in g["dst"]]
        assert g["L"] == len(number) == sum(len(alt) for pos in positions for alt in pos)
        # the states: the start, then the entries in flat order; a first entry's states in context 1 one per predecessor, never merged
        entries = [st[0] for st in g["states"][1:]]
        assert [number[e] for e in entries] == sorted(number[e] for e in entries) and set(entries) == set(number)
        assert np.array_equal(np.bincount(g["src"], minlength=g["S"]) > 0, np.ones(g["S"], bool))  # every state has its loop at least
