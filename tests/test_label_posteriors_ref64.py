"""Pins tests/label_posteriors_ref64.py (the float64 reference tests/test_gpu_align_labels.py compares with) two ways, to 1e-12:
summed by pdf its per-arc posteriors are tests/posteriors_ref64.forward_backward's post, and on graphs small enough its label posteriors
are the enumeration of every path (posteriors_ref64.enumerate_paths run per arc, summed by label).  CPU only."""
import numpy as np
import pytest

from tests import label_posteriors_ref64 as LR
from tests import posteriors_ref64 as PR
from tests.test_viterbi_ref64 import graph, random_graph

NINF = -np.inf
F = np.float32
BAR = 1e-12


def _labelings(rng, g):
    A = len(g["src"])
    return {"pdf": np.asarray(g["pdf"]), "arc": np.arange(A), "one": np.zeros(A, np.int64), "coarse": rng.integers(0, 3, size=A) * 5 + 2}


@pytest.mark.parametrize("seed", range(16))
def test_random_cyclic_graphs_against_enumeration_and_by_pdf(seed):
    rng = np.random.default_rng(100 + seed)
    S, A, T = int(rng.integers(1, 6)), int(rng.integers(1, 8)), int(rng.integers(0, 6))
    g = random_graph(rng, S, A, integer=False)
    y = (rng.standard_normal((T, 3)) * 2).astype(F)
    for scale in (1.0, 0.3):
        fb = PR.forward_backward(g, y, scale)
        r = LR.arc_posteriors(g, y, scale)
        assert r["ok"] == fb["ok"] and (r["logprob"] == fb["logprob"] or abs(r["logprob"] - fb["logprob"]) <= BAR * max(1.0, abs(fb["logprob"])))
        assert np.abs(LR.sum_by(r["arc_post"], g["pdf"], np.arange(g["P"])) - fb["post"]).max(initial=0.0) <= BAR
        e = PR.enumerate_paths(*LR.per_arc_graph(g, y), scale)  # per arc, by brute force
        assert e["ok"] == r["ok"] and e["post"].shape == (T, A)
        for name, label in _labelings(rng, g).items():
            got = LR.label_posteriors(g, label, y, scale)
            assert got["labels"].tolist() == sorted(set(int(v) for v in label)) and got["post"].shape == (T, len(got["labels"]))
            want = LR.sum_by(e["post"], label, got["labels"])
            assert np.abs(got["post"] - want).max(initial=0.0) <= BAR, (seed, scale, name, e["paths"])
            if r["ok"] and T:
                assert np.abs(got["post"].sum(1) - 1.0).max() <= BAR
            if not r["ok"]:
                assert not got["post"].any()


def test_a_cycle_with_many_paths():
    """(the random cases above are not all trivial: this one has a cycle, 5 frames and labels that split a pdf and join two)"""
    g = graph(3, [(0, 0, 0, -0.2), (0, 1, 1, -0.4), (1, 0, 2, -0.1), (1, 1, 0, -0.3), (1, 2, 1, -0.7), (2, 0, 2, -0.6), (0, 2, 0, -1.0)],
              [0, -0.5, NINF], [NINF, -0.25, 0])
    label = [4, 4, 9, 1, 9, 1, 7]  # pdf 0 is on labels 4, 1 and 7; label 9 joins pdfs 2 and 1
    y = np.random.default_rng(3).standard_normal((5, 3)).astype(F)
    e = PR.enumerate_paths(*LR.per_arc_graph(g, y), 0.7)
    assert e["paths"] > 100
    got = LR.label_posteriors(g, label, y, 0.7)
    assert got["labels"].tolist() == [1, 4, 7, 9]
    assert np.abs(got["post"] - LR.sum_by(e["post"], label, got["labels"])).max() <= BAR
    fb = PR.forward_backward(g, y, 0.7)
    assert np.abs(LR.sum_by(got["arc_post"], g["pdf"], np.arange(3)) - fb["post"]).max() <= BAR
    assert abs(got["logprob"] - e["logprob"]) <= BAR * abs(e["logprob"])


def test_transcript_graphs_by_pdf(pkg):
    """larger than an enumeration reaches: transcript graphs with alternatives and optional units, unit and arc labels"""
    rng = np.random.default_rng(4)
    for labels in ("unit", "arc"):
        g = pkg.synth.make_alignment_graph(rng.integers(0, 30, size=12).tolist(), optional=[1, 7], alternatives={3: [5, 6]}, num_pdfs=30, seed=2, labels=labels)
        y = (rng.standard_normal((25, 30)) * 3).astype(F)
        fb = PR.forward_backward(g, y, 0.5)
        got = LR.label_posteriors(g, g["label"], y, 0.5)
        assert got["ok"] and len(got["labels"]) == g["L"] and got["logprob"] == fb["logprob"]
        assert np.abs(LR.sum_by(got["arc_post"], g["pdf"], np.arange(30)) - fb["post"]).max() <= BAR
        assert np.abs(got["post"].sum(1) - 1.0).max() <= BAR


def test_no_path_and_zero_frames():
    g = graph(4, [(0, 1, 0, 0.0), (1, 2, 1, 0.0), (2, 3, 2, 0.0), (3, 3, 2, -0.5)], [0, NINF, NINF, NINF], [NINF, NINF, NINF, 0])
    r = LR.label_posteriors(g, [3, 3, 1, 0], np.zeros((2, 3), F))  # the shortest accepting path has 3 arcs
    assert not r["ok"] and r["logprob"] == NINF and r["post"].shape == (2, 3) and not r["post"].any()
    r = LR.label_posteriors(g, [3, 3, 1, 0], np.zeros((0, 3), F))
    assert not r["ok"] and r["post"].shape == (0, 3)
    r = LR.label_posteriors(g, [3, 3, 1, 0], np.zeros((4, 3), F))
    assert r["ok"] and r["labels"].tolist() == [0, 1, 3] and np.allclose(r["post"], [[0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0]], atol=BAR)
