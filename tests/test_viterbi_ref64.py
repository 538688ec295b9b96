"""Pins tests/viterbi_ref64.py (the float64 reference the GPU alignment tests compare with bit for bit) against the enumeration of every
path on graphs of at most 4 states and at most 6 frames, and checks synth.make_alignment_graph.  CPU only."""
import numpy as np
import pytest

from tests import viterbi_ref64 as V

NINF = -np.inf


def graph(S, arcs, init, final, P=3):
    """arcs: list of (src, dst, pdf, logprob)"""
    a = np.asarray(arcs, dtype=np.float64).reshape(-1, 4)
    return {"S": S, "P": P, "src": a[:, 0].astype(np.int32), "dst": a[:, 1].astype(np.int32), "pdf": a[:, 2].astype(np.int32),
            "logprob": a[:, 3].astype(np.float32), "init": np.asarray(init, dtype=np.float32), "final": np.asarray(final, dtype=np.float32)}


def random_graph(rng, S, A, integer):
    arcs = [(int(rng.integers(0, S)), int(rng.integers(0, S)), int(rng.integers(0, 3)),
             float(rng.integers(-2, 1)) if integer else float(-rng.random())) for _ in range(A)]
    init = [0.0 if rng.random() < 0.6 else NINF for _ in range(S)]
    final = [float(rng.integers(-1, 1)) if rng.random() < 0.6 else NINF for _ in range(S)]
    init[0] = 0.0
    return graph(S, arcs, init, final)


def check(g, y, scale=1.0):
    r = V.best_path(g, y, scale)
    score, arcs = V.enumerate_best(g, y, scale)
    assert r["score"] == score, (r["score"], score)
    if arcs is None:
        assert not r["ok"] and (r["pdfs"] == -1).all() and (r["states"] == -1).all()
        return r
    assert r["ok"]
    assert np.array_equal(r["arcs"], arcs), (r["arcs"], arcs)
    assert np.array_equal(r["pdfs"], np.asarray(g["pdf"])[arcs])
    T = len(arcs)
    if T:
        assert np.array_equal(r["states"][:T], np.asarray(g["src"])[arcs]) and r["states"][T] == g["dst"][arcs[-1]]
    return r


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs_against_enumeration(seed):
    rng = np.random.default_rng(seed)
    S, A, T = int(rng.integers(1, 5)), int(rng.integers(1, 7)), int(rng.integers(0, 5))
    g = random_graph(rng, S, A, integer=False)
    y = rng.standard_normal((T, 3)).astype(np.float32)
    check(g, y, 1.0)
    check(g, y, 0.3)


@pytest.mark.parametrize("seed", range(12))
def test_exact_ties_against_enumeration(seed):
    """integer-valued scores: many paths tie exactly; the first arc of the arc list and the lowest final state win"""
    rng = np.random.default_rng(100 + seed)
    S, A, T = int(rng.integers(2, 5)), int(rng.integers(3, 7)), int(rng.integers(1, 6))
    g = random_graph(rng, S, A, integer=True)
    y = rng.integers(-1, 1, size=(T, 3)).astype(np.float32)
    check(g, y)


def test_ties_follow_the_arc_order():
    # two parallel arcs 0 -> 1 with equal scores: the first of the list wins; listed the other way round, the other one does
    arcs = [(0, 1, 0, -1.0), (0, 1, 1, -1.0), (1, 1, 2, 0.0)]
    y = np.zeros((3, 3), np.float32)
    r = check(graph(2, arcs, [0, NINF], [NINF, 0]), y)
    assert list(r["pdfs"]) == [0, 2, 2]
    r = check(graph(2, [arcs[1], arcs[0], arcs[2]], [0, NINF], [NINF, 0]), y)
    assert list(r["pdfs"]) == [1, 2, 2]
    # equal final states: the lowest wins
    r = check(graph(3, [(0, 1, 0, 0.0), (0, 2, 1, 0.0)], [0, NINF, NINF], [NINF, 0, 0]), np.zeros((1, 3), np.float32))
    assert list(r["states"]) == [0, 1]


def test_six_frames_four_states():
    rng = np.random.default_rng(7)
    g = graph(4, [(0, 1, 0, -0.1), (1, 1, 0, -0.2), (1, 2, 1, -0.3), (2, 2, 1, -0.1), (2, 3, 2, -0.5), (3, 3, 2, -0.2), (0, 2, 1, -1.5)],
              [0, NINF, NINF, NINF], [NINF, NINF, NINF, 0])
    check(g, rng.standard_normal((6, 3)).astype(np.float32), 0.3)


def test_unreachable_finals_and_short_utterances():
    # the only final state cannot be reached from the initial one
    g = graph(3, [(0, 1, 0, 0.0), (1, 0, 1, 0.0), (2, 2, 2, 0.0)], [0, NINF, NINF], [NINF, NINF, 0])
    r = check(g, np.zeros((4, 3), np.float32))
    assert not r["ok"] and r["score"] == NINF
    # the shortest accepting path has 3 arcs: 2 frames are too few, 3 and 5 (with the loop) are enough
    g = graph(4, [(0, 1, 0, 0.0), (1, 2, 1, 0.0), (2, 3, 2, 0.0), (3, 3, 2, -0.5)], [0, NINF, NINF, NINF], [NINF, NINF, NINF, 0])
    r = check(g, np.zeros((2, 3), np.float32))
    assert not r["ok"] and r["score"] == NINF and list(r["pdfs"]) == [-1, -1]
    assert check(g, np.zeros((3, 3), np.float32))["ok"] and check(g, np.zeros((5, 3), np.float32))["score"] == -1.0
    # a NaN or -inf output on the only path: no candidate, no path
    y = np.zeros((3, 3), np.float32)
    y[1, 1] = np.nan
    assert not check(g, y)["ok"]
    y[1, 1] = NINF
    assert not check(g, y)["ok"]


def test_make_alignment_graph(pkg):
    seq = [3, 1, 4, 1, 5, 9, 2, 6]
    for kw in (dict(), dict(self_loops=False), dict(optional=[0, 3, 7]), dict(alternatives={0: [11], 2: [7, 8], 7: [10, 12, 13]}),
               dict(optional=[1, 4], alternatives={2: [7, 8], 5: [14]}, seed=3)):
        g = pkg.synth.make_alignment_graph(seq, **kw)
        S = g["S"]
        assert len(g["init"]) == S and len(g["final"]) == S and g["init"][0] == 0 and (g["init"][1:] == NINF).all()
        assert g["src"].min() >= 0 and g["dst"].max() < S and g["pdf"].min() >= 0 and g["pdf"].max() < g["P"] and (g["logprob"] <= 0).all()
        # every state is reachable from the start, and reaches a final state
        fwd, bwd = {0}, set(np.nonzero(g["final"] > NINF)[0])
        for _ in range(S):
            fwd |= {int(d) for s, d in zip(g["src"], g["dst"]) if s in fwd}
            bwd |= {int(s) for s, d in zip(g["src"], g["dst"]) if d in bwd}
        assert fwd == set(range(S)) and bwd == set(range(S))
        # the pdf sequence itself, every unit for one frame, is accepted: main unit k is state k + 1
        path = [0] + [k + 1 for k in range(len(seq))]
        assert g["final"][path[-1]] == 0
        for k, p in enumerate(seq):
            hit = (g["src"] == path[k]) & (g["dst"] == path[k + 1])
            assert hit.sum() == 1 and g["pdf"][hit][0] == p
        if kw.get("self_loops", True):
            loops = g["src"] == g["dst"]
            assert loops.sum() == S - 1 and np.array_equal(g["pdf"][loops], g["pdf"][[np.nonzero(g["dst"] == d)[0][0] for d in g["dst"][loops]]])
    # with a high score on the transcript's pdfs the best path of a plain graph is the transcript, repeats where the frames are more
    g = pkg.synth.make_alignment_graph(seq)
    y = np.full((len(seq), g["P"]), -5.0, np.float32)
    y[np.arange(len(seq)), seq] = 5.0
    r = V.best_path(g, y)
    assert r["ok"] and list(r["pdfs"]) == seq
    assert not V.best_path(g, y[:-1])["ok"]  # one frame short of the shortest accepting path
    g = pkg.synth.make_alignment_graph(seq, optional=[7])
    assert V.best_path(g, y[:-1])["ok"]
