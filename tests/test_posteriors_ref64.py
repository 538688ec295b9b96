"""Pins tests/posteriors_ref64.py (the float64 reference the GPU forward-backward tests compare with) four independent ways: the
enumeration of every path on graphs of at most 5 states and 5 frames, the chain numerator's reference on time-synchronous graphs, the
denominator's reference (leaky 0) on a cyclic graph, and invariants (rows sum to 1, logprob >= the best path's score).  CPU only.

test_reordering_noise shuffles each graph's arc list and prints how far the reference itself moves: the floor under the GPU bars of
tests/test_gpu_posteriors.py (logprob 1e-9 relative, post 2^-23 = 1.19e-7 absolute).  Printed values of this file's cases:
    transcript graphs, 40 frames         logprob 0        relative, post 1.42e-14 absolute
    cyclic 300 states, 30 frames         logprob 8.03e-16 relative, post 1.96e-13
    peaky,  denominator graph 150 frames logprob 3.67e-16 relative, post 5.27e-13
    peaky,  supervision graphs           logprob 0        relative, post 0
    beyond, denominator graph 150 frames logprob 1.87e-16 relative, post 1.82e-12
    beyond, supervision graphs           logprob 0        relative, post 0
-- almost five decades and more below the bars on every family, the hostile ones included: the bars stand as the issue states them."""
import numpy as np
import pytest

from tests import chain_ref64 as R
from tests import posteriors_ref64 as PR
from tests import viterbi_ref64 as V
from tests.test_viterbi_ref64 import graph, random_graph

NINF = -np.inf
F = np.float32


def close(got, ref, what=""):
    assert got["ok"] == ref["ok"], (what, got["logprob"], ref["logprob"])
    if not ref["ok"]:
        assert got["logprob"] == ref["logprob"] and not got["post"].any()
        return
    assert abs(got["logprob"] - ref["logprob"]) <= 1e-12 * max(1.0, abs(ref["logprob"])), (what, got["logprob"], ref["logprob"])
    assert np.abs(got["post"] - ref["post"]).max(initial=0.0) <= 1e-12, what


# ----------------------------------------------------------------------------------------------------------------- 1. every path
@pytest.mark.parametrize("seed", range(16))
def test_random_cyclic_graphs_against_enumeration(seed):
    rng = np.random.default_rng(seed)
    S, A, T = int(rng.integers(1, 6)), int(rng.integers(1, 8)), int(rng.integers(0, 6))
    g = random_graph(rng, S, A, integer=False)
    y = (rng.standard_normal((T, 3)) * 2).astype(F)
    for scale in (1.0, 0.3):
        e = PR.enumerate_paths(g, y, scale)
        close(PR.forward_backward(g, y, scale), e, "seed %d scale %g (%d paths)" % (seed, scale, e["paths"]))


def test_enumeration_sees_many_paths():
    """(the random cases above are not all trivial: this one has a cycle and 5 frames)"""
    g = graph(3, [(0, 0, 0, -0.2), (0, 1, 1, -0.4), (1, 0, 2, -0.1), (1, 1, 0, -0.3), (1, 2, 1, -0.7), (2, 0, 2, -0.6), (0, 2, 0, -1.0)],
              [0, -0.5, NINF], [NINF, -0.25, 0])
    y = np.random.default_rng(3).standard_normal((5, 3)).astype(F)
    e = PR.enumerate_paths(g, y, 0.7)
    assert e["paths"] > 100
    close(PR.forward_backward(g, y, 0.7), e)
    assert np.allclose(e["post"].sum(1), 1.0, atol=1e-12)


def test_no_path_zero_frames_and_non_finite_outputs():
    g = graph(4, [(0, 1, 0, 0.0), (1, 2, 1, 0.0), (2, 3, 2, 0.0), (3, 3, 2, -0.5)], [0, NINF, NINF, NINF], [NINF, NINF, NINF, 0])
    r = PR.forward_backward(g, np.zeros((2, 3), F))  # the shortest accepting path has 3 arcs
    assert not r["ok"] and r["logprob"] == NINF and not r["post"].any()
    close(r, PR.enumerate_paths(g, np.zeros((2, 3), F)))
    # zero frames: LSE(init + final)
    z = graph(3, [(0, 1, 0, 0.0)], [0, -1.0, NINF], [-2.0, -0.5, 0])
    r = PR.forward_backward(z, np.zeros((0, 3), F))
    assert r["ok"] and abs(r["logprob"] - np.logaddexp(-2.0, -1.5)) < 1e-15 and r["post"].shape == (0, 3)
    close(r, PR.enumerate_paths(z, np.zeros((0, 3), F)))
    # a NaN or -inf on the only path: no candidate; +inf: logprob +inf, not ok, zeros
    for bad, want in ((np.nan, NINF), (NINF, NINF), (np.inf, np.inf)):
        y = np.zeros((3, 3), F)
        y[1, 1] = bad
        r = PR.forward_backward(g, y)
        assert not r["ok"] and r["logprob"] == want and not r["post"].any()
    # a -inf column that only one of two paths uses: skipped, the other path carries everything
    two = graph(3, [(0, 1, 0, -0.1), (0, 1, 1, -0.2), (1, 2, 2, 0.0)], [0, NINF, NINF], [NINF, NINF, 0])
    y = np.zeros((2, 3), F)
    y[0, 0] = NINF
    r = PR.forward_backward(two, y)
    assert r["ok"] and abs(r["logprob"] + 0.2) < 1e-7 and r["post"][0, 1] == 1.0 and r["post"][0, 0] == 0.0


# ----------------------------------------------------------------------------------------------------------------- 2. the numerator
@pytest.mark.parametrize("kind,seed", [("plain", 0), ("plain", 1), ("lattice", 0), ("lattice", 1)])
def test_against_the_numerator_reference(pkg, kind, seed):
    P, T, B = 30, 25, 3
    sup = (pkg.synth.make_supervision(B, T, P, max_alt=2, seed=seed) if kind == "plain"
           else pkg.synth.make_supervision_lattice(B, T, P, tolerance=2, alternatives=2, seed=seed))
    y = (np.random.default_rng(seed).standard_normal((T * B, P)) * 2).astype(F)
    lp, post = R.num_forward_backward(sup, y)
    for s, g in enumerate(pkg.synth.alignment_graphs_from_supervision(sup)):
        r = PR.forward_backward(g, y[s::B])
        assert r["ok"] and abs(r["logprob"] - lp[s]) <= 1e-12 * abs(lp[s]), (s, r["logprob"], lp[s])
        want = post[s::B]
        assert np.abs(r["post"] - want[:, :g["P"]]).max() <= 1e-12 and not want[:, g["P"]:].any()


# ----------------------------------------------------------------------------------------------------------------- 3. the denominator
@pytest.mark.parametrize("H,seed", [(20, 1), (70, 2)])
def test_against_the_denominator_reference_without_leak(pkg, H, seed):
    """a cyclic graph, which the numerator cannot check.  The denominator's reference works in the probability domain on
    exp(clip(y, -30, 30)): |y| stays below 30, and its graph takes the probabilities that the alignment graph's float32 logs stand for."""
    P, T, B = 25, 12, 2
    den = pkg.synth.make_den_graph(H, P, mean_out_degree=4.0, seed=seed)
    g = pkg.synth.alignment_graph_from_den(den)
    den = dict(den, prob=np.exp(g["logprob"].astype(np.float64)), init=np.exp(g["init"].astype(np.float64)))
    y = (np.random.default_rng(seed).standard_normal((T * B, P)) * 3).astype(F)
    assert np.abs(y).max() < 30
    lp, gamma = R.den_forward_backward(den, y, B, leaky=0.0)
    for s in range(B):
        r = PR.forward_backward(g, y[s::B])
        assert r["ok"] and abs(r["logprob"] - lp[s]) <= 1e-12 * abs(lp[s]), (s, r["logprob"], lp[s])
        assert np.abs(r["post"] - gamma[s::B]).max() <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- 4. invariants
def _families(pkg):
    """name -> list of (graph, y): the families the GPU tests run on"""
    rng = np.random.default_rng(11)
    out = {}
    seqs = [rng.integers(0, 40, size=n).tolist() for n in (1, 5, 17)]
    tg = [pkg.synth.make_alignment_graph(seqs[0], num_pdfs=40, seed=1),
          pkg.synth.make_alignment_graph(seqs[1], optional=[1, 4], alternatives={2: [7, 8]}, num_pdfs=40, seed=2),
          pkg.synth.make_alignment_graph(seqs[2], optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]}, num_pdfs=40, seed=3)]
    out["transcript"] = [(g, (rng.standard_normal((40, 40)) * 3).astype(F)) for g in tg]
    cyc = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(H=300, P=50))
    out["cyclic"] = [(cyc, (rng.standard_normal((30, 50)) * 4).astype(F))]
    H, P, B, T = 40, 30, 2, 150
    den = R.graph(pkg, H, P)
    sup = pkg.synth.make_supervision_from_den(den, B, T, num_paths=2, seed=T)
    for family in ("peaky", "beyond"):
        y = R.make_logits(family, sup, P)
        out[family + " den"] = [(pkg.synth.alignment_graph_from_den(den), y[s::B]) for s in range(B)]
        out[family + " sup"] = [(g, y[s::B]) for s, g in enumerate(pkg.synth.alignment_graphs_from_supervision(sup))]
    return out


def test_invariants(pkg):
    for name, cases in _families(pkg).items():
        for g, y in cases:
            r = PR.forward_backward(g, y)
            assert r["ok"], name
            assert np.abs(r["post"].sum(1) - 1.0).max() <= 1e-9, (name, np.abs(r["post"].sum(1) - 1.0).max())
            assert r["post"].min() >= 0.0
            best = V.best_path(g, y)["score"]
            assert r["logprob"] >= best - 1e-12 * abs(best), (name, r["logprob"], best)
            # the path that align reports has a non-zero posterior at every frame
            assert (r["post"][np.arange(len(y)), V.best_path(g, y)["pdfs"]] > 0).all()
    # one path: the sum over paths is the best path's score
    sup = pkg.synth.make_supervision(3, 25, 30, max_alt=1, seed=2)
    y = (np.random.default_rng(13).standard_normal((75, 30)) * 2).astype(F)
    for s, g in enumerate(pkg.synth.alignment_graphs_from_supervision(sup)):
        r, v = PR.forward_backward(g, y[s::3]), V.best_path(g, y[s::3])
        assert r["ok"] and abs(r["logprob"] - v["score"]) <= 1e-13 * abs(v["score"])
        assert np.array_equal(np.argmax(r["post"], 1), v["pdfs"]) and np.abs(r["post"].max(1) - 1.0).max() <= 1e-12


def test_reordering_noise(pkg):
    """the reference on each graph with its arc list shuffled: the largest change of logprob (relative) and of post (absolute)"""
    rng = np.random.default_rng(5)
    for name, cases in _families(pkg).items():
        dl, dp = 0.0, 0.0
        for g, y in cases:
            r = PR.forward_backward(g, y)
            for _ in range(3):
                perm = rng.permutation(len(g["src"]))
                q = PR.forward_backward(dict(g, src=g["src"][perm], dst=g["dst"][perm], pdf=g["pdf"][perm], logprob=g["logprob"][perm]), y)
                dl = max(dl, abs(q["logprob"] - r["logprob"]) / abs(r["logprob"]))
                dp = max(dp, float(np.abs(q["post"] - r["post"]).max()))
        print("POSTERIORS reference reordering noise, %-12s: logprob %.3g relative, post %.3g absolute" % (name, dl, dp))
        # the GPU bars (1e-9 relative, 2^-23 absolute) have to sit well above the reference's own noise
        assert dl <= 1e-10 and dp <= 2.0 ** -23 / 10
