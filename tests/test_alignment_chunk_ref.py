"""CPU: the numpy statement of a chunk's supervision lattice (tests/alignment_chunk_ref.py; include/tdnnf_hip.h, "ALIGNMENT CHUNKS") has
the properties the definition promises.  Every minibatch the GPU test assigns is a valid time-synchronous acceptor; the chunk
[0, utt_frames) is the utterance's lattice array for array; for utterances of up to 7 frames, every (o, T) and four tolerances, the
accepting paths are exactly the restrictions of the utterance's accepting paths, by brute force; synth's array route gives the statement's
arrays; infer.chunk_begins spreads the chunks as it says."""
import numpy as np
import pytest

from tests import alignment_chunk_ref as chk
from tests import alignment_supervision_ref as ali


def batches():
    out = []
    for context in (0, 1):
        for chunks, T, tol in chk.small_batches():
            out.append(pytest.param(context, chunks, T, tol, id="c%d-U%d-T%d-tol%d" % (context, chunks[0][1], T, tol)))
        for name, (chunks, T, tol) in (("narrow", chk.narrow_batch()), ("wide", chk.wide_batch())):
            out.append(pytest.param(context, chunks, T, tol, id="c%d-%s" % (context, name)))
    return out


@pytest.mark.parametrize("context,chunks,T,tol", batches())
def test_every_minibatch_is_a_time_synchronous_acceptor(pkg, context, chunks, T, tol):
    us = ali.unit_set(pkg.synth, context)
    s = chk.lattice(us, chunks, T, tol)
    assert s["B"] == len(chunks) and s["seq_state_begin"][0] == 0 and s["seq_arc_begin"][0] == 0
    time, src, dst = s["state_time"], s["arc_src"], s["arc_dst"]
    for q in range(s["B"]):
        s0, s1, a0, a1 = s["seq_state_begin"][q], s["seq_state_begin"][q + 1], s["seq_arc_begin"][q], s["seq_arc_begin"][q + 1]
        t = time[s0:s1]
        assert t[0] == 0 and (t[1:] >= 1).all() and (np.diff(t) >= 0).all() and t[-1] == T and set(t.tolist()) == set(range(T + 1))
        assert ((src[a0:a1] >= s0) & (src[a0:a1] < s1) & (dst[a0:a1] >= s0) & (dst[a0:a1] < s1)).all()
        assert (time[dst[a0:a1]] == time[src[a0:a1]] + 1).all() and (s["arc_pdf"][a0:a1] >= 0).all() and (s["arc_pdf"][a0:a1] < ali.P).all()
        pairs = list(zip(src[a0:a1].tolist(), dst[a0:a1].tolist()))
        assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
        assert np.array_equal(s["final_logprob"][s0:s1] == 0.0, t == T) and np.isneginf(s["final_logprob"][s0:s1][t < T]).all()
        # every state is on a path from the start to a final state: nothing has to be trimmed
        fwd, bwd = np.zeros(s1 - s0, bool), t == T
        fwd[0] = True
        for a in range(a0, a1):
            fwd[dst[a] - s0] |= fwd[src[a] - s0]
        for a in range(a1 - 1, a0 - 1, -1):
            bwd[src[a] - s0] |= bwd[dst[a] - s0]
        assert fwd.all() and bwd.all()
        # the start has an arc into every state of time 1
        assert dst[a0:a1][src[a0:a1] == s0].tolist() == [s0 + 1 + j for j in range(int((t == 1).sum()))]


@pytest.mark.parametrize("context", [0, 1])
def test_the_chunk_of_the_whole_utterance_is_its_lattice(pkg, context):
    us = ali.unit_set(pkg.synth, context)
    for T in ali.FRAMES:
        for tol in ali.tolerances(T):
            al = ali.small_batch(T)
            want, got = ali.lattice(us, al, T, tol), chk.lattice(us, [(a, T, 0) for a in al], T, tol)
            for k, v in want.items():
                assert np.array_equal(got[k], v) and (not isinstance(v, np.ndarray) or got[k].dtype == v.dtype), (T, tol, k)


def accepting_paths(final, arcs, name=None):
    """the accepting paths, each the tuple of its arcs' (destination, pdf); name: the destinations' names, default their numbers"""
    out = {}
    for s, d, p in arcs:
        out.setdefault(s, []).append((d, p))
    paths, stack = set(), [(0, ())]
    while stack:
        s, seq = stack.pop()
        if final[s] == 0.0:
            paths.add(seq)
        for d, p in out.get(s, []):
            stack.append((d, seq + ((name[d - 1] if name else d, p),)))
    return paths


@pytest.mark.parametrize("context", [0, 1])
def test_the_paths_of_a_chunk_are_the_restrictions_of_the_utterances_paths(pkg, context):
    """a path is its states and pdfs frame by frame; a chunk's states are named by the states of U they are"""
    us = ali.unit_set(pkg.synth, context)
    cases = 0
    for Tu in range(1, 8):
        rng = np.random.default_rng(Tu)
        for units, starts in ali.small_batch(Tu) + [ali.random_alignment(rng, Tu, mean_dur=2.0)]:
            units, starts = [int(u) for u in units], [int(b) for b in starts]
            for tol in (0, 1, 2, Tu + 3):
                _, final, arcs = ali.sequence(us, units, starts, Tu, tol)
                whole = accepting_paths(final, arcs)
                assert whole and all(len(p) == Tu for p in whole)
                for T in range(1, Tu + 1):
                    for o in range(0, Tu - T + 1):
                        _, cfinal, carcs = chk.sequence(us, units, starts, Tu, o, T, tol)
                        got = accepting_paths(cfinal, carcs, name=chk.kept_states(units, starts, Tu, o, T, tol))
                        assert got == {p[o:o + T] for p in whole}, (Tu, units, starts, tol, o, T)
                        cases += 1
    assert cases > 1000


@pytest.mark.parametrize("context,chunks,T,tol", batches())
def test_synth_cuts_the_same_lattice_with_array_operations(pkg, context, chunks, T, tol):
    """synth.supervision_lattice_from_alignment_chunks (the host route tools/graphs_bench.py times) is the statement, array for array"""
    us = ali.unit_set(pkg.synth, context)
    want = chk.lattice(us, chunks, T, tol, weight=0.5)
    got = pkg.synth.supervision_lattice_from_alignment_chunks(us, [c[0] for c in chunks], [c[1] for c in chunks], [c[2] for c in chunks], T, tol, weight=0.5)
    assert set(want) == set(got) and (got["B"], got["T"], got["weight"]) == (want["B"], want["T"], 0.5)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k


def test_the_two_large_minibatches_are_narrow_and_wide(pkg):
    us = ali.unit_set(pkg.synth, 0)
    chunks, T, tol = chk.narrow_batch()
    assert (len(chunks), T, tol) == (4, 150, 5) and all(c[1] == 400 for c in chunks) and not ali.is_wide(chk.lattice(us, chunks, T, tol))
    chunks, T, tol = chk.wide_batch()
    assert (len(chunks), T, tol) == (2, 60, 40) and all(c[1] == 150 for c in chunks) and ali.is_wide(chk.lattice(us, chunks, T, tol))


def test_chunk_begins(pkg):
    cb = pkg.infer.chunk_begins
    assert cb(7, 8) == [] and cb(8, 8) == [0] and cb(40, 8) == [0, 8, 16, 24, 32] and cb(9, 8) == [0, 1]
    assert cb(1000, 150) == [round(i * 850 / 6) for i in range(7)]
    for Tu in range(1, 60):
        for T in range(1, Tu + 1):
            b = cb(Tu, T)
            assert b[0] == 0 and b[-1] == Tu - T and len(b) == -(-Tu // T) and all(0 < y - x <= T for x, y in zip(b, b[1:]))  # no frame left out
    with pytest.raises(ValueError):
        cb(10, 0)
