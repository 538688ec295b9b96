"""CPU: the numpy statement of the alignment supervision lattice (tests/alignment_supervision_ref.py) has the properties the definition
promises (include/tdnnf_hip.h, "ALIGNMENT SUPERVISIONS"), on the minibatches the GPU test assigns: states sorted by time, every arc one
frame ahead, every state on a path from the start to a final state, the alignment itself a path, arcs ordered by (source, destination)
with no pair twice -- and, for T <= 7, as many accepting paths as there are boundary vectors inside the UNtightened windows in strict order,
counted by brute force: the tightening prunes only what no path uses."""
import itertools

import numpy as np
import pytest

from tests import alignment_supervision_ref as ali


def batches():
    out = []
    for context in (0, 1):
        for T in ali.FRAMES:
            for tol in ali.tolerances(T):
                out.append(pytest.param(context, ali.small_batch(T), T, tol, id="c%d-T%d-tol%d" % (context, T, tol)))
        for name, (al, T, tol) in (("narrow", ali.narrow_batch()), ("wide", ali.wide_batch())):
            out.append(pytest.param(context, al, T, tol, id="c%d-%s" % (context, name)))
    return out


def count_paths(time, final, arcs, T):
    ways = np.zeros(len(time), dtype=object)
    ways[0] = 1
    for s, d, _ in arcs:  # (by source, and the sources by time: every way into s is counted before it is passed on)
        ways[d] += ways[s]
    return sum(int(ways[i]) for i in range(len(time)) if final[i] == 0.0)


def brute_force_paths(starts, T, tol):
    n = len(starts)
    ranges = [range(0, 1)] + [range(max(int(b) - tol, 0), min(int(b) + tol, T - 1) + 1) for b in starts[1:]]
    return sum(1 for v in itertools.product(*ranges) if all(v[k] < v[k + 1] for k in range(n - 1)))


@pytest.mark.parametrize("context,alignments,T,tol", batches())
def test_the_lattice_is_what_the_definition_promises(pkg, context, alignments, T, tol):
    us = ali.unit_set(pkg.synth, context)
    for units, starts in alignments:
        units, starts = [int(u) for u in units], [int(b) for b in starts]
        n = len(units)
        assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:])) and starts[-1] < T
        lo, hi = ali.windows(starts, T, tol)
        assert all(lo[k] <= starts[k] <= hi[k] for k in range(n))
        time, final, arcs = ali.sequence(us, units, starts, T, tol)
        S = len(time)
        assert time[0] == 0 and time[1] == 1 and all(a <= b for a, b in zip(time, time[1:])) and time[-1] == T
        assert all(time[d] == time[s] + 1 and 0 <= p < ali.P for s, d, p in arcs)
        pairs = [(s, d) for s, d, _ in arcs]
        assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
        out = {}
        for s, d, p in arcs:
            out.setdefault(s, []).append((d, p))
        assert all(1 <= len(v) <= 2 for v in out.values())
        # reachable from the start, and reaching a final state
        fwd, bwd = np.zeros(S, bool), np.asarray([f == 0.0 for f in final])
        fwd[0] = True
        for s, d, _ in arcs:
            fwd[d] |= fwd[s]
        for s, d, _ in reversed(arcs):
            bwd[s] |= bwd[d]
        assert fwd.all() and bwd.all() and all(time[i] == T for i in range(S) if final[i] == 0.0)
        # the alignment is a path: frame t carries the entry pdf of its unit at the unit's start and the loop pdf elsewhere
        want = []
        for k in range(n):
            left = units[k - 1] if k else -1
            end = starts[k + 1] if k + 1 < n else T
            want += [ali.entry_pdf(us, left, units[k])] + [ali.loop_pdf(us, left, units[k])] * (end - starts[k] - 1)
        here = {0}
        for t in range(T):
            here = {d for s in here for d, p in out.get(s, []) if p == want[t]}
            assert here, t
        if tol == 0 or n == T:
            assert S == T + 1 and len(arcs) == T
        if T <= 7:
            assert count_paths(time, final, arcs, T) == brute_force_paths(starts, T, tol)


@pytest.mark.parametrize("context,alignments,T,tol", batches())
def test_synth_builds_the_same_lattice_with_array_operations(pkg, context, alignments, T, tol):
    """synth.supervision_lattice_from_alignments (the host route tools/graphs_bench.py times) is the statement, array for array"""
    us = ali.unit_set(pkg.synth, context)
    want, got = ali.lattice(us, alignments, T, tol, weight=0.5), pkg.synth.supervision_lattice_from_alignments(us, alignments, T, tol, weight=0.5)
    assert set(want) == set(got) and (got["B"], got["T"], got["weight"]) == (want["B"], want["T"], 0.5)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k


def test_the_two_large_minibatches_are_narrow_and_wide(pkg):
    us = ali.unit_set(pkg.synth, 0)
    al, T, tol = ali.narrow_batch()
    assert (len(al), T, tol) == (4, 150, 5) and not ali.is_wide(ali.lattice(us, al, T, tol))
    al, T, tol = ali.wide_batch()
    assert (len(al), T, tol) == (2, 60, 40) and ali.is_wide(ali.lattice(us, al, T, tol))
