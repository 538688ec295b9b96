"""Float64 reference of best-path alignment (include/tdnnf_hip.h, "best-path alignment"): a helper module like tests/chain_ref64.py,
pinned by tests/test_viterbi_ref64.py against the enumeration of every path, used by tests/test_gpu_align.py bit for bit.

    term(arc, t)  = float64(arc_logprob) + float64(acoustic_scale) * float64(y[t, arc_pdf])
    alpha_0[s]    = float64(initial_logprob[s])
    alpha_t+1[d]  = max over arcs into d of  alpha_t[src] + term(arc, t)
    score         = max over s of  alpha_T[s] + float64(final_logprob[s])

An arc is a candidate only if its sum is greater than -inf (a NaN is not); among equal candidates the arc that comes first in the
graph's arc list wins, among equal final states the lowest.  No accepting path: ok False, score -inf, pdf-ids and states -1; a score
of +inf: ok False as well.

A graph is the dict of synth.make_alignment_graph: {S, P, src, dst, pdf, logprob, init, final}, states numbered from 0."""
import numpy as np


def best_path(g, y, acoustic_scale=1.0):
    """y: [T, >= P] float32 rows of one utterance.  Returns dict(score, ok, pdfs [T] int32, states [T + 1] int32, arcs [T] int32: the
    chosen arcs' indexes in the graph's arc list)."""
    S = int(g["S"])
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    lp = np.asarray(g["logprob"], dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32)
    T, A = y.shape[0], len(src)
    scale = np.float64(np.float32(acoustic_scale))
    order = np.argsort(dst, kind="stable")  # by destination, the arc list's order within one
    seg_state, seg_first = np.unique(dst[order], return_index=True)
    alpha = np.asarray(g["init"], dtype=np.float32).astype(np.float64)
    bp = np.full((T, S), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            cand = alpha[src] + (lp + scale * y[t, pdf].astype(np.float64))
            cand = np.where(np.isnan(cand), -np.inf, cand)[order]
            nxt = np.full(S, -np.inf)
            if A:
                best = np.maximum.reduceat(cand, seg_first)
                nxt[seg_state] = best
                seg_of = np.searchsorted(seg_first, np.arange(A), side="right") - 1
                hit = np.where((cand == best[seg_of]) & (cand > -np.inf), np.arange(A), A)
                first = np.minimum.reduceat(hit, seg_first)
                ok = first < A
                bp[t, seg_state[ok]] = order[first[ok]]
            alpha = nxt
        fin = alpha + np.asarray(g["final"], dtype=np.float32).astype(np.float64)
    fin = np.where(np.isnan(fin), -np.inf, fin)
    score = float(fin.max())
    pdfs, states, arcs = np.full(T, -1, np.int32), np.full(T + 1, -1, np.int32), np.full(T, -1, np.int32)
    ok = score > -np.inf and score < np.inf
    if ok:
        st = int(np.argmax(fin))  # (the first of equal maxima)
        states[T] = st
        for t in range(T - 1, -1, -1):
            a = int(bp[t, st])
            assert a >= 0
            arcs[t], pdfs[t], st = a, pdf[a], int(src[a])
            states[t] = st
    return dict(score=score if score > -np.inf else -np.inf, ok=bool(ok), pdfs=pdfs, states=states, arcs=arcs)


def enumerate_best(g, y, acoustic_scale=1.0):
    """The same by brute force for tiny cases: every arc sequence of length T, scored with the sums in the recursion's order; the winner
    among equal scores is the one the tie rules above pick (decided from the last frame backwards, as a trace-back does: lowest final
    state, then at every frame from the last to the first the earliest arc among the paths that still tie).  Returns (score, arcs)."""
    import itertools
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    lp = np.asarray(g["logprob"], dtype=np.float32).astype(np.float64)
    init = np.asarray(g["init"], dtype=np.float32).astype(np.float64)
    final = np.asarray(g["final"], dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32)
    T, A, S = y.shape[0], len(src), int(g["S"])
    scale = np.float64(np.float32(acoustic_scale))
    best, winners = -np.inf, []
    starts = range(S) if T == 0 else [None]
    for path in itertools.product(range(A), repeat=T):
        for s_only in starts:
            if T == 0:
                v, end = init[s_only], s_only
            else:
                if any(dst[path[t]] != src[path[t + 1]] for t in range(T - 1)):
                    continue
                v = init[src[path[0]]]
                for t, a in enumerate(path):
                    v = v + (lp[a] + scale * np.float64(y[t, pdf[a]]))
                end = dst[path[-1]]
            v = v + final[end]
            if not v > -np.inf:
                continue
            key = (int(end),) + tuple(int(a) for a in reversed(path))
            if v > best:
                best, winners = v, [key]
            elif v == best:
                winners.append(key)
    if not winners:
        return -np.inf, None
    key = min(winners)
    return float(best), np.asarray(list(reversed(key[1:])), dtype=np.int32)
