"""Float64 reference of the label posteriors (include/tdnnf_hip.h, "label posteriors"): forward-backward as tests/posteriors_ref64.py runs
it, but the posterior of every ARC is formed and kept, and summed by a label of the caller's instead of by pdf:

    gamma_arc[t, a]  = exp(alpha_t[src_a] + term(a, t) + beta_t+1[dst_a] - logprob)
    post[t, k]       = sum over the arcs a with label[a] == labels[k], in arc order, of gamma_arc[t, a]

with labels the ascending list of the distinct labels of the graph's arcs (what tdnnf_align_graphs_labels returns).  alpha, beta, term and
logprob are formed exactly as there (np.logaddexp arc by arc in the graph's arc order; a candidate counts only if it compares greater
than -inf).  Pinned by tests/test_label_posteriors_ref64.py: summed by pdf it is posteriors_ref64.forward_backward's post, and on tiny
graphs it is the enumeration of every path (posteriors_ref64.enumerate_paths on per_arc_graph, summed by label).  Used by tests/test_gpu_align_labels.py.  The posteriors are UNWEIGHTED.

A graph is the dict of synth.make_alignment_graph: {S, P, src, dst, pdf, logprob, init, final}, states numbered from 0; the labels come
beside it, one int per arc."""
import numpy as np


def arc_posteriors(g, y, acoustic_scale=1.0):
    """y: [T, >= P] float32 rows of one utterance.  Returns dict(logprob, ok, arc_post [T, A] float64: zeros without a finite logprob)."""
    S = int(g["S"])
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    lp = np.asarray(g["logprob"], dtype=np.float32).astype(np.float64)
    init = np.asarray(g["init"], dtype=np.float32).astype(np.float64)
    final = np.asarray(g["final"], dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32)
    T, A = y.shape[0], len(src)
    scale = np.float64(np.float32(acoustic_scale))
    arc_post = np.zeros((T, A))
    with np.errstate(invalid="ignore", over="ignore"):
        term = lp[None, :] + scale * y[:, pdf].astype(np.float64)  # [T, A]
        alpha = np.full((T + 1, S), -np.inf)
        alpha[0] = init
        for t in range(T):
            cand = alpha[t, src] + term[t]
            keep = cand > -np.inf
            np.logaddexp.at(alpha[t + 1], dst[keep], cand[keep])
        logprob = -np.inf
        for v in alpha[T] + final:
            if v > -np.inf:
                logprob = np.logaddexp(logprob, v)
        logprob = float(logprob)
        ok = bool(np.isfinite(logprob))
        if ok:
            beta = final.copy()
            for t in range(T - 1, -1, -1):
                out = term[t] + beta[dst]
                v = alpha[t, src] + out
                keep = v > -np.inf
                arc_post[t, keep] = np.exp(v[keep] - logprob)
                beta = np.full(S, -np.inf)
                keep = out > -np.inf
                np.logaddexp.at(beta, src[keep], out[keep])
    return dict(logprob=logprob, ok=ok, arc_post=arc_post)


def sum_by(arc_post, key, columns):
    """[T, A] summed into [T, len(columns)]: column k takes the arcs with key == columns[k], one after the other in arc order"""
    key, columns = np.asarray(key, dtype=np.int64), np.asarray(columns, dtype=np.int64)
    col = np.searchsorted(columns, key)
    assert (np.diff(columns) > 0).all() and (columns[col] == key).all()
    out = np.zeros((arc_post.shape[0], len(columns)))
    for t in range(arc_post.shape[0]):
        np.add.at(out[t], col, arc_post[t])
    return out


def label_posteriors(g, label, y, acoustic_scale=1.0):
    """Returns dict(logprob, ok, labels [L] int32 ascending, post [T, L] float64, arc_post [T, A])."""
    r = arc_posteriors(g, y, acoustic_scale)
    labels = np.unique(np.asarray(label, dtype=np.int64))
    return dict(r, labels=labels.astype(np.int32), post=sum_by(r["arc_post"], label, labels))


def per_arc_graph(g, y):
    """(g', y') with the arc's own index for its pdf and y'[t, a] = y[t, pdf[a]]: the same paths with the same scores, so a per-pdf reference
    run on it (posteriors_ref64.forward_backward, .enumerate_paths) returns the posteriors per ARC"""
    pdf = np.asarray(g["pdf"], dtype=np.int64)
    return dict(g, P=len(pdf), pdf=np.arange(len(pdf), dtype=np.int32)), np.asarray(y, dtype=np.float32)[:, pdf]
