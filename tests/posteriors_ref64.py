"""Float64 reference of forward-backward over pdf-labelled graphs (include/tdnnf_hip.h, "forward-backward"): a helper module like
tests/viterbi_ref64.py, pinned by tests/test_posteriors_ref64.py four independent ways, used by tests/test_gpu_posteriors.py.

    term(arc, t)   = float64(arc_logprob) + float64(acoustic_scale) * float64(y[t, arc_pdf])
    alpha_0[s]     = float64(initial_logprob[s])
    alpha_t+1[d]   = LSE over arcs into d   of  alpha_t[src] + term(arc, t)
    logprob        = LSE over s             of  alpha_T[s] + float64(final_logprob[s])
    beta_T[s]      = float64(final_logprob[s])
    beta_t[s]      = LSE over arcs out of s of  term(arc, t) + beta_t+1[dst]
    gamma[t, p]    = sum over arcs with pdf p of exp(alpha_t[src] + term(arc, t) + beta_t+1[dst] - logprob)

Every LSE is np.logaddexp applied arc by arc in the graph's arc order (ufunc.at is unbuffered: one arc after the other); a candidate
counts only if it compares greater than -inf, so a NaN or -inf one adds nothing.  ok iff logprob is finite; without it post is zeros.
The posteriors are UNWEIGHTED (the library's weight multiplies them).

A graph is the dict of synth.make_alignment_graph: {S, P, src, dst, pdf, logprob, init, final}, states numbered from 0."""
import numpy as np


def forward_backward(g, y, acoustic_scale=1.0):
    """y: [T, >= P] float32 rows of one utterance.  Returns dict(logprob, ok, post [T, P] float64)."""
    S, P = int(g["S"]), int(g["P"])
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    lp = np.asarray(g["logprob"], dtype=np.float32).astype(np.float64)
    init = np.asarray(g["init"], dtype=np.float32).astype(np.float64)
    final = np.asarray(g["final"], dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32)
    T = y.shape[0]
    scale = np.float64(np.float32(acoustic_scale))
    post = np.zeros((T, P))
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
                np.add.at(post[t], pdf[keep], np.exp(v[keep] - logprob))
                beta = np.full(S, -np.inf)
                keep = out > -np.inf
                np.logaddexp.at(beta, src[keep], out[keep])
    return dict(logprob=logprob, ok=ok, post=post)


def enumerate_paths(g, y, acoustic_scale=1.0):
    """The same by brute force for tiny cases: every arc sequence of length T that is a path from a state with init > -inf to one with
    final > -inf, its score summed in path order; logprob is the log-sum over the paths' scores (taken against their maximum), post[t, p]
    the sum of exp(score - logprob) over the paths whose arc at frame t carries pdf p.  Returns dict(logprob, ok, post, paths)."""
    import itertools
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    lp = np.asarray(g["logprob"], dtype=np.float32).astype(np.float64)
    init = np.asarray(g["init"], dtype=np.float32).astype(np.float64)
    final = np.asarray(g["final"], dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32)
    T, A, S, P = y.shape[0], len(src), int(g["S"]), int(g["P"])
    scale = np.float64(np.float32(acoustic_scale))
    scores, paths = [], []
    if T == 0:
        for s in range(S):
            if init[s] + final[s] > -np.inf:
                scores.append(init[s] + final[s])
                paths.append(())
    else:
        for path in itertools.product(range(A), repeat=T):
            if any(dst[path[t]] != src[path[t + 1]] for t in range(T - 1)):
                continue
            v = init[src[path[0]]]
            for t, a in enumerate(path):
                v = v + (lp[a] + scale * np.float64(y[t, pdf[a]]))
            v = v + final[dst[path[-1]]]
            if v > -np.inf:
                scores.append(v)
                paths.append(path)
    post = np.zeros((T, P))
    if not scores:
        return dict(logprob=-np.inf, ok=False, post=post, paths=0)
    scores = np.asarray(scores)
    m = scores.max()
    logprob = float(m + np.log(np.exp(scores - m).sum()))
    for v, path in zip(scores, paths):
        for t, a in enumerate(path):
            post[t, pdf[a]] += np.exp(v - logprob)
    return dict(logprob=logprob, ok=bool(np.isfinite(logprob)), post=post, paths=len(scores))
