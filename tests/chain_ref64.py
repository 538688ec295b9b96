"""Float64 reference of the chain objective's two forward-backward passes, and the hostile inputs the chain tests run on (a helper module
like tests/view_layouts.py; pinned by tests/test_chain_ref64.py, used by tests/test_gpu_chain_hostile.py).

Plain numpy, one sequence at a time.  Nothing here shares a line with oracle/oracle_chain.c or the kernels: the denominator keeps BOTH
recursions normalised to sum 1 per frame and carries the scales as logs (so no value leaves the range of a double however peaky the
input), the numerator is log-domain throughout.

Row order of every matrix: row = t * B + s, columns = pdf-ids (as nnet_output)."""
import types

import numpy as np

F = np.float32


def den_forward_backward(g, y, B, leaky):
    """(log p_den per sequence [B], occupancies gamma_den [T * B, P]) of the leaky-HMM denominator on x = exp(clip(y, -30, 30)).

    alpha'(0) = init + leaky sum(init) init; alpha(t) = sum over arcs alpha'(t-1, src) prob x(t-1, pdf); alpha'(t) = alpha(t) +
    leaky sum(alpha(t)) init; total = sum alpha'(T).  beta'(T) = 1; beta(t) = beta'(t) + leaky <init, beta'(t)>; beta'(t, i) = sum over
    arcs from i of prob x(t, pdf) beta(t+1, dst).  gamma(t, pdf) = sum over arcs alpha'(t, src) prob x(t, pdf) beta(t+1, dst) / total --
    for EVERY element, clamped or not (Kaldi's derivative is gamma whatever ApplyExpLimited did to the element)."""
    H, P = int(g["H"]), int(g["P"])
    src, dst, pdf = (np.asarray(g[k], dtype=np.int64) for k in ("src", "dst", "pdf"))
    prob, init = np.asarray(g["prob"], dtype=np.float64), np.asarray(g["init"], dtype=np.float64)
    y = np.asarray(y)
    T = y.shape[0] // B
    assert y.shape == (T * B, P)
    x_all = np.exp(np.clip(y.astype(np.float64), -30.0, 30.0))
    logprob, gamma = np.zeros(B), np.zeros((T * B, P))
    for s in range(B):
        x = x_all[s::B]  # [T, P]
        w = prob[None, :] * x[:, pdf]  # arc weights of every frame [T, A]
        a = np.zeros((T + 1, H))  # alpha'(t) / its sum
        la = np.zeros(T + 1)  # log of what a[t] was divided by, cumulative
        v = init + leaky * init.sum() * init
        la[0] = np.log(v.sum())
        a[0] = v / v.sum()
        for t in range(1, T + 1):
            v = np.bincount(dst, weights=a[t - 1, src] * w[t - 1], minlength=H)
            v = v + leaky * v.sum() * init
            la[t] = la[t - 1] + np.log(v.sum())
            a[t] = v / v.sum()
        logprob[s] = la[T]  # (sum of a[T] is 1)
        b = np.full(H, 1.0 + leaky * init.sum())  # beta(T)
        lb = 0.0
        for t in range(T - 1, -1, -1):
            arc = w[t] * b[dst]
            # alpha'(t, src) arc / total with the scales put back: exp(la[t] + lb - la[T])
            gamma[t * B + s] = np.bincount(pdf, weights=a[t, src] * arc, minlength=P) * np.exp(la[t] + lb - la[T])
            v = np.bincount(src, weights=arc, minlength=H)
            v = v + leaky * float(init @ v)
            n = v.sum()
            lb += np.log(n)
            b = v / n
    return logprob, gamma


def num_forward_backward(sup, y):
    """(log p_num per sequence [B], UNWEIGHTED posteriors gamma_num [T * B, P]) of the supervision's time-synchronous graphs, log-domain on
    the raw y: the numerator applies no clamp."""
    B, T = int(sup["B"]), int(sup["T"])
    y = np.asarray(y).astype(np.float64)
    st, fin = np.asarray(sup["state_time"]), np.asarray(sup["final_logprob"], dtype=np.float64)
    a_src, a_dst, a_pdf = np.asarray(sup["arc_src"]), np.asarray(sup["arc_dst"]), np.asarray(sup["arc_pdf"])
    a_lp = np.asarray(sup["arc_logprob"], dtype=np.float64)
    logprob, post = np.zeros(B), np.zeros_like(y)
    for s in range(B):
        s0, s1 = int(sup["seq_state_begin"][s]), int(sup["seq_state_begin"][s + 1])
        a0, a1 = int(sup["seq_arc_begin"][s]), int(sup["seq_arc_begin"][s + 1])
        src, dst, pdf = a_src[a0:a1] - s0, a_dst[a0:a1] - s0, a_pdf[a0:a1]
        t_arc = st[a_src[a0:a1]]
        ll = a_lp[a0:a1] + y[t_arc * B + s, pdf]
        la, lb = np.full(s1 - s0, -np.inf), fin[s0:s1].copy()
        la[0] = 0.0
        by_t = [np.nonzero(t_arc == t)[0] for t in range(T)]
        for t in range(T):  # states are sorted by time and arcs go from t to t + 1: frame by frame
            for k in by_t[t]:
                la[dst[k]] = np.logaddexp(la[dst[k]], la[src[k]] + ll[k])
        tot = -np.inf
        for i in np.nonzero(fin[s0:s1] > -np.inf)[0]:
            tot = np.logaddexp(tot, la[i] + fin[s0 + i])
        for t in range(T - 1, -1, -1):
            for k in by_t[t]:
                lb[src[k]] = np.logaddexp(lb[src[k]], ll[k] + lb[dst[k]])
        logprob[s] = tot
        np.add.at(post, (t_arc * B + s, pdf), np.exp(la[src] + ll + lb[dst] - tot))
    return logprob, post


# ---------------------------------------------------------------------------------------------------------------- hostile inputs
FAMILIES = ("peaky", "beyond", "long-peaky")


def supervision_pdfs(sup, s, t):
    """pdf-ids on the arcs of sequence s that leave a state of time t"""
    a0, a1 = int(sup["seq_arc_begin"][s]), int(sup["seq_arc_begin"][s + 1])
    k = np.nonzero(np.asarray(sup["state_time"])[np.asarray(sup["arc_src"][a0:a1])] == t)[0]
    return np.asarray(sup["arc_pdf"][a0:a1])[k]


def make_logits(family, sup, P, seed=0):
    """nnet_output [T * B, P] float32 of one family:
    peaky / long-peaky  N(-8, 2^2) with one pdf per row raised by 25 -- for about half the rows a pdf of that frame's supervision (the
                        numerator then sees dominant paths and buried ones), else any pdf: what a trained chain net gives, the recursions
                        carry 10-25 decades per frame;
    beyond              N(0, 25^2): about 23 % of the elements outside the +-30 of ApplyExpLimited."""
    assert family in FAMILIES
    B, T = int(sup["B"]), int(sup["T"])
    rng = np.random.default_rng([seed, FAMILIES.index(family), B, T, P])
    if family == "beyond":
        return (rng.standard_normal((T * B, P)) * 25.0).astype(F)
    y = -8.0 + 2.0 * rng.standard_normal((T * B, P))
    for t in range(T):
        for s in range(B):
            on_path = rng.random() < 0.5
            pdfs = supervision_pdfs(sup, s, t)
            p = int(rng.choice(pdfs)) if on_path else int(rng.integers(0, P))
            y[t * B + s, p] += 25.0
    return y.astype(F)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


_graphs, _cases = {}, {}


def graph(pkg, H, P):
    if (H, P) not in _graphs:
        _graphs[(H, P)] = pkg.synth.make_den_graph(H, P, mean_out_degree=4.0, seed=H)
    return _graphs[(H, P)]


def make_case(pkg, ora, family, H, P, B, T, leaky, seed=0):
    """One hostile case with everything the tests compare against, computed once: the float64 reference, the oracle's results on the same input,
    and the oracle's own distance from the reference (what f32 alpha with double accumulation costs on this input).  Cached; its arrays are
    shared between tests and read-only.  Asserts that the oracle itself copes with the input (ok == 1): a change of seed must not silently
    produce a case that the reference side fails."""
    import ctypes as C
    key = (family, H, P, B, T, float(leaky), seed)
    if key in _cases:
        return _cases[key]
    c = types.SimpleNamespace()
    c.family, c.H, c.P, c.B, c.T, c.leaky = family, H, P, B, T, leaky
    c.g = graph(pkg, H, P)
    c.sup = pkg.synth.make_supervision_from_den(c.g, B, T, num_paths=2, seed=T + seed, weight=1.0)
    c.y = make_logits(family, c.sup, P, seed)
    c.den_lp, c.den_gamma = den_forward_backward(c.g, c.y, B, leaky)
    c.num_lp, c.num_post = num_forward_backward(c.sup, c.y)
    L = ora.lib()
    gs, ss = ora.den_graph_struct(c.g), ora.supervision_struct(c.sup)
    objf, l2t, w = C.c_double(), C.c_double(), C.c_double()
    c.d_ora, c.xd_ora = np.zeros_like(c.y), np.zeros_like(c.y)
    ok = L.oracle_chain_objf_and_deriv(C.byref(gs), C.byref(ss), ora.omat(c.y), leaky, 0.0, 0.1, C.byref(objf), C.byref(l2t), C.byref(w),
                                       ora.omat(c.d_ora), ora.omat(c.xd_ora))
    assert ok == 1, "the oracle fails on %s: choose another seed" % (key,)
    c.objf_ora, c.weight = objf.value, w.value
    den = C.c_double()
    c.gamma_ora = np.zeros_like(c.y)
    assert L.oracle_chain_denominator(C.byref(gs), ora.omat(c.y), B, leaky, 1.0, C.byref(den), ora.omat(c.gamma_ora)) == 1
    c.den_ora = den.value
    c.num_ora = L.oracle_chain_numerator(C.byref(ss), ora.omat(c.y), None)
    # the oracle against float64 on this input
    c.ora_gamma_rel = rel_l2(c.gamma_ora, c.den_gamma)
    c.ora_lp_rel = abs(c.den_ora - c.den_lp.sum()) / abs(c.den_lp.sum())
    c.ora_frame_sum = float(np.abs(c.gamma_ora.astype(np.float64).sum(1) - 1.0).max())
    # its largest single occupancy error, formed as the tests form the device's: posteriors minus derivative
    c.ora_gamma_maxabs = float(np.abs((c.xd_ora.astype(np.float64) - c.d_ora) - c.den_gamma).max())
    c.ora_post_maxabs = float(np.abs(c.xd_ora - c.num_post).max())
    for a in (c.y, c.den_lp, c.den_gamma, c.num_lp, c.num_post, c.d_ora, c.xd_ora, c.gamma_ora):
        a.setflags(write=False)
    _cases[key] = c
    return c
