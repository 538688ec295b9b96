"""CPU: synth.make_supervision_lattice -- tolerance lattices of any width as numerator supervisions.  The generator's structural
properties, the CPU oracle's numerator on such a lattice against brute-force path enumeration (the method of
test_oracle_chain_optim.py), and the archive round trip."""
import ctypes as C
import itertools

import numpy as np
import torch

F = np.float32


def _per_frame(sup):
    B, T = sup["B"], sup["T"]
    per = np.zeros((B, T + 1), np.int64)
    for b in range(B):
        per[b] = np.bincount(sup["state_time"][sup["seq_state_begin"][b]:sup["seq_state_begin"][b + 1]], minlength=T + 1)
    return per


def _check_structure(sup):
    B, T = sup["B"], sup["T"]
    st, ssb, sab = sup["state_time"], sup["seq_state_begin"], sup["seq_arc_begin"]
    src, dst = sup["arc_src"], sup["arc_dst"]
    assert len(ssb) == B + 1 and len(sab) == B + 1 and ssb[-1] == len(st) and sab[-1] == len(src)
    for b in range(B):
        t = st[ssb[b]:ssb[b + 1]]
        assert t[0] == 0 and (t[1:] > 0).all() and (np.diff(t) >= 0).all() and t.max() == T  # start first, sorted by time
        a = slice(sab[b], sab[b + 1])
        assert (src[a] >= ssb[b]).all() and (src[a] < ssb[b + 1]).all() and (dst[a] >= ssb[b]).all() and (dst[a] < ssb[b + 1]).all()
    assert (st[dst] == st[src] + 1).all()  # every arc goes t -> t + 1
    fin = np.isfinite(sup["final_logprob"])
    assert fin.any() and (st[fin] == T).all()  # finals only at T
    assert (sup["arc_pdf"] >= 0).all() and (sup["arc_logprob"] <= 0).all() and (sup["arc_logprob"] > -0.5001).all()
    # every state is on a path from its sequence's start to a final state
    acc = np.zeros(len(st), bool)
    acc[ssb[:-1]] = True
    co = fin.copy()
    t_src = st[src]
    for t in range(T):
        m = (t_src == t) & acc[src]
        acc[dst[m]] = True
    for t in range(T - 1, -1, -1):
        m = (t_src == t) & co[dst]
        co[src[m]] = True
    assert acc.all() and co.all(), (int(acc.sum()), int(co.sum()), len(st))


def test_generator_structure(pkg):
    for kw in [dict(B=4, T=30, P=40), dict(B=3, T=8, P=20, alternatives=3), dict(B=130, T=4, P=90, alternatives=5), dict(B=2, T=20, P=200, alternatives=24),
               dict(B=2, T=5, P=7, tolerance=0), dict(B=1, T=1, P=3), dict(B=2, T=40, P=50, tolerance=4, mean_dur=5.0, alternatives=2)]:
        sup = pkg.synth.make_supervision_lattice(seed=7, **kw)
        assert sup["B"] == kw["B"] and sup["T"] == kw["T"] and sup["arc_pdf"].max() < kw["P"]
        _check_structure(sup)
    # tolerance 0, one alternative: a single path
    one = pkg.synth.make_supervision_lattice(2, 9, 11, tolerance=0, seed=1)
    assert (_per_frame(one) == 1).all() and len(one["arc_src"]) == 2 * 9


def test_generator_width(pkg):
    """Over the cap of 4 states per frame the kernel entry used to refuse at the default parameters; over 64 in a frame with 24 alternatives."""
    sup = pkg.synth.make_supervision_lattice(4, 500, 600)
    B, T = sup["B"], sup["T"]
    assert len(sup["state_time"]) / (B * T) > 4.0
    assert len(sup["state_time"]) > B * 4 * (T + 1)  # what the library calls wide
    wide = pkg.synth.make_supervision_lattice(2, 20, 200, alternatives=24)
    assert _per_frame(wide).max() > 64
    assert _per_frame(pkg.synth.make_supervision_lattice(2, 20, 200, alternatives=100)).max() > 256


def test_generator_is_deterministic_per_seed(pkg):
    a = pkg.synth.make_supervision_lattice(3, 25, 30, alternatives=2, seed=5, weight=0.5)
    b = pkg.synth.make_supervision_lattice(3, 25, 30, alternatives=2, seed=5, weight=0.5)
    c = pkg.synth.make_supervision_lattice(3, 25, 30, alternatives=2, seed=6, weight=0.5)
    assert a["weight"] == 0.5 and set(a) == set(pkg.synth.make_supervision(1, 2, 3))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["arc_pdf"]) != len(c["arc_pdf"]) or not np.array_equal(a["arc_pdf"], c["arc_pdf"])
    for k, dt in [("seq_state_begin", np.int32), ("state_time", np.int32), ("arc_src", np.int32), ("arc_pdf", np.int32), ("arc_logprob", F), ("final_logprob", F)]:
        assert a[k].dtype == dt, k


def test_oracle_numerator_on_a_lattice_vs_brute_force(ora, pkg):
    L = ora.lib()
    B, T, P = 2, 5, 6
    sup = pkg.synth.make_supervision_lattice(B, T, P, tolerance=1, alternatives=2, mean_dur=2.0, seed=3)
    assert _per_frame(sup).max() >= 3
    rng = np.random.default_rng(2)
    y = rng.standard_normal((T * B, P)).astype(F)
    post = np.zeros_like(y)
    ss = ora.supervision_struct(sup)
    tot = L.oracle_chain_numerator(C.byref(ss), ora.omat(y), ora.omat(post))
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    total = 0
    for s in range(B):
        a0, a1 = sup["seq_arc_begin"][s], sup["seq_arc_begin"][s + 1]
        by_time = [[a for a in range(a0, a1) if sup["state_time"][sup["arc_src"][a]] == t] for t in range(T)]
        terms = []
        for path in itertools.product(*by_time):
            okp = sup["arc_src"][path[0]] == sup["seq_state_begin"][s] and np.isfinite(sup["final_logprob"][sup["arc_dst"][path[-1]]])
            for u, v in zip(path[:-1], path[1:]):
                okp = okp and sup["arc_dst"][u] == sup["arc_src"][v]
            if okp:
                terms.append(sum(float(sup["arc_logprob"][a]) + yt[sup["state_time"][sup["arc_src"][a]] * B + s, int(sup["arc_pdf"][a])] for a in path)
                             + float(sup["final_logprob"][sup["arc_dst"][path[-1]]]))
        assert len(terms) > 1
        total = total + torch.logsumexp(torch.stack(terms), 0)
    assert abs(tot - float(total.detach())) < 1e-5 * abs(float(total.detach()))
    total.backward()
    np.testing.assert_allclose(post, yt.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(post.sum(1), 1.0, rtol=1e-4)


def test_archive_round_trip(pkg, tmp_path):
    """egs writer -> reader -> merge gives the generator's arrays back."""
    E = pkg.egs
    B, T, P, ctx = 3, 8, 20, 5
    sup = pkg.synth.make_supervision_lattice(B, T, P, alternatives=3, seed=4)
    rng = np.random.default_rng(0)
    rows = 3 * T + 2 * ctx
    feats = [rng.standard_normal((rows, 6)).astype(F) for _ in range(B)]
    path = tmp_path / "lattice.ark"
    with E.Writer(path) as w:
        for b in range(B):
            w.write("utt%d" % b, feats[b], -ctx, E.sequence_of(sup, b), P, compress=False)
    egs = list(E.Reader(path))
    for b, e in enumerate(egs):
        info = e.supervision_info()
        assert info["num_states"] == sup["seq_state_begin"][b + 1] - sup["seq_state_begin"][b]
        assert info["num_arcs"] == sup["seq_arc_begin"][b + 1] - sup["seq_arc_begin"][b]
    _, _, s = E.merge(egs, -ctx, rows, with_ivectors=False)
    for k in ("seq_state_begin", "seq_arc_begin", "state_time", "arc_src", "arc_dst", "arc_pdf", "final_logprob", "arc_logprob"):
        assert np.array_equal(s[k], sup[k]), k
    assert s["weight"] == 1.0 and s["B"] == B and s["T"] == T
