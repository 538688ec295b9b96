"""-m gpu: forward-backward over pdf-labelled graphs (csrc/align_fb.hip, include/tdnnf_hip.h "forward-backward") against
tests/posteriors_ref64.py, on the shapes of tests/test_gpu_align.py (the same boundaries decide the code path).

Bars (the order of a sum is the library's, so nothing here is bit for bit against the reference):
    logprob   1e-9 relative: the bar tests/test_gpu_align.py uses for double sums taken in another order;
    post      |post - float32(weight * gamma_ref)| <= 2^-23 * weight: one float32 ulp at `weight` -- the output is a float rounded once
              from a double whose error is orders below that;
    row sums  every row of an accepted utterance sums to weight within 1e-6 * weight (summed in float64).
The reference's own reordering noise (tests/test_posteriors_ref64.py, test_reordering_noise) stays below 1e-15 relative / 2e-12 absolute on
every family run here, the hostile ones included, so these bars stand as stated.  One case has a floor under the relative logprob bar:
the zero-frame utterance on a denominator graph, whose logprob is log 1 up to rounding -- ten times the reference's own noise there
(test_utterance_of_no_frames says how it was measured).  Between two calls, between the two forms (option align_form) and between the
call with and without a posterior matrix, results ARE compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import chain_ref64 as R
from tests import posteriors_ref64 as PR
from tests.gpu_util import Hip, dev, host, padded

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf
ULP = 2.0 ** -23
FILL = -3.0  # what post_out holds before a call


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _stack(ys):
    return np.concatenate(ys) if ys else np.zeros((0, 1), F)


def _run(pkg, graphs, ys, utt_graph=None, scale=1.0, weight=1.0, ag=None, post=True):
    """the call on the utterances' rows stacked (row_stride 1): per utterance (logprob, ok, post [T, P] or None), downloaded"""
    ag = ag or pkg.hipabi.AlignGraphs(graphs)
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    y = dev(_stack(ys))
    if post:
        out = torch.full((max(sum(frames), 1), ag.P), FILL, dtype=torch.float32, device="cuda")
        p, res = ag.posteriors(y, frames, rows, 1, utt_graph, scale, weight, out=out)
        p = host(p)
    else:
        p, res = None, ag.logprob(y, frames, rows, 1, utt_graph, scale)
    res = host(res)
    return [(res[u, 0], res[u, 1], p[rows[u]:rows[u] + T].copy() if post else None) for u, T in enumerate(frames)]


def _close(got, ref, weight=1.0, what="", lp_floor=0.0):
    """lp_floor: an absolute floor under the logprob bar, for the one case whose logprob is 0 up to rounding (test_utterance_of_no_frames)"""
    lp, ok, post = got
    w = float(F(weight))
    assert ok == (1.0 if ref["ok"] else 0.0), (what, ok, lp, ref["logprob"])
    if np.isfinite(ref["logprob"]):
        assert abs(lp - ref["logprob"]) <= max(1e-9 * abs(ref["logprob"]), lp_floor), (what, lp, ref["logprob"])
    else:
        assert lp == ref["logprob"], (what, lp, ref["logprob"])
    if post is None:
        return
    P = ref["post"].shape[1]
    assert post.shape[1] == P or (post[:, P:] == 0).all(), what  # (pdfs beyond the utterance's own graph: no arc names them)
    want = (w * ref["post"]).astype(F)
    err = np.abs(post[:, :P].astype(np.float64) - want).max(initial=0.0)
    assert err <= ULP * w, (what, err)
    if ref["ok"] and len(post):
        assert np.abs(post.sum(1, dtype=np.float64) - w).max() <= 1e-6 * w, what
    if not ref["ok"]:
        assert (post == 0).all(), what


def _check(pkg, graphs, ys, utt_graph=None, scale=1.0, weight=1.0, lp_floor=0.0):
    graphs = [graphs] if isinstance(graphs, dict) else graphs
    got = _run(pkg, graphs, ys, utt_graph, scale, weight)
    refs = []
    for u, y in enumerate(ys):
        gi = utt_graph[u] if utt_graph is not None else (0 if len(graphs) == 1 else u)
        refs.append(PR.forward_backward(graphs[gi], y, scale))
        _close(got[u], refs[-1], weight, "utterance %d" % u, lp_floor if len(y) == 0 else 0.0)
    return got, refs


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, z in zip(a, b):
        assert np.array_equal(np.asarray(x[:2]).view(np.int64), np.asarray(z[:2]).view(np.int64))
        if x[2] is not None and z[2] is not None:
            assert np.array_equal(x[2].view(np.int32), z[2].view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------- transcript graphs
def _transcripts(pkg, P=40):
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, P, size=n).tolist() for n in (1, 5, 17)]
    return [pkg.synth.make_alignment_graph(seqs[0], num_pdfs=P, seed=1),
            pkg.synth.make_alignment_graph(seqs[1], optional=[1, 4], alternatives={2: [7, 8]}, num_pdfs=P, seed=2),
            pkg.synth.make_alignment_graph(seqs[2], optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]}, num_pdfs=P, seed=3)]


@pytest.mark.parametrize("scale,weight", [(1.0, 1.0), (0.3, 1.0), (1.0, 0.25), (0.3, 0.25)])
def test_mixed_call(pkg, hip, scale, weight):
    """three different transcript graphs with utterances of 1, 7 and 40 frames in ONE call"""
    graphs = _transcripts(pkg)
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in (1, 7, 40)]
    _, refs = _check(pkg, graphs, ys, scale=F(scale), weight=F(weight))
    assert all(r["ok"] for r in refs)
    # the same three graphs shared and reordered through utt_graph, six utterances
    ys6 = ys + [rng.standard_normal((T, 40)).astype(F) for T in (9, 3, 25)]
    _check(pkg, graphs, ys6, utt_graph=[0, 1, 2, 1, 0, 2], scale=F(scale), weight=F(weight))


@pytest.mark.parametrize("S", [64, 65, 1024, 1025])
def test_block_size_boundaries_cyclic(pkg, hip, S):
    """the workgroup has 64 threads up to 64 states, 256 up to 1024, 1024 above: the last graph of each size and the first of the next"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=4.0, seed=S))
    rng = np.random.default_rng(S)
    _, refs = _check(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (9, 4)])
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("S,deg", [(10, 70), (100, 300)])
def test_heavy_destination_rows(pkg, hip, S, deg):
    """one state whose in-degree exceeds 64 (and, at deg 300, the 256 threads): a wave takes the row and merges its (m, sum) pairs; with
    6 pdfs on some hundred arcs the pdf rows of the second case are heavy too"""
    rng = np.random.default_rng(deg)
    heavy = S // 2
    src = np.concatenate([rng.integers(0, S, size=deg), np.arange(S), rng.integers(0, S, size=2 * S)]).astype(np.int32)
    dst = np.concatenate([np.full(deg, heavy), (np.arange(S) + 1) % S, rng.integers(0, S, size=2 * S)]).astype(np.int32)
    perm = rng.permutation(len(src))
    src, dst = src[perm], dst[perm]
    g = {"S": S, "P": 6, "src": src, "dst": dst, "pdf": rng.integers(0, 6, size=len(src)).astype(np.int32),
         "logprob": (-rng.random(len(src)) * 2).astype(F), "init": np.zeros(S, F), "final": np.where(np.arange(S) == heavy, 0, NINF).astype(F)}
    assert pkg.hipabi.AlignGraphs(g).info()["max_in_degree"] >= deg
    ys = [rng.standard_normal((T, 6)).astype(F) for T in (6, 3)]
    _, refs = _check(pkg, g, ys)
    assert all(r["ok"] for r in refs)


def test_heavy_source_and_pdf_rows(pkg, hip):
    """one state with more than 64 outgoing arcs (a wave takes its beta row) and one pdf on more than 64 arcs (a wave takes its
    posterior and sums the lanes' shares by butterfly), beside light rows of both kinds"""
    rng = np.random.default_rng(77)
    S, P, fan, hub = 40, 9, 100, 3
    src = np.concatenate([np.full(fan, hub), rng.integers(0, S, size=90), np.arange(S)]).astype(np.int32)
    dst = np.concatenate([rng.integers(0, S, size=fan), rng.integers(0, S, size=90), (np.arange(S) + 1) % S]).astype(np.int32)
    pdf = np.concatenate([rng.integers(1, P, size=fan), np.zeros(90, np.int64), rng.integers(1, P, size=S)]).astype(np.int32)
    perm = rng.permutation(len(src))
    g = {"S": S, "P": P, "src": src[perm], "dst": dst[perm], "pdf": pdf[perm], "logprob": (-rng.random(len(src))).astype(F),
         "init": np.where(np.arange(S) % 5 == 0, -0.5, NINF).astype(F), "final": np.where(np.arange(S) % 3 == 0, -0.25, NINF).astype(F)}
    assert np.bincount(g["src"], minlength=S)[hub] > 64 and np.bincount(g["pdf"], minlength=P)[0] > 64
    assert np.bincount(g["pdf"], minlength=P)[1:].max() <= 64 and np.bincount(g["dst"], minlength=S).max() <= 64
    _, refs = _check(pkg, g, [rng.standard_normal((T, P)).astype(F) * 2 for T in (8, 2)], weight=F(0.25))
    assert all(r["ok"] for r in refs)


@pytest.mark.parametrize("S,P", [(30, 512), (30, 513), (100, 2048), (100, 2049)])
def test_row_staging_threshold(pkg, hip, S, P):
    """the LDS form keeps the frame's output row in LDS while a thread can carry its share in 8 registers -- up to 8 * 64 = 512 pdfs at
    64 threads, 8 * 256 = 2048 at 256 -- and gathers from global memory above: the last size of the one and the first of the other"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=6.0, seed=P))
    assert g["pdf"].max() > P - 40  # (pdfs near the end of the row are on arcs)
    rng = np.random.default_rng(P)
    ys = [rng.standard_normal((T, P)).astype(F) for T in (7, 1, 2)]
    got, _ = _check(pkg, g, ys)
    _same_bits([(a, b, None) for a, b, _ in got], _run(pkg, g, ys, post=False))  # (the forward-only launch forms at the same thresholds)


@pytest.mark.parametrize("S", [6400, 6401, 9600, 9601])
def test_state_vector_thresholds(pkg, hip, S):
    """150 KiB of LDS hold three vectors of doubles (the two state vectors and alpha_t, staged for the posterior step) up to 6 400
    states and two up to 9 600: above 6 400 the posterior step gathers alpha_t from the workspace, above 9 600 the state vectors lie
    there too (option align_form 0, by size).  The last graph of each kind and the first of the next."""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=3.0, seed=S))
    rng = np.random.default_rng(S)
    ys = [rng.standard_normal((T, 50)).astype(F) for T in (3, 2)]
    got, refs = _check(pkg, g, ys)
    assert all(r["ok"] for r in refs)
    _same_bits([(a, b, None) for a, b, _ in got], _run(pkg, g, ys, post=False))
    ag = pkg.hipabi.AlignGraphs(g)
    vectors = 2 * 16 * S if S > 9600 else 0  # (the workspace form's two vectors per utterance)
    assert ag.posteriors_workspace_bytes(None, [3, 2]) == 16 + 256 + 8 * (4 + 3) * S + vectors


# ------------------------------------------------------------------------------------------------------------------------- forms
def test_both_forms_and_logprob_only(pkg, hip):
    den = pkg.synth.make_den_graph(H=300, P=50)
    g = pkg.synth.alignment_graph_from_den(den)
    ag = pkg.hipabi.AlignGraphs.from_den_graph(den)
    rng = np.random.default_rng(9)
    ys = [rng.standard_normal((30, 50)).astype(F) * 4 for _ in range(4)]
    refs = [PR.forward_backward(g, y) for y in ys]
    res, lp_only, nbytes = {}, {}, {}
    for form in (1, 2):
        with pkg.hipabi.option("align_form", form):
            res[form] = _run(pkg, None, ys, utt_graph=[0, 0, 0, 0], ag=ag)
            again = _run(pkg, None, ys, utt_graph=[0, 0, 0, 0], ag=ag)
            lp_only[form] = _run(pkg, None, ys, utt_graph=[0, 0, 0, 0], ag=ag, post=False)
            nbytes[form] = (ag.posteriors_workspace_bytes([0] * 4, [30] * 4), ag.posteriors_workspace_bytes([0] * 4, [30] * 4, False))
        for u in range(4):
            _close(res[form][u], refs[u], 1.0, "form %d utterance %d" % (form, u))
        _same_bits(res[form], again)  # two calls of one form
        _same_bits(res[form], lp_only[form])  # the forward recursion alone gives the same logprob bits
    _same_bits(res[1], res[2])  # the two forms
    # the workspace: the per-utterance table, alpha of every frame (posteriors only), the two vectors of every utterance (workspace form only)
    alpha = 8 * 4 * 31 * 300
    assert nbytes[1] == (16 + 256 + alpha, 16 + 256)
    assert nbytes[2] == (16 + 256 + alpha + 4 * 16 * 300, 16 + 256 + 4 * 16 * 300)


# ------------------------------------------------------------------------------------------------------------------------- hostile inputs
@pytest.mark.parametrize("family", ["peaky", "beyond"])
def test_hostile_inputs(pkg, hip, family):
    """the peaky and beyond-+-30 outputs of tests/chain_ref64.py, 150 frames, on the denominator graph and on the supervision's own graphs"""
    H, P, B, T = 40, 30, 2, 150
    den = R.graph(pkg, H, P)
    sup = pkg.synth.make_supervision_from_den(den, B, T, num_paths=2, seed=T)
    y = R.make_logits(family, sup, P)
    ys = [y[s::B] for s in range(B)]
    g = pkg.synth.alignment_graph_from_den(den)
    _, refs = _check(pkg, g, ys, utt_graph=[0, 0])
    print("POSTERIORS hostile %s: logprobs on the denominator graph %s" % (family, [r["logprob"] for r in refs]))
    assert all(r["ok"] for r in refs)
    _, refs = _check(pkg, pkg.synth.alignment_graphs_from_supervision(sup), ys)
    assert all(r["ok"] for r in refs)
    # non-finite outputs are data too: a NaN or -inf is never a candidate, +inf makes logprob +inf and ok 0
    bad = ys[0][:20].copy()
    bad[3, :] = np.nan
    bad[7, ::2] = NINF
    (gp,), (r,) = _check(pkg, g, [bad])
    assert not r["ok"] and gp[0] == NINF and gp[1] == 0.0 and (gp[2] == 0).all()  # (frame 3 admits no arc)
    bad[3, :] = 0.0
    (gp,), (r,) = _check(pkg, g, [bad])
    assert r["ok"] and gp[1] == 1.0 and (gp[2][7, ::2] == 0).all()  # the -inf columns are skipped, the rest carries the mass
    bad[5, 1] = np.inf
    (gp,), (r,) = _check(pkg, g, [bad])
    assert gp[1] == 0.0 and gp[0] == np.inf and (gp[2] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------- no accepting path
def test_no_accepting_path_leaves_neighbours_alone(pkg, hip):
    graphs = _transcripts(pkg)
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30)]  # graph 1 needs at least 3 frames
    got, refs = _check(pkg, graphs, ys)
    assert [r["ok"] for r in refs] == [True, False, True]
    assert got[1][0] == NINF and got[1][1] == 0.0 and got[1][2].shape == (2, 40) and (got[1][2] == 0).all()
    alone = _run(pkg, [graphs[0], graphs[2]], [ys[0], ys[2]])
    _same_bits(alone, [got[0], got[2]])


def test_utterance_of_no_frames(pkg, hip):
    """zero frames: logprob = LSE(init + final), no row; on a transcript graph the start state is not final.
    On the denominator graph init is the log of a distribution and every state is final at 0, so logprob = log(1) up to rounding:
    7.18e-9 in the reference, the sum of 70 terms near e^-4.  A bar relative to that remainder asks for more than a double sum holds:
    the reference itself moves by up to 2.58e-16 absolute (3.6e-8 relative) when its states are summed in another order (50 shuffles
    of the state order, measured on the CPU).  So for the zero-frame utterances of this graph, and for them only, the bar is ten times
    the reference's own noise, 2.6e-15 absolute, where 1e-9 relative is smaller; first run on the GPU: 1.44e-16 from the reference."""
    den = pkg.synth.make_den_graph(H=70, P=20, mean_out_degree=4.0, seed=6)
    g = pkg.synth.alignment_graph_from_den(den)
    rng = np.random.default_rng(2)
    ys = [np.zeros((0, 20), F), rng.standard_normal((5, 20)).astype(F), np.zeros((0, 20), F)]
    got, refs = _check(pkg, g, ys, utt_graph=[0, 0, 0], lp_floor=2.6e-15)
    init = g["init"].astype(np.float64)
    assert refs[0]["ok"] and abs(got[0][0] - np.log(np.exp(init).sum())) <= 1e-9 and got[0][2].shape == (0, 20)
    t = pkg.synth.make_alignment_graph([1, 2], num_pdfs=20)
    _, refs = _check(pkg, [t, g], ys, utt_graph=[0, 1, 0])  # (the zero-frame utterances are on the transcript graph here: -inf, compared exactly)
    assert [r["ok"] for r in refs] == [False, True, False]
    lp = _run(pkg, [t, g], ys, utt_graph=[0, 1, 0], post=False)
    assert [x[1] for x in lp] == [0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------------- layouts, guards
def test_row_layouts_and_guard_elements(pkg, hip):
    """the same data concatenated (row_stride 1) and t-major (row_stride B) inside views whose stride exceeds their columns; post_out has
    more columns than num_pdfs and more rows than the call uses; sentinels in everything the call must not touch: the padding columns
    and unused rows of post_out, before and after results and the workspace (which starts 4 bytes off a 16-byte boundary)"""
    den = pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2)
    g = pkg.synth.alignment_graph_from_den(den)
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(4)
    B, frames, P = 3, [11, 5, 8], 20
    Tmax = max(frames)
    tmajor = rng.standard_normal((Tmax * B, P)).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    refs = [PR.forward_backward(g, y) for y in ys]
    cat = _run(pkg, None, ys, ag=ag)
    view, buf = padded(tmajor)
    assert view.stride(0) > view.shape[1]
    G = 5
    fr, frp = pkg.hipabi.iarr(frames)
    rb, rbp = pkg.hipabi.iarr(np.arange(B))
    nbytes = ag.posteriors_workspace_bytes(None, frames)
    post_buf = torch.full((Tmax * B + 2, P + 7), -81.0, dtype=torch.float32, device="cuda")  # two more rows, seven more columns
    post_view = post_buf[:Tmax * B + 1, :P + 3]  # a view of P + 3 columns with stride P + 7
    res_buf = torch.full((2 * B + 2 * G,), -79.0, dtype=torch.float64, device="cuda")
    nws = (nbytes + 3) // 4
    ws_buf = torch.full((nws + 2 * G,), -80.0, dtype=torch.float32, device="cuda")
    pkg.hipabi.check(hip.lib.tdnnf_align_posteriors(ag.h, B, None, frp, rbp, B, pkg.hipabi.pmat(view), 1.0, 1.0, pkg.hipabi.pmat(post_view),
                                                    hip.vec(res_buf[G:]), hip.vec(ws_buf[G:]), nbytes, hip.stream()))
    post, res, ws = host(post_buf), host(res_buf), host(ws_buf)
    for a, fill in ((res, -79.0), (ws, -80.0)):
        assert (a[:G] == fill).all() and (a[-G:] == fill).all()
    assert (host(buf)[:, P:] == 7.0).all()  # (the input view's padding columns)
    assert (post[:, P:] == -81.0).all() and (post[Tmax * B:] == -81.0).all()  # columns >= num_pdfs and rows behind the call's
    for u, T in enumerate(frames):
        assert (post[u::B][T:Tmax, :] == -81.0).all()  # the rows of the frames this utterance does not have
        got = (res[G + 2 * u], res[G + 2 * u + 1], post[u::B][:T, :P])
        _close(got, refs[u], 1.0, "t-major utterance %d" % u)
        _close(cat[u], refs[u], 1.0, "concatenated utterance %d" % u)
        _same_bits([got], [cat[u]])
    # without a posterior matrix: results alone, in a workspace without the alpha region
    nb0 = ag.posteriors_workspace_bytes(None, frames, False)
    assert nbytes - nb0 == 8 * sum((T + 1) * 90 for T in frames)
    ws0 = torch.full(((nb0 + 3) // 4 + 2 * G,), -80.0, dtype=torch.float32, device="cuda")
    res0 = torch.full((2 * B + 2 * G,), -79.0, dtype=torch.float64, device="cuda")
    pkg.hipabi.check(hip.lib.tdnnf_align_posteriors(ag.h, B, None, frp, rbp, B, pkg.hipabi.pmat(view), 1.0, 1.0, None, hip.vec(res0[G:]),
                                                    hip.vec(ws0[G:]), nb0, hip.stream()))
    assert np.array_equal(host(res0).view(np.int64), res.view(np.int64))
    assert (host(ws0)[:G] == -80.0).all() and (host(ws0)[-G:] == -80.0).all()


# ------------------------------------------------------------------------------------------------------------------------- the numerator
def test_cross_check_with_the_numerator(pkg, hip):
    """on a supervision's own graphs the sum of the logprobs is the chain numerator's results[3]: each side within its own bar of its
    float64 reference -- this call 1e-9 relative, the numerator the 1e-4 relative of tests/test_gpu_num_lattice.py"""
    from tests.test_gpu_align import _num_logprob
    P, T = 30, 25
    den = pkg.synth.make_den_graph(20, P, mean_out_degree=3.0, seed=1)
    rng = np.random.default_rng(13)
    for kind, B, seed in (("plain", 3, 2), ("lattice", 1, 0), ("lattice", 2, 1)):
        sup = (pkg.synth.make_supervision(B, T, P, max_alt=2, seed=seed) if kind == "plain"
               else pkg.synth.make_supervision_lattice(B, T, P, tolerance=2, alternatives=2, seed=seed))
        y = rng.standard_normal((T * B, P)).astype(F) * 2
        graphs = pkg.synth.alignment_graphs_from_supervision(sup)
        ag = pkg.hipabi.AlignGraphs(graphs, num_pdfs=P)
        post, res = ag.posteriors(dev(y), [T] * B, np.arange(B), B)
        post, res = host(post), host(res)
        num = _num_logprob(pkg, hip, den, sup, y)
        ref_lp, ref_post = R.num_forward_backward(sup, y)
        print("POSTERIORS numerator cross-check %s B %d: forward-backward %.17g numerator %.17g float64 %.17g" % (kind, B, res[:, 0].sum(), num, ref_lp.sum()))
        assert (res[:, 1] == 1.0).all()
        assert abs(res[:, 0].sum() - ref_lp.sum()) <= 1e-9 * abs(ref_lp.sum())
        assert abs(num - ref_lp.sum()) <= 1e-4 * abs(ref_lp.sum())
        assert np.abs(post.astype(np.float64) - ref_post.astype(F)).max() <= ULP  # (t-major rows, as the numerator's)


# ------------------------------------------------------------------------------------------------------------------------- the model
def test_acoustic_model_posteriors_and_archive(pkg, hip, tmp_path):
    from tests.test_gpu_infer import FSF, SMALL, make_model, utterances
    cfg, net = make_model(pkg, SMALL)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    rng = np.random.default_rng(17)
    utts = utterances(rng, [50, 7, 95])
    outs = [-(-T // FSF) for T in (50, 7, 95)]
    P = cfg.num_pdfs
    graphs = [pkg.synth.make_alignment_graph(rng.integers(0, P, size=n).tolist(), optional=[1], num_pdfs=P, seed=n) for n in (6, 2, 40)]
    ag = pkg.hipabi.AlignGraphs(graphs)
    a = model.posteriors(utts, ag, acoustic_scale=1.0)
    lp = model.logprob(utts, ag, acoustic_scale=1.0)
    ali = model.align(utts, ag, acoustic_scale=1.0)
    y = model.compute(utts)
    b = pkg.infer.posteriors(y, ag, acoustic_scale=1.0)
    lp2 = pkg.infer.logprob(y, ag)
    assert [tuple(x[0].shape) for x in a] == [(o, P) for o in outs]
    for u, (x, z) in enumerate(zip(a, b)):
        ref = PR.forward_backward(graphs[u], host(y[u]))
        assert x[0].dtype == torch.float32 and x[0].is_cuda
        assert x[1] == z[1] == lp[u][0] == lp2[u][0] and x[2] == z[2] == lp[u][1] == lp2[u][1] == ref["ok"]
        assert np.array_equal(host(x[0]), host(z[0]))
        _close((x[1], 1.0 if x[2] else 0.0, host(x[0])), ref, 1.0, "utterance %d" % u)
        if x[2]:  # the pdf that align reports at each frame has a non-zero posterior, and the sum over paths is no less than the best path
            assert ali[u][2] and (host(x[0])[np.arange(outs[u]), host(ali[u][0])] > 0).all()
            assert x[1] >= ali[u][1] - 1e-9 * abs(ali[u][1])
    assert [x[2] for x in a] == [True, True, False]  # (32 output frames for a transcript of at least 39 units)
    # shared graph through utt_graph
    c = pkg.infer.posteriors(y, ag, utt_graph=[0, 1, 0], weight=0.5)
    ref = PR.forward_backward(graphs[0], host(y[2]))
    _close((c[2][1], 1.0, host(c[2][0])), ref, 0.5)
    # archive round trip
    path = tmp_path / "post.ark"
    items = [("utt%d" % u, x[0]) for u, x in enumerate(a)] + [("empty", np.zeros((0, P), F))]
    pkg.infer.write_posterior_archive(path, items, min_post=1e-4)
    back = pkg.infer.read_posterior_archive(path)
    assert list(back) == ["utt0", "utt1", "utt2", "empty"] and back["empty"] == []
    for u, x in enumerate(a):
        m = host(x[0])
        assert len(back["utt%d" % u]) == outs[u]
        for t, pairs in enumerate(back["utt%d" % u]):
            ids = np.nonzero(m[t] > 1e-4)[0]
            assert [p for p, _ in pairs] == ids.tolist() and np.array_equal(np.asarray([v for _, v in pairs], F), m[t, ids])
    assert all(len(pairs) == 0 for pairs in back["utt2"])  # (no accepting path: every posterior is 0)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, hip):
    lib = hip.lib
    ok = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5)
    ag = pkg.hipabi.AlignGraphs(ok, num_pdfs=5)
    frames, rows = pkg.hipabi.iarr([4, 6]), pkg.hipabi.iarr([0, 4])
    y = dev(np.zeros((10, 5), F))
    nbytes = ag.posteriors_workspace_bytes(None, [4, 6])
    assert nbytes == 16 + 256 + 8 * (5 + 7) * ok["S"]
    assert ag.posteriors_workspace_bytes(None, [4, 6], False) == 16 + 256
    assert ag.posteriors_workspace_bytes(None, [4, -1]) == 0 and ag.posteriors_workspace_bytes([0, 1], [4, 6]) == 0
    ws = hip.ws(nbytes)
    post = torch.full((10, 5), -5.0, dtype=torch.float32, device="cuda")
    res = torch.full((4,), -5.0, dtype=torch.float64, device="cuda")
    call = lambda y_, rows_, nb, stride=1, post_=post: lib.tdnnf_align_posteriors(ag.h, 2, None, frames[1], rows_[1], stride, pkg.hipabi.pmat(y_), 1.0, 1.0,
                                                                                  pkg.hipabi.pmat(post_), hip.vec(res), hip.vec(ws), nb, hip.stream())
    assert call(y, rows, nbytes - 1) == 1 and b"workspace" in lib.tdnnf_last_error()
    assert call(y, rows, 16 + 256) == 1 and b"workspace" in lib.tdnnf_last_error()  # (the log-prob-only size does not do with a post_out)
    assert call(y, pkg.hipabi.iarr([0, 5]), nbytes) == 1 and b"rows" in lib.tdnnf_last_error()      # rows 5 .. 10 of 10
    assert call(y, pkg.hipabi.iarr([-1, 4]), nbytes) == 1 and b"rows" in lib.tdnnf_last_error()
    assert call(y, pkg.hipabi.iarr([0, 1]), nbytes, 2) == 1 and b"rows" in lib.tdnnf_last_error()   # t-major: 1 + 5 * 2 = row 11
    assert call(dev(np.zeros((10, 4), F)), rows, nbytes) == 1 and b"columns" in lib.tdnnf_last_error()
    narrow = torch.full((10, 4), -5.0, dtype=torch.float32, device="cuda")
    assert call(y, rows, nbytes, post_=narrow) == 1 and b"post_out" in lib.tdnnf_last_error() and b"columns" in lib.tdnnf_last_error()
    short = torch.full((9, 5), -5.0, dtype=torch.float32, device="cuda")
    assert call(y, rows, nbytes, post_=short) == 1 and b"post_out" in lib.tdnnf_last_error() and b"rows" in lib.tdnnf_last_error()
    assert (host(post) == -5.0).all() and (host(res) == -5.0).all() and (host(narrow) == -5.0).all() and (host(short) == -5.0).all()  # nothing was launched
    assert call(y, rows, nbytes) == 0
    assert (host(res)[[1, 3]] == 1.0).all() and np.abs(host(post).sum(1, dtype=np.float64) - 1.0).max() <= 1e-6
    with pkg.hipabi.option("align_form", 3):
        assert call(y, rows, nbytes) == 1 and b"align_form" in lib.tdnnf_last_error()
        assert ag.posteriors_workspace_bytes(None, [4, 6]) == 0
