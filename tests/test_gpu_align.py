"""-m gpu: best-path alignment (csrc/align.hip, include/tdnnf_hip.h "best-path alignment") against tests/viterbi_ref64.py.

Score, pdf-ids and states are compared BIT FOR BIT: the kernel's additions are IEEE double in the reference's order and a max is exact.
The only tolerance here is the cross-check with the numerator (1e-9 relative: two double sums of the same at most 2 T + 2 terms in
different orders)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from tests import chain_ref64 as R
from tests import viterbi_ref64 as V
from tests.gpu_util import Hip, dev, host, padded

pytestmark = pytest.mark.gpu
F = np.float32
NINF = -np.inf


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _stack(ys):
    return np.concatenate(ys) if ys else np.zeros((0, 1), F)


def _run(pkg, graphs, ys, utt_graph=None, scale=1.0, ag=None):
    """the call on the utterances' rows stacked (row_stride 1): per utterance (score, ok, pdfs, states), downloaded"""
    ag = ag or pkg.hipabi.AlignGraphs(graphs)
    frames = [len(y) for y in ys]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    pdfs, states, res = ag.best_path(dev(_stack(ys)), frames, rows, 1, utt_graph, scale, states=True)
    pdfs, states, res = host(pdfs), host(states), host(res)
    out, p0 = [], 0
    for u, T in enumerate(frames):
        out.append((res[u, 0], res[u, 1], pdfs[p0:p0 + T].copy(), states[p0 + u:p0 + u + T + 1].copy()))
        p0 += T
    return out


def _same(got, ref, what=""):
    score, ok, pdfs, states = got
    assert ok == (1.0 if ref["ok"] else 0.0), (what, ok, ref["ok"])
    assert score == ref["score"], (what, float(score).hex(), float(ref["score"]).hex())
    assert np.array_equal(pdfs, ref["pdfs"]), (what, pdfs, ref["pdfs"])
    assert np.array_equal(states, ref["states"]), (what, states, ref["states"])


def _check(pkg, graphs, ys, utt_graph=None, scale=1.0):
    graphs = [graphs] if isinstance(graphs, dict) else graphs
    got = _run(pkg, graphs, ys, utt_graph, scale)
    refs = []
    for u, y in enumerate(ys):
        gi = utt_graph[u] if utt_graph is not None else (0 if len(graphs) == 1 else u)
        refs.append(V.best_path(graphs[gi], y, scale))
        _same(got[u], refs[-1], "utterance %d" % u)
    return got, refs


def _check_is_path(g, got):
    """state_out describes a path of the graph: consecutive states joined by an arc that carries the reported pdf, from an initial state to a final one"""
    _, ok, pdfs, states = got
    assert ok == 1.0
    arcs = set(zip(g["src"].tolist(), g["dst"].tolist(), g["pdf"].tolist()))
    assert g["init"][states[0]] > NINF and g["final"][states[-1]] > NINF
    for t, p in enumerate(pdfs):
        assert (int(states[t]), int(states[t + 1]), int(p)) in arcs, (t, states[t], states[t + 1], p)


# ------------------------------------------------------------------------------------------------------------------------- transcript graphs
def _transcripts(pkg, P=40):
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, P, size=n).tolist() for n in (1, 5, 17)]
    return [pkg.synth.make_alignment_graph(seqs[0], num_pdfs=P, seed=1),
            pkg.synth.make_alignment_graph(seqs[1], optional=[1, 4], alternatives={2: [7, 8]}, num_pdfs=P, seed=2),
            pkg.synth.make_alignment_graph(seqs[2], optional=[0, 9], alternatives={3: [1], 16: [2, 3, 4]}, num_pdfs=P, seed=3)]


@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_mixed_call(pkg, hip, scale):
    """three different transcript graphs with utterances of 1, 7 and 40 frames in ONE call"""
    graphs = _transcripts(pkg)
    rng = np.random.default_rng(5)
    ys = [rng.standard_normal((T, 40)).astype(F) * 3 for T in (1, 7, 40)]
    got, refs = _check(pkg, graphs, ys, scale=F(scale))
    assert all(r["ok"] for r in refs)
    for g, r in zip(graphs, got):
        _check_is_path(g, r)
    # the same three graphs shared and reordered through utt_graph, six utterances
    ys6 = ys + [rng.standard_normal((T, 40)).astype(F) for T in (9, 3, 25)]
    _check(pkg, graphs, ys6, utt_graph=[0, 1, 2, 1, 0, 2], scale=F(scale))


@pytest.mark.parametrize("S", [64, 65, 1024, 1025])
def test_block_size_boundaries_cyclic(pkg, hip, S):
    """the workgroup has 64 threads up to 64 states, 256 up to 1024, 1024 above: the last graph of each size and the first of the next"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, 50, mean_out_degree=4.0, seed=S))
    assert pkg.hipabi.AlignGraphs(g).info()["num_states"] == S
    rng = np.random.default_rng(S)
    got, _ = _check(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (9, 4)])
    _check_is_path(g, got[0])


def test_block_size_boundary_transcript(pkg, hip):
    """a 65-state transcript graph (256 threads), accepted only from 64 frames on: 63 frames give no path, 70 a path"""
    rng = np.random.default_rng(3)
    g = pkg.synth.make_alignment_graph(rng.integers(0, 50, size=64).tolist(), num_pdfs=50, seed=4)
    assert g["S"] == 65
    got, refs = _check(pkg, g, [rng.standard_normal((T, 50)).astype(F) for T in (70, 63, 64)])
    assert [r["ok"] for r in refs] == [True, False, True]
    _check_is_path(g, got[0])


@pytest.mark.parametrize("S,deg", [(10, 70), (100, 300), (1100, 1100)])
def test_heavy_rows(pkg, hip, S, deg):
    """one state whose in-degree exceeds the workgroup size (64 / 256 / 1024 threads): a wave takes the row.  Integer-valued scores, so
    that many of the row's arcs tie and the merge of the lanes' results has to pick the first of the caller's order."""
    rng = np.random.default_rng(deg)
    heavy = S // 2
    src = np.concatenate([rng.integers(0, S, size=deg), np.arange(S), rng.integers(0, S, size=2 * S)]).astype(np.int32)
    dst = np.concatenate([np.full(deg, heavy), (np.arange(S) + 1) % S, rng.integers(0, S, size=2 * S)]).astype(np.int32)
    perm = rng.permutation(len(src))
    src, dst = src[perm], dst[perm]
    g = {"S": S, "P": 6, "src": src, "dst": dst, "pdf": rng.integers(0, 6, size=len(src)).astype(np.int32),
         "logprob": rng.integers(-2, 1, size=len(src)).astype(F), "init": np.zeros(S, F), "final": np.where(np.arange(S) == heavy, 0, NINF).astype(F)}  # (paths end in the heavy row: its back-pointer is followed)
    info = pkg.hipabi.AlignGraphs(g).info()
    assert info["max_in_degree"] >= deg and info["num_arcs"] == len(src)
    ys = [rng.integers(-1, 2, size=(T, 6)).astype(F) for T in (6, 3)]
    got, refs = _check(pkg, g, ys)
    assert refs[0]["ok"] and refs[0]["states"][-1] == heavy
    _check_is_path(g, got[0])


@pytest.mark.parametrize("S,P", [(30, 512), (30, 513), (100, 2048), (100, 2049)])
def test_row_staging_threshold(pkg, hip, S, P):
    """the LDS form keeps the frame's output row in LDS while a thread can carry its share in 8 registers -- up to 8 * 64 = 512 pdfs at
    64 threads, 8 * 256 = 2048 at 256 -- and gathers from global memory above: the last size of the one and the first of the other"""
    g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(S, P, mean_out_degree=6.0, seed=P))
    assert g["pdf"].max() > P - 40  # (pdfs near the end of the row are on arcs)
    rng = np.random.default_rng(P)
    got, _ = _check(pkg, g, [rng.standard_normal((T, P)).astype(F) for T in (7, 1, 2)])
    _check_is_path(g, got[0])


# ------------------------------------------------------------------------------------------------------------------------- free decode
def test_free_decode_both_forms(pkg, hip):
    den = pkg.synth.make_den_graph(H=300, P=50)
    g = pkg.synth.alignment_graph_from_den(den)
    ag = pkg.hipabi.AlignGraphs.from_den_graph(den)
    rng = np.random.default_rng(9)
    ys = [rng.standard_normal((30, 50)).astype(F) * 4 for _ in range(4)]
    refs = [V.best_path(g, y) for y in ys]
    res = {}
    for form in (1, 2):
        with pkg.hipabi.option("align_form", form):
            res[form] = _run(pkg, None, ys, utt_graph=[0, 0, 0, 0], ag=ag)
        for u in range(4):
            _same(res[form][u], refs[u], "form %d utterance %d" % (form, u))
            _check_is_path(g, res[form][u])
    for a, b in zip(res[1], res[2]):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # the workspace of the global form is larger by the two state vectors of every utterance
    with pkg.hipabi.option("align_form", 1):
        n1 = ag.workspace_bytes([0] * 4, [30] * 4)
    with pkg.hipabi.option("align_form", 2):
        n2 = ag.workspace_bytes([0] * 4, [30] * 4)
    assert n1 == 16 + 256 + 4 * 4 * 30 * 300 and n2 == n1 + 4 * 16 * 300


# ------------------------------------------------------------------------------------------------------------------------- ties
def test_ties_first_arc_of_the_callers_order(pkg, hip):
    rng = np.random.default_rng(21)
    S, A, P = 7, 60, 4
    g = {"S": S, "P": P, "src": rng.integers(0, S, size=A).astype(np.int32), "dst": rng.integers(0, S, size=A).astype(np.int32),
         "pdf": rng.integers(0, P, size=A).astype(np.int32), "logprob": rng.integers(-1, 1, size=A).astype(F),
         "init": np.zeros(S, F), "final": np.zeros(S, F)}
    y = rng.integers(0, 2, size=(12, P)).astype(F)
    (got,), (ref,) = _check(pkg, g, [y])
    # parallel arcs with equal scores: the first listed wins, and with the list permuted the permuted choice does
    perm = rng.permutation(A)
    gp = dict(g, src=g["src"][perm], dst=g["dst"][perm], pdf=g["pdf"][perm], logprob=g["logprob"][perm])
    (gotp,), (refp,) = _check(pkg, gp, [y])
    assert got[0] == gotp[0]  # the same best score
    assert not np.array_equal(perm[refp["arcs"]], ref["arcs"])  # (the case does have ties: the permuted list's choice is another path)
    # the smallest case, by hand
    two = {"S": 2, "P": 3, "src": np.asarray([0, 0, 1], np.int32), "dst": np.asarray([1, 1, 1], np.int32), "pdf": np.asarray([0, 1, 2], np.int32),
           "logprob": np.asarray([-1, -1, 0], F), "init": np.asarray([0, NINF], F), "final": np.asarray([NINF, 0], F)}
    (a,), _ = _check(pkg, two, [np.zeros((3, 3), F)])
    assert list(a[2]) == [0, 2, 2]
    swapped = dict(two, pdf=np.asarray([1, 0, 2], np.int32))
    (b,), _ = _check(pkg, swapped, [np.zeros((3, 3), F)])
    assert list(b[2]) == [1, 2, 2]
    # equal final states: the lowest
    fin = {"S": 3, "P": 3, "src": np.asarray([0, 0], np.int32), "dst": np.asarray([2, 1], np.int32), "pdf": np.asarray([0, 1], np.int32),
           "logprob": np.zeros(2, F), "init": np.asarray([0, NINF, NINF], F), "final": np.asarray([NINF, 0, 0], F)}
    (c,), _ = _check(pkg, fin, [np.zeros((1, 3), F)])
    assert list(c[3]) == [0, 1] and list(c[2]) == [1]


# ------------------------------------------------------------------------------------------------------------------------- hostile inputs
@pytest.mark.parametrize("family", ["peaky", "beyond"])
def test_hostile_inputs(pkg, hip, family):
    """the peaky and beyond-+-30 outputs of tests/chain_ref64.py, 150 frames: scores of 1e3 .. 1e4, still bit-equal; free decode on the
    denominator graph and forced alignment on the supervision's own graphs"""
    H, P, B, T = 40, 30, 2, 150
    den = R.graph(pkg, H, P)
    sup = pkg.synth.make_supervision_from_den(den, B, T, num_paths=2, seed=T)
    y = R.make_logits(family, sup, P)
    ys = [y[s::B] for s in range(B)]
    got, refs = _check(pkg, pkg.synth.alignment_graph_from_den(den), ys, utt_graph=[0, 0])
    print("ALIGN hostile %s: free-decode scores %s" % (family, [r["score"] for r in refs]))
    assert all(r["ok"] for r in refs)
    if family == "beyond":
        assert min(abs(r["score"]) for r in refs) > 3e3
    got, refs = _check(pkg, pkg.synth.alignment_graphs_from_supervision(sup), ys)
    assert all(r["ok"] for r in refs)
    # non-finite outputs are data too: a NaN or -inf is never a candidate, +inf makes the score +inf and ok 0
    bad = ys[0][:20].copy()
    bad[3, :] = np.nan
    bad[7, ::2] = NINF
    g = pkg.synth.alignment_graph_from_den(den)
    _, (r,) = _check(pkg, g, [bad])
    assert not r["ok"] and r["score"] == NINF  # (frame 3 admits no arc)
    bad[3, :] = 0.0
    bad[5, 1] = np.inf
    (gp,), (r,) = _check(pkg, g, [bad])
    assert gp[1] == 0.0 and gp[0] == np.inf and (gp[2] == -1).all()


# ------------------------------------------------------------------------------------------------------------------------- no accepting path
def test_no_accepting_path_leaves_neighbours_alone(pkg, hip):
    graphs = _transcripts(pkg)
    rng = np.random.default_rng(8)
    ys = [rng.standard_normal((T, 40)).astype(F) for T in (12, 2, 30)]  # graph 1 needs at least 3 frames
    got, refs = _check(pkg, graphs, ys)
    assert [r["ok"] for r in refs] == [True, False, True]
    assert got[1][0] == NINF and got[1][1] == 0.0 and (got[1][2] == -1).all() and (got[1][3] == -1).all()
    alone = _run(pkg, [graphs[0], graphs[2]], [ys[0], ys[2]])
    for a, b in zip(alone, (got[0], got[2])):
        assert a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_utterance_of_no_frames(pkg, hip):
    """zero frames: the score is the best initial + final, the path one state; on a transcript graph the start state is not final"""
    den = pkg.synth.make_den_graph(H=70, P=20, mean_out_degree=4.0, seed=6)
    g = pkg.synth.alignment_graph_from_den(den)
    rng = np.random.default_rng(2)
    ys = [np.zeros((0, 20), F), rng.standard_normal((5, 20)).astype(F), np.zeros((0, 20), F)]
    got, refs = _check(pkg, g, ys, utt_graph=[0, 0, 0])
    assert refs[0]["ok"] and got[0][0] == float(np.float64(g["init"].max())) and list(got[0][3]) == [int(np.argmax(g["init"]))]
    t = pkg.synth.make_alignment_graph([1, 2], num_pdfs=20)
    _, refs = _check(pkg, [t, g], ys, utt_graph=[0, 1, 0])
    assert [r["ok"] for r in refs] == [False, True, False]


# ------------------------------------------------------------------------------------------------------------------------- layouts, guards
def test_row_layouts_and_guard_elements(pkg, hip):
    """the same data concatenated (row_stride 1) and t-major (row_stride B) inside a view whose stride exceeds its columns; sentinels
    before and after pdf_out, state_out, results and the workspace (which starts 4 bytes off a 16-byte boundary)"""
    den = pkg.synth.make_den_graph(H=90, P=20, mean_out_degree=5.0, seed=2)
    g = pkg.synth.alignment_graph_from_den(den)
    ag = pkg.hipabi.AlignGraphs(g)
    rng = np.random.default_rng(4)
    B, frames = 3, [11, 5, 8]
    Tmax = max(frames)
    tmajor = rng.standard_normal((Tmax * B, 20)).astype(F)
    ys = [tmajor[u::B][:frames[u]] for u in range(B)]
    refs = [V.best_path(g, y) for y in ys]
    cat = _run(pkg, None, ys, ag=ag)
    view, buf = padded(tmajor)
    assert view.stride(0) > view.shape[1]
    total, G = sum(frames), 5
    fr, frp = pkg.hipabi.iarr(frames)
    rb, rbp = pkg.hipabi.iarr(np.arange(B))
    nbytes = ag.workspace_bytes(None, frames)
    pdf_buf = torch.full((total + 2 * G,), -77, dtype=torch.int32, device="cuda")
    st_buf = torch.full((total + B + 2 * G,), -78, dtype=torch.int32, device="cuda")
    res_buf = torch.full((2 * B + 2 * G,), -79.0, dtype=torch.float64, device="cuda")
    nws = (nbytes + 3) // 4
    ws_buf = torch.full((nws + 2 * G,), -80.0, dtype=torch.float32, device="cuda")
    pkg.hipabi.check(hip.lib.tdnnf_align_best_path(ag.h, B, None, frp, rbp, B, pkg.hipabi.pmat(view), 1.0, hip.vec(pdf_buf[G:]), hip.vec(st_buf[G:]),
                                                   hip.vec(res_buf[G:]), hip.vec(ws_buf[G:]), nbytes, hip.stream()))
    pdfs, states, res, ws = host(pdf_buf), host(st_buf), host(res_buf), host(ws_buf)
    for a, fill in ((pdfs, -77), (states, -78), (res, -79.0), (ws, -80.0)):
        assert (a[:G] == fill).all() and (a[-G:] == fill).all()
    assert (host(buf)[:, 20:] == 7.0).all()  # (the view's padding columns)
    p0 = 0
    for u, T in enumerate(frames):
        got = (res[G + 2 * u], res[G + 2 * u + 1], pdfs[G + p0:G + p0 + T], states[G + p0 + u:G + p0 + u + T + 1])
        _same(got, refs[u], "t-major utterance %d" % u)
        _same(cat[u], refs[u], "concatenated utterance %d" % u)
        p0 += T
    # state_out may be NULL
    pdf2 = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    ws2 = hip.ws(nbytes)
    pkg.hipabi.check(hip.lib.tdnnf_align_best_path(ag.h, B, None, frp, rbp, B, pkg.hipabi.pmat(view), 1.0, hip.vec(pdf2), None, hip.vec(res_buf[G:]),
                                                   hip.vec(ws2), nbytes, hip.stream()))
    assert np.array_equal(host(pdf2), pdfs[G:-G])


# ------------------------------------------------------------------------------------------------------------------------- the numerator
def _num_logprob(pkg, hip, den, sup, y):
    dg, ds = pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup)
    nb = hip.chain_objf_workspace_bytes(dg.h, ds.B, ds.T)
    ws = hip.ws(nb)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    hip.chain_objf(dg.h, ds.h, dev(y), None, 1e-5, 0.0, hip.vec(res), hip.vec(ws), nb, hip.stream())
    r = host(res)
    assert r[5] == 1.0
    return float(r[3])


def test_cross_check_with_the_numerator(pkg, hip):
    P, T = 30, 25
    den = pkg.synth.make_den_graph(20, P, mean_out_degree=3.0, seed=1)
    rng = np.random.default_rng(13)
    # one path per sequence: the best path IS the numerator's only path -- per sequence (B = 1) and summed over a minibatch (B = 3)
    for B, seed in ((1, 0), (1, 1), (3, 2)):
        sup = pkg.synth.make_supervision(B, T, P, max_alt=1, seed=seed)
        y = rng.standard_normal((T * B, P)).astype(F) * 2
        graphs = pkg.synth.alignment_graphs_from_supervision(sup)
        ag = pkg.hipabi.AlignGraphs(graphs, num_pdfs=P)
        _, _, res = ag.best_path(dev(y), [T] * B, np.arange(B), B)
        res = host(res)
        num = _num_logprob(pkg, hip, den, sup, y)
        print("ALIGN numerator cross-check B %d: best path %.17g numerator %.17g" % (B, res[:, 0].sum(), num))
        assert (res[:, 1] == 1.0).all() and abs(res[:, 0].sum() - num) <= 1e-9 * abs(num)
        for s in range(B):
            assert res[s, 0] == V.best_path(graphs[s], y[s::B])["score"]
    # a lattice: the best path is one of the paths the numerator sums
    for seed in (0, 1):
        sup = pkg.synth.make_supervision_lattice(1, T, P, tolerance=2, alternatives=2, seed=seed)
        y = rng.standard_normal((T, P)).astype(F) * 2
        graphs = pkg.synth.alignment_graphs_from_supervision(sup)
        (got,), (ref,) = _check(pkg, graphs, [y])
        num = _num_logprob(pkg, hip, den, sup, y)
        print("ALIGN lattice: best path %.17g numerator %.17g" % (got[0], num))
        assert ref["ok"] and got[0] <= num and got[0] > num - 40.0  # (and not absurdly far below: the lattice has far fewer than e^40 paths)


# ------------------------------------------------------------------------------------------------------------------------- the model
def test_acoustic_model_align_and_archive(pkg, hip, tmp_path):
    from tests.test_gpu_infer import FSF, SMALL, make_model, utterances
    cfg, net = make_model(pkg, SMALL)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    rng = np.random.default_rng(17)
    utts = utterances(rng, [50, 7, 95])
    outs = [-(-T // FSF) for T in (50, 7, 95)]
    P = cfg.num_pdfs
    graphs = [pkg.synth.make_alignment_graph(rng.integers(0, P, size=n).tolist(), optional=[1], num_pdfs=P, seed=n) for n in (6, 2, 40)]
    ag = pkg.hipabi.AlignGraphs(graphs)
    a = model.align(utts, ag, acoustic_scale=1.0)
    y = model.compute(utts)
    b = pkg.infer.align(y, ag, acoustic_scale=1.0)
    assert [len(x[0]) for x in a] == outs
    for u, (x, z) in enumerate(zip(a, b)):
        ref = V.best_path(graphs[u], host(y[u]))
        assert x[0].dtype == torch.int32 and x[0].is_cuda
        assert x[1] == z[1] == ref["score"] and x[2] == z[2] == ref["ok"]
        assert np.array_equal(host(x[0]), ref["pdfs"]) and np.array_equal(host(z[0]), ref["pdfs"])
    assert [x[2] for x in a] == [True, True, False]  # (32 output frames for a transcript of at least 39 units)
    # shared graph through utt_graph
    c = pkg.infer.align(y, ag, utt_graph=[0, 1, 0])
    assert c[2][2] and c[2][1] == V.best_path(graphs[0], host(y[2]))["score"]
    # archive round trip
    path = tmp_path / "ali.ark"
    pkg.infer.write_int_vector_archive(path, [("utt%d" % u, x[0]) for u, x in enumerate(a)] + [("empty", [])])
    data, pos, back = open(path, "rb").read(), 0, {}
    while pos < len(data):
        end = data.index(b" ", pos)
        key = data[pos:end].decode()
        assert data[end + 1:end + 3] == b"\0B" and data[end + 3] == 4
        n, = struct.unpack_from("<i", data, end + 4)
        back[key] = np.frombuffer(data, dtype="<i4", count=n, offset=end + 8)
        pos = end + 8 + 4 * n
    assert list(back) == ["utt0", "utt1", "utt2", "empty"] and len(back["empty"]) == 0
    for u, x in enumerate(a):
        assert np.array_equal(back["utt%d" % u], host(x[0]))


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, hip):
    lib = hip.lib
    Err = pkg.hipabi.HipAbiError
    ok = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5)
    with pytest.raises(Err, match="pdf"):
        pkg.hipabi.AlignGraphs(dict(ok, pdf=np.where(np.arange(len(ok["pdf"])) == 2, 5, ok["pdf"])), num_pdfs=5)
    with pytest.raises(Err, match="pdf"):  # (an epsilon arc in the usual encodings)
        pkg.hipabi.AlignGraphs(dict(ok, pdf=np.where(np.arange(len(ok["pdf"])) == 0, -1, ok["pdf"])), num_pdfs=5)
    with pytest.raises(Err, match="state"):
        pkg.hipabi.AlignGraphs(dict(ok, dst=np.where(np.arange(len(ok["dst"])) == 1, ok["S"], ok["dst"])), num_pdfs=5)
    with pytest.raises(Err, match="state"):  # a state of ANOTHER graph of the set
        pkg.hipabi.AlignGraphs([ok, dict(ok, src=np.where(np.arange(len(ok["src"])) == 1, -1, ok["src"]))], num_pdfs=5)
    with pytest.raises(Err, match="initial"):
        pkg.hipabi.AlignGraphs(dict(ok, init=np.full(ok["S"], NINF, F)), num_pdfs=5)
    with pytest.raises(Err, match="final"):
        pkg.hipabi.AlignGraphs(dict(ok, final=np.full(ok["S"], NINF, F)), num_pdfs=5)
    ag = pkg.hipabi.AlignGraphs(ok, num_pdfs=5)
    frames, rows = pkg.hipabi.iarr([4, 6]), pkg.hipabi.iarr([0, 4])
    y = dev(np.zeros((10, 5), F))
    nbytes = ag.workspace_bytes(None, [4, 6])
    assert nbytes == 16 + 256 + 4 * (4 + 6) * ok["S"]
    ws, pdf_out = hip.ws(nbytes), torch.full((10,), -5, dtype=torch.int32, device="cuda")
    res = torch.full((4,), -5.0, dtype=torch.float64, device="cuda")
    call = lambda y_, rows_, nb, stride=1: lib.tdnnf_align_best_path(ag.h, 2, None, frames[1], rows_[1], stride, pkg.hipabi.pmat(y_), 1.0, hip.vec(pdf_out),
                                                                     None, hip.vec(res), hip.vec(ws), nb, hip.stream())
    assert call(y, rows, nbytes - 1) == 1 and b"workspace" in lib.tdnnf_last_error()
    assert call(y, pkg.hipabi.iarr([0, 5]), nbytes) == 1 and b"rows" in lib.tdnnf_last_error()      # rows 5 .. 10 of 10
    assert call(y, pkg.hipabi.iarr([-1, 4]), nbytes) == 1 and b"rows" in lib.tdnnf_last_error()
    assert call(y, pkg.hipabi.iarr([0, 1]), nbytes, 2) == 1 and b"rows" in lib.tdnnf_last_error()   # t-major: 1 + 5 * 2 = row 11
    assert call(dev(np.zeros((10, 4), F)), rows, nbytes) == 1 and b"columns" in lib.tdnnf_last_error()
    assert (host(pdf_out) == -5).all() and (host(res) == -5.0).all()  # nothing was launched
    assert call(y, rows, nbytes) == 0
    assert (host(res)[[1, 3]] == 1.0).all()
    with pkg.hipabi.option("align_form", 3):
        assert call(y, rows, nbytes) == 1 and b"align_form" in lib.tdnnf_last_error()
