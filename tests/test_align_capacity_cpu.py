"""CPU: the bounds a reserved tdnnf_align_graphs allocates its tables at (tdnn-f_nas_amd/csrc/align_tables.h align_table_bound), built with
g++ as tests/test_align_tables_cpu.py builds the header, against the tables align_build_tables makes: no table of any set of graphs may
have more slots, heavy rows or arc entries than the bound for its graphs, rows and arcs, and the arc bound -- 63 * 64 padding entries a
graph -- is attained, so it is not merely generous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "align_tables.h"
static tdnnf::AlignHostTables T;
extern "C" void ac_build(int G, int P, const int *sb, const int *ab, const int *src, const int *dst, const int *pdf, const float *lp, const int *label) {
  T = tdnnf::AlignHostTables();
  tdnnf::align_build_tables(G, P, sb, ab, src, dst, pdf, lp, &T, true, label);
}
// out[0 .. 3): slots, heavy, arcs of table k (0 by_dst, 1 by_src, 2 by_pdf, 3 by_label); out[3]: the table's rows
extern "C" void ac_sizes(int k, long long *out) {
  const tdnnf::AlignHostTable &t = k == 0 ? T.by_dst : k == 1 ? T.by_src : k == 2 ? T.by_pdf : T.by_label;
  out[0] = (long long)t.slots.size(); out[1] = (long long)t.heavy.size(); out[2] = (long long)t.arcs.size();
  out[3] = k < 2 ? T.graphs.back().state0 + T.graphs.back().num_states : k == 2 ? (long long)T.col_pdfs.size() : (long long)T.col_labels.size();
}
extern "C" void ac_bound(long long G, long long rows, long long arcs, long long *out) {
  const tdnnf::AlignTableBound b = tdnnf::align_table_bound(G, rows, arcs);
  out[0] = b.slots; out[1] = b.heavy; out[2] = b.arcs;
}
extern "C" int ac_pad_per_graph() { return tdnnf::kAlignPadPerGraph; }
'''
P = 11


@pytest.fixture(scope="module")
def ac(tmp_path_factory):
    d = tmp_path_factory.mktemp("ac")
    (d / "ac.cc").write_text(SRC)
    so = str(d / "libac.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), str(d / "ac.cc"), "-o", so])
    return C.CDLL(so)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def in_degrees(lengths, seed):
    """state i has lengths[i] incoming arcs; pdfs and labels at random (so by_pdf and by_label get rows of their own lengths)"""
    rng = np.random.default_rng(seed)
    S = len(lengths)
    dst = np.repeat(np.arange(S), lengths)
    src = rng.integers(0, S, len(dst))
    order = rng.permutation(len(dst))
    return dict(S=S, src=src[order], dst=dst[order], pdf=rng.integers(0, P, len(dst)), label=rng.integers(0, 5, len(dst)))


def one_key(n):
    """one state with n loops, all of one pdf and one label: every table has the one row of n arcs"""
    z = np.zeros(n, np.int64)
    return dict(S=1, src=z, dst=z, pdf=z + 3, label=z + 2)


def measure(ac, graphs):
    """per table (slots, heavy, arcs, rows) and the bound for the set's graphs, that table's rows and the set's arcs"""
    sb = np.concatenate([[0], np.cumsum([g["S"] for g in graphs])]).astype(np.int32)
    ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]).astype(np.int32)
    cat = lambda key, off=None: np.concatenate([np.asarray(g[key]) + (0 if off is None else off[i]) for i, g in enumerate(graphs)]).astype(np.int32)
    src, dst, pdf, label = cat("src", sb), cat("dst", sb), cat("pdf"), cat("label")
    lp = np.zeros(len(src), np.float32)
    ac.ac_build(len(graphs), P, p(sb), p(ab), p(src), p(dst), p(pdf), p(lp), p(label))
    out = []
    for k in range(4):
        have, bound = np.zeros(4, np.int64), np.zeros(3, np.int64)
        ac.ac_sizes(k, p(have))
        ac.ac_bound(C.c_longlong(len(graphs)), C.c_longlong(int(have[3])), C.c_longlong(int(ab[-1])), p(bound))
        out.append((have[:3].tolist(), bound.tolist()))
    return out, int(ab[-1])


def holds(ac, graphs):
    sizes, arcs = measure(ac, graphs)
    for k, (have, bound) in enumerate(sizes):
        assert all(h <= b for h, b in zip(have, bound)), (k, have, bound)
    return sizes, arcs


SETS = {
    "row-lengths": [in_degrees([0, 1, 63, 64, 65], 1)],
    "staircase": [in_degrees(list(range(64, -1, -1)), 2)],
    "many-one-state-graphs": [in_degrees([k % 4], 3 + k) for k in range(130)] + [one_key(64), one_key(65), one_key(0)],
    "a-row-of-64-beside-63-empty": [in_degrees([64] + [0] * 63, 4)],
    "a-row-of-64-alone": [one_key(64)],
    "all-of-64": [in_degrees([64] * 65, 5)],
}
for rows in (1, 63, 64, 65, 129):
    SETS["%d-rows" % rows] = [in_degrees(np.random.default_rng(rows).integers(0, 4, rows).tolist(), rows)]
    SETS["%d-rows-one-long" % rows] = [in_degrees([64] + [1] * (rows - 1), rows)]


@pytest.mark.parametrize("name", list(SETS))
def test_bounds_hold_on_the_edges(ac, name):
    holds(ac, SETS[name])


def test_bounds_hold_on_random_graphs(ac):
    rng = np.random.default_rng(7)
    for trial in range(300):
        graphs = []
        for _ in range(int(rng.integers(1, 5))):
            S = int(rng.integers(1, 140))
            top = int(rng.choice([1, 3, 64, 66, 200]))
            lengths = rng.integers(0, top + 1, S) * (rng.random(S) < rng.random())
            graphs.append(in_degrees(lengths.astype(np.int64).tolist(), 100 * trial + len(graphs)))
        holds(ac, graphs)


def test_the_arc_bound_is_attained(ac):
    assert ac.ac_pad_per_graph() == 63 * 64 == 4032
    for name in ("a-row-of-64-beside-63-empty", "a-row-of-64-alone"):
        sizes, arcs = holds(ac, SETS[name])
        assert arcs == 64
        have, bound = sizes[0]  # by destination: the row of 64 arcs leads one slice whose 63 other lanes are all padding
        assert have[2] == bound[2] == 64 + 4032
    # and per graph: two such graphs pad twice as much
    sizes, arcs = holds(ac, [one_key(64), one_key(64)])
    assert all(have[2] == bound[2] == 128 + 2 * 4032 for have, bound in sizes)
    # the slot bound too: 65 rows take two slices, 128 = 65 + 63 slots; a row of 65 arcs is one heavy row = 65 / 65
    sizes, _ = holds(ac, SETS["all-of-64"])
    assert sizes[0][0][0] == sizes[0][1][0] == 128
    sizes, _ = holds(ac, [one_key(65)])
    assert all(have[1] == bound[1] == 1 and have[0] == 0 for have, bound in sizes)
