"""CPU: the fourth arc table of a labelled tdnnf_align_graphs (tdnn-f_nas_amd/csrc/align_tables.h, by_label) built with g++ as
tests/test_align_tables_cpu.py builds the other three, and decoded back: one row per distinct label of a graph, the row's arcs in the
caller's order with the arc's pdf in the 4th int, its column -- the label's rank in the graph's ascending label list -- in the 4th int of
its slot or heavy-row descriptor; a label on 65 arcs is a heavy row and one on 64 the longest light one; and the three old tables are byte
for byte what they are without labels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "align_tables.h"
static tdnnf::AlignHostTables T;
static const tdnnf::AlignHostTable &table(int k) { return k == 0 ? T.by_dst : k == 1 ? T.by_src : k == 2 ? T.by_pdf : T.by_label; }
static const std::vector<tdnnf::AlignInt4> &array(int k, int which) { return which == 0 ? table(k).slots : which == 1 ? table(k).heavy : table(k).arcs; }
extern "C" void lt_build(int G, int P, const int *sb, const int *ab, const int *src, const int *dst, const int *pdf, const float *lp, int columns,
                         const int *label) {
  T = tdnnf::AlignHostTables();
  tdnnf::align_build_tables(G, P, sb, ab, src, dst, pdf, lp, &T, columns != 0, label);
}
extern "C" int lt_size(int k, int which) { return (int)array(k, which).size(); }
extern "C" void lt_copy(int k, int which, int *out) { memcpy(out, array(k, which).data(), 16 * array(k, which).size()); }
extern "C" void lt_graphs(int *out) { memcpy(out, T.graphs.data(), sizeof(tdnnf::AlignGraphDev) * T.graphs.size()); }
extern "C" int lt_num_ranges() { return (int)T.label_range.size(); }
extern "C" void lt_ranges(int *out) {
  static_assert(sizeof(tdnnf::AlignRange) == 4 * sizeof(int), "four ints");
  memcpy(out, T.label_range.data(), sizeof(tdnnf::AlignRange) * T.label_range.size());
}
extern "C" int lt_list_size(int which) { return (int)(which == 0 ? T.lcol_begin : which == 1 ? T.col_labels : which == 2 ? T.col_begin : T.col_pdfs).size(); }
extern "C" void lt_list(int which, int *out) {
  const std::vector<int> &v = which == 0 ? T.lcol_begin : which == 1 ? T.col_labels : which == 2 ? T.col_begin : T.col_pdfs;
  memcpy(out, v.data(), sizeof(int) * v.size());
}
'''
P = 9


@pytest.fixture(scope="module")
def lt(tmp_path_factory):
    d = tmp_path_factory.mktemp("lt")
    (d / "lt.cc").write_text(SRC)
    so = str(d / "liblt.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"),
                           str(d / "lt.cc"), "-o", so])
    return C.CDLL(so)


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def random_graph(S, A, labels, seed):
    rng = np.random.default_rng(seed)
    return dict(S=S, src=rng.integers(0, S, size=A), dst=rng.integers(0, S, size=A), pdf=rng.integers(0, P - 1, size=A), lp=-rng.random(A),
                label=rng.permutation(np.asarray(labels)))


def edges():
    """label 40 on 64 arcs (the longest light row), label 7 on 65 (heavy), label 1000 on 300 (heavy, the greatest label), and 70 labels on
    one or two arcs each between them, so the light rows fill a slice and start a second; labels 0 .. 6 are on no arc"""
    small = np.concatenate([100 + 3 * np.arange(70), 100 + 3 * np.arange(25)])
    return random_graph(50, 64 + 65 + 300 + len(small), np.concatenate([np.full(64, 40), np.full(65, 7), np.full(300, 1000), small]), 5)


SETS = {"one-label": [random_graph(3, 10, np.zeros(10, np.int64), 1)], "arc-labels": [random_graph(20, 130, np.arange(130), 2)],
        "edges": [edges()], "three-graphs": [random_graph(20, 130, 500 - np.arange(130), 2), edges(), random_graph(7, 40, np.arange(40) % 5, 3)]}


def build(lt, graphs, labels=True, columns=True):
    sb = np.concatenate([[0], np.cumsum([g["S"] for g in graphs])]).astype(np.int32)
    ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]).astype(np.int32)
    src = np.concatenate([g["src"] + sb[i] for i, g in enumerate(graphs)]).astype(np.int32)
    dst = np.concatenate([g["dst"] + sb[i] for i, g in enumerate(graphs)]).astype(np.int32)
    pdf = np.concatenate([g["pdf"] for g in graphs]).astype(np.int32)
    lp = np.concatenate([g["lp"] for g in graphs]).astype(np.float32)
    label = np.concatenate([g["label"] for g in graphs]).astype(np.int32)
    lt.lt_build(len(graphs), P, p(sb), p(ab), p(src), p(dst), p(pdf), p(lp), int(columns), p(label) if labels else None)
    tables = []
    for k in range(4):
        arrays = []
        for which in range(3):
            a = np.zeros((lt.lt_size(k, which), 4), np.int32)
            lt.lt_copy(k, which, p(a))
            arrays.append(a)
        tables.append(arrays)
    gd = np.zeros((len(graphs), 14), np.int32)
    lt.lt_graphs(p(gd))
    ranges = np.zeros((lt.lt_num_ranges(), 4), np.int32)
    lt.lt_ranges(p(ranges))
    lists = []
    for which in range(4):
        v = np.zeros(lt.lt_list_size(which), np.int32)
        lt.lt_list(which, p(v))
        lists.append(v)
    return tables, gd, ranges, lists, (sb, ab, src, dst, pdf, lp, label)


@pytest.mark.parametrize("name", list(SETS))
def test_by_label_decodes_back_into_the_graphs(lt, name):
    graphs = SETS[name]
    tables, gd, ranges, (lcol_begin, col_labels, _, _), (sb, ab, src, dst, pdf, lp, label) = build(lt, graphs)
    slots, heavy, arcs = tables[3]
    bits = lp.view(np.int32)
    assert len(ranges) == len(graphs) and lcol_begin.tolist()[0] == 0 and len(lcol_begin) == len(graphs) + 1
    used = np.zeros(len(arcs), bool)
    next_slot = next_heavy = 0
    for k, g in enumerate(graphs):
        want_list = sorted(set(int(v) for v in g["label"]))
        assert col_labels[lcol_begin[k]:lcol_begin[k + 1]].tolist() == want_list  # the ascending label column list
        slot0, num_slots, heavy0, num_heavy = (int(v) for v in ranges[k])
        assert slot0 == next_slot and heavy0 == next_heavy and num_slots % 64 == 0
        next_slot, next_heavy = slot0 + num_slots, heavy0 + num_heavy
        rows, lengths = {}, []
        for row, length, pos, column in slots[slot0:slot0 + num_slots].tolist():
            if row < 0:
                assert (row, length, pos, column) == (-1, 0, 0, 0)
                lengths.append(-1)
                continue
            assert 1 <= length <= 64 and column == row and column not in rows  # skip_empty: no empty row; the row is the label's rank
            at_ = pos + 64 * np.arange(length)
            assert not used[at_].any()
            used[at_] = True
            rows[column] = [tuple(a) for a in arcs[at_].tolist()]
            lengths.append(length)
        assert all(a >= b for a, b in zip(lengths, lengths[1:]))  # slices in non-increasing length, the empty lanes last
        for row, first, last, column in heavy[heavy0:heavy0 + num_heavy].tolist():
            assert last - first > 64 and column == row and column not in rows and not used[first:last].any()
            used[first:last] = True
            rows[column] = [tuple(a) for a in arcs[first:last].tolist()]
        # one row per distinct label, at the label's rank; its arcs in the caller's order: (source, destination, log-prob bits, PDF)
        assert sorted(rows) == list(range(len(want_list)))
        want = {}
        for a in range(ab[k], ab[k + 1]):
            want.setdefault(want_list.index(int(label[a])), []).append((int(src[a] - sb[k]), int(dst[a] - sb[k]), int(bits[a]), int(pdf[a])))
        assert rows == want
    assert next_slot == len(slots) and next_heavy == len(heavy)
    assert used.sum() == ab[-1]  # every arc exactly once
    assert (arcs[~used] == np.array([0, 0, 0, -1])).all()  # a slice's padding


def test_heavy_above_64_arcs(lt):
    tables, _, ranges, (_, col_labels, _, _), _ = build(lt, SETS["edges"])
    slots, heavy, _ = tables[3]
    assert col_labels.tolist()[:3] == [7, 40, 100] and col_labels[-1] == 1000 and len(col_labels) == 73
    assert ranges.tolist() == [[0, 128, 0, 2]]  # 71 light rows in two slices, two heavy rows
    assert [(h[3], h[2] - h[1]) for h in heavy.tolist()] == [(0, 65), (72, 300)]  # label 7 at column 0, label 1000 at the last
    assert slots[0].tolist()[:2] == [1, 64] and slots[0, 3] == 1  # label 40, on 64 arcs, leads the light rows
    assert (slots[71:, 0] == -1).all() and (slots[:71, 0] >= 0).all()


@pytest.mark.parametrize("columns", [False, True])
def test_old_tables_are_byte_equal_without_labels(lt, columns):
    graphs = SETS["three-graphs"]
    with_l = build(lt, graphs, True, columns)
    without = build(lt, graphs, False, columns)
    for k in range(3):
        for which in range(3):
            assert with_l[0][k][which].tobytes() == without[0][k][which].tobytes() and len(with_l[0][k][2]) > 0
    assert with_l[1].tobytes() == without[1].tobytes()  # AlignGraphDev: the same 14 ints a graph
    assert with_l[3][2].tolist() == without[3][2].tolist() and with_l[3][3].tolist() == without[3][3].tolist()  # col_begin, col_pdfs
    # no labels: no fourth table, no ranges, no list
    assert all(len(a) == 0 for a in without[0][3]) and len(without[2]) == 0 and without[3][0].tolist() == [0] and len(without[3][1]) == 0
