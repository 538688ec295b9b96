"""CPU: the column lists of a tdnnf_align_graphs (tdnn-f_nas_amd/csrc/align_tables.h) -- per graph the ascending distinct pdfs of its arcs,
and in the 4th int of every by_pdf slot and heavy-row descriptor the rank of the row's pdf in that list, which addresses the compact
posteriors.  The header is built with g++ (as tests/test_align_tables_cpu.py builds it) and ALL THREE tables are compared, int for int,
with tables laid out here from the layout the header documents: rows of at most 64 arcs sorted by descending length (stable), cut into
slices of 64 lanes whose j-th arcs lie side by side, the longer rows behind them one after the other; the 4th int 0 in by_dst / by_src."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "align_tables.h"
static tdnnf::AlignHostTables T;
static const tdnnf::AlignHostTable &table(int k) { return k == 0 ? T.by_dst : k == 1 ? T.by_src : T.by_pdf; }
static const std::vector<tdnnf::AlignInt4> &array(int k, int which) { return which == 0 ? table(k).slots : which == 1 ? table(k).heavy : table(k).arcs; }
extern "C" void pc_build(int G, int P, const int *sb, const int *ab, const int *src, const int *dst, const int *pdf, const float *lp) {
  T = tdnnf::AlignHostTables();
  tdnnf::align_build_tables(G, P, sb, ab, src, dst, pdf, lp, &T, true);  // (with columns: what tdnnf_align_graphs_create uploads)
}
extern "C" int pc_size(int k, int which) { return (int)array(k, which).size(); }
extern "C" void pc_copy(int k, int which, int *out) { memcpy(out, array(k, which).data(), 16 * array(k, which).size()); }
extern "C" void pc_graphs(int *out) { memcpy(out, T.graphs.data(), sizeof(tdnnf::AlignGraphDev) * T.graphs.size()); }
extern "C" int pc_num_col_begin() { return (int)T.col_begin.size(); }
extern "C" int pc_num_col_pdfs() { return (int)T.col_pdfs.size(); }
extern "C" void pc_cols(int *begin, int *pdfs) {
  memcpy(begin, T.col_begin.data(), sizeof(int) * T.col_begin.size());
  memcpy(pdfs, T.col_pdfs.data(), sizeof(int) * T.col_pdfs.size());
}
'''


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc")
    (d / "pc.cc").write_text(SRC)
    so = str(d / "libpc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"),
                           str(d / "pc.cc"), "-o", so])
    return C.CDLL(so)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


P = 90


def graph(S, pdf, seed):
    """S states and one arc per entry of pdf, in the given (unsorted) order, between random states"""
    rng = np.random.default_rng(seed)
    pdf = np.asarray(pdf)
    pdf = pdf[rng.permutation(len(pdf))]
    return dict(S=S, src=rng.integers(0, S, size=len(pdf)), dst=rng.integers(0, S, size=len(pdf)), pdf=pdf, lp=-rng.random(len(pdf)))


def counted(counts):
    """pdf array from {pdf: number of arcs}"""
    return np.concatenate([np.full(n, q) for q, n in counts.items()])


SETS = {
    # two graphs whose pdf sets differ and overlap; pdfs 0, 1, 6 and everything above 60 are on no arc
    "two-graphs": [graph(7, counted({5: 3, 2: 1, 40: 2, 9: 4}), 1), graph(4, counted({9: 1, 60: 2, 3: 5}), 2)],
    # the light / heavy boundary: pdf 11 on 64 arcs (the longest light row), pdf 4 on 65 (heavy), beside light rows on either side of both
    "64-65-arcs": [graph(20, counted({11: 64, 4: 65, 1: 2, 7: 1, 50: 3, 89: 1}), 3)],
    # the slice boundary: 64 distinct pdfs fill one slice, 65 need a second one with 63 empty lanes
    "64-pdfs": [graph(9, np.arange(3, 67), 4)],
    "65-pdfs": [graph(9, np.concatenate([np.arange(3, 68), [10, 10, 30]]), 5)],
    # every arc on one pdf: one column, as a light row and as a heavy one
    "one-pdf": [graph(5, np.full(6, 17), 6)],
    "one-pdf-heavy": [graph(5, np.full(130, 88), 7)],
    # heavy rows whose ranks differ from their order of appearance, two graphs, a graph without arcs in between
    "all": [graph(30, counted({70: 100, 2: 70, 33: 64, 8: 1}), 8), graph(3, np.zeros(0, np.int64), 9), graph(12, np.arange(0, 90), 10),
            graph(6, counted({89: 66, 0: 65}), 11)],
}


def build(pc, graphs):
    sb = np.concatenate([[0], np.cumsum([g["S"] for g in graphs])]).astype(np.int32)
    ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]).astype(np.int32)
    cat = lambda key, off=None: np.concatenate([g[key] + (0 if off is None else off[i]) for i, g in enumerate(graphs)])
    src, dst, pdf, lp = cat("src", sb).astype(np.int32), cat("dst", sb).astype(np.int32), cat("pdf").astype(np.int32), cat("lp").astype(np.float32)
    pc.pc_build(len(graphs), P, p(sb), p(ab), p(src), p(dst), p(pdf), p(lp))
    tables = {}
    for k, name in enumerate(("by_dst", "by_src", "by_pdf")):
        arrays = []
        for which in range(3):
            a = np.zeros((pc.pc_size(k, which), 4), np.int32)
            pc.pc_copy(k, which, p(a))
            arrays.append(a)
        tables[name] = arrays
    gd = np.zeros((len(graphs), 14), np.int32)
    pc.pc_graphs(p(gd))
    begin, pdfs = np.zeros(pc.pc_num_col_begin(), np.int32), np.zeros(pc.pc_num_col_pdfs(), np.int32)
    pc.pc_cols(p(begin), p(pdfs))
    return tables, gd, begin, pdfs, (sb, ab, src, dst, pdf, lp)


def layout(stacked, G):
    """the three tables and the per-graph ranges from the documented layout: ({name: [slots, heavy, arcs]}, ranges [G, 3, 4], column lists)"""
    sb, ab, src, dst, pdf, lp = stacked
    bits = lp.view(np.int32)
    tabs = {n: [[], [], []] for n in ("by_dst", "by_src", "by_pdf")}
    ranges, cols = np.zeros((G, 3, 4), np.int64), []
    for k in range(G):
        S, arcs = int(sb[k + 1] - sb[k]), range(int(ab[k]), int(ab[k + 1]))
        cols.append(sorted(set(int(pdf[a]) for a in arcs)))
        for ti, name in enumerate(("by_dst", "by_src", "by_pdf")):
            slots, heavy, tarcs = tabs[name]
            rows = {r: [] for r in (range(S) if name != "by_pdf" else cols[k])}  # by_pdf: only the pdfs an arc names have a row
            for a in arcs:
                s, d = int(src[a] - sb[k]), int(dst[a] - sb[k])
                row, arc = {"by_dst": (d, (s, pdf[a], bits[a], a)), "by_src": (s, (d, pdf[a], bits[a], a)), "by_pdf": (int(pdf[a]), (s, d, bits[a], a))}[name]
                rows[row].append([int(v) for v in arc])
            fourth = (lambda r: cols[k].index(r)) if name == "by_pdf" else (lambda r: 0)
            slot0, heavy0 = len(slots), len(heavy)
            light = sorted((r for r in sorted(rows) if len(rows[r]) <= 64), key=lambda r: -len(rows[r]))  # (sorted() is stable)
            for first in range(0, len(light), 64):
                base, width = len(tarcs), len(rows[light[first]])
                tarcs += [[0, 0, 0, -1] for _ in range(64 * width)]
                for lane in range(64):
                    if first + lane >= len(light):
                        slots.append([-1, 0, 0, 0])
                        continue
                    r = light[first + lane]
                    slots.append([r, len(rows[r]), base + lane, fourth(r)])
                    for j, arc in enumerate(rows[r]):
                        tarcs[base + 64 * j + lane] = arc
            for r in sorted(rows):
                if len(rows[r]) > 64:
                    heavy.append([r, len(tarcs), len(tarcs) + len(rows[r]), fourth(r)])
                    tarcs += rows[r]
            ranges[k, ti] = (slot0, len(slots) - slot0, heavy0, len(heavy) - heavy0)
    return {n: [np.asarray(a, np.int32).reshape(-1, 4) for a in t] for n, t in tabs.items()}, ranges, cols


@pytest.mark.parametrize("name", list(SETS))
def test_column_lists_and_ranks(pc, name):
    graphs = SETS[name]
    tables, gd, begin, pdfs, stacked = build(pc, graphs)
    sb, ab, _, _, pdf, _ = stacked
    want, ranges, cols = layout(stacked, len(graphs))
    # the column list of every graph: sorted(set(arc_pdf))
    assert begin.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in cols])]).tolist()
    for k, g in enumerate(graphs):
        assert pdfs[begin[k]:begin[k + 1]].tolist() == cols[k] == sorted(set(g["pdf"].tolist()))
    # the graphs' ranges and all three tables, int for int
    assert np.array_equal(gd[:, 0], sb[:-1]) and np.array_equal(gd[:, 1], np.diff(sb))
    assert np.array_equal(gd[:, 2:].reshape(len(graphs), 3, 4), ranges)
    for tname in ("by_dst", "by_src", "by_pdf"):
        for which, part in enumerate(("slots", "heavy", "arcs")):
            assert np.array_equal(tables[tname][which], want[tname][which]), (tname, part)
    # said once more without the layout: a by_pdf row carries the rank of its pdf, an empty lane nothing, the other tables 0
    slots, heavy, _ = tables["by_pdf"]
    seen = 0
    for k in range(len(graphs)):
        slot0, num_slots, heavy0, num_heavy = (int(v) for v in gd[k, 10:14])
        live = [q for q in slots[slot0:slot0 + num_slots].tolist() if q[0] >= 0]
        assert all(q == [-1, 0, 0, 0] for q in slots[slot0:slot0 + num_slots].tolist() if q[0] < 0)
        rows = live + heavy[heavy0:heavy0 + num_heavy].tolist()
        assert sorted(q[3] for q in rows) == list(range(len(cols[k])))  # every column has exactly one row: one owner per (frame, column)
        assert all(cols[k][q[3]] == q[0] for q in rows)
        seen += len(rows)
    assert seen == len(pdfs)
    for tname in ("by_dst", "by_src"):
        assert (tables[tname][0][:, 3] == 0).all() and (tables[tname][1][:, 3] == 0).all()


def test_the_boundaries_are_where_they_should_be(pc):
    tables, gd, begin, pdfs, _ = build(pc, SETS["64-65-arcs"])
    slots, heavy, _ = tables["by_pdf"]
    assert heavy.tolist()[0][0] == 4 and heavy[0, 2] - heavy[0, 1] == 65 and heavy[0, 3] == 1  # pdfs 1 4 7 11 50 89: pdf 4 is column 1
    assert slots[0].tolist()[:2] == [11, 64] and slots[0, 3] == 3                               # the row of 64 arcs leads the light ones
    assert pdfs.tolist() == [1, 4, 7, 11, 50, 89]
    for name, (num_slots, empty) in {"64-pdfs": (64, 0), "65-pdfs": (128, 63)}.items():
        tables, gd, begin, pdfs, _ = build(pc, SETS[name])
        assert int(gd[0, 11]) == num_slots and int((tables["by_pdf"][0][:, 0] < 0).sum()) == empty and len(pdfs) == num_slots - empty
    tables, gd, begin, pdfs, _ = build(pc, SETS["one-pdf-heavy"])
    assert pdfs.tolist() == [88] and int(gd[0, 11]) == 0 and tables["by_pdf"][1].tolist() == [[88, 0, 130, 0]]
    tables, gd, begin, pdfs, _ = build(pc, SETS["all"])
    assert begin.tolist() == [0, 4, 4, 94, 96]  # the graph without arcs has no column
    assert tables["by_pdf"][1][:, [0, 3]].tolist() == [[2, 0], [70, 3], [0, 0], [89, 1]]
