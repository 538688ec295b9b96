"""CPU: the host side of a tdnnf_align_graphs (tdnn-f_nas_amd/csrc/align_tables.h: the three sliced arc tables and the launch-form plan
of the recursions that walk them) built with g++ and checked from Python: the tables are decoded back into the graphs' arcs, the plan is
compared with values written out by hand from the constants at every threshold."""
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
extern "C" void at_build(int G, int P, const int *sb, const int *ab, const int *src, const int *dst, const int *pdf, const float *lp) {
  T = tdnnf::AlignHostTables();
  tdnnf::align_build_tables(G, P, sb, ab, src, dst, pdf, lp, &T);
}
extern "C" int at_size(int k, int which) { return (int)array(k, which).size(); }
extern "C" void at_copy(int k, int which, int *out) { memcpy(out, array(k, which).data(), 16 * array(k, which).size()); }
extern "C" void at_graphs(int *out) {
  static_assert(sizeof(tdnnf::AlignGraphDev) == 14 * sizeof(int), "two ints and three ranges of four");
  memcpy(out, T.graphs.data(), sizeof(tdnnf::AlignGraphDev) * T.graphs.size());
}
extern "C" int at_max_in_degree(int g) { return T.max_in_degree[g]; }
extern "C" int at_plan(int S, int P, int form, int want_alpha, long long budget, long long *out, char *err, int err_len) {
  tdnnf::AlignFormPlan p;
  std::string e;
  if (!tdnnf::align_form_plan(S, P, form, want_alpha != 0, (size_t)budget, "who: ", &p, &e)) {
    snprintf(err, err_len, "%s", e.c_str());
    return 0;
  }
  out[0] = p.threads; out[1] = p.lds; out[2] = p.alpha_in_lds; out[3] = p.row_in_lds; out[4] = (long long)p.lds_bytes;
  return 1;
}
'''


@pytest.fixture(scope="module")
def at(tmp_path_factory):
    d = tmp_path_factory.mktemp("at")
    (d / "at.cc").write_text(SRC)
    so = str(d / "libat.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"),
                           str(d / "at.cc"), "-o", so])
    return C.CDLL(so)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ tables
P = 9


def chain(S, seed):
    """S states, each with its loop and an arc to the next: S light rows by destination and by source"""
    rng = np.random.default_rng(seed)
    st = np.arange(S)
    src, dst = np.concatenate([st, st[:-1]]), np.concatenate([st, st[1:]])
    order = rng.permutation(len(src))  # the caller's order is no sorted order
    return dict(S=S, src=src[order], dst=dst[order], pdf=rng.integers(0, P - 1, size=len(src)), lp=-rng.random(len(src)))


def edges():
    """70 states: 64 arcs enter state 0 (the longest light row) and 65 state 1 (heavy); 64 leave state 2 and 65 state 3; pdf 0 is on 64
    arcs and pdf 1 on 65; nothing enters state 4, nothing leaves state 5; no arc names pdf P - 1"""
    S = 70
    src = np.concatenate([np.arange(6, 70), np.arange(5, 70), np.full(64, 2), np.full(65, 3)])
    dst = np.concatenate([np.full(64, 0), np.full(65, 1), np.arange(6, 70), np.arange(5, 70)])
    src[src == 5] = 6
    dst[dst == 4] = 6
    pdf = np.concatenate([np.full(64, 0), np.full(65, 1), 2 + np.arange(129) % (P - 3)])
    order = np.random.default_rng(5).permutation(len(src))
    g = dict(S=S, src=src[order], dst=dst[order], pdf=pdf[order], lp=-np.random.default_rng(6).random(len(src)))
    deg = lambda a: np.bincount(a, minlength=S)
    assert deg(g["dst"])[0] == 64 and deg(g["dst"])[1] == 65 and deg(g["src"])[2] == 64 and deg(g["src"])[3] == 65
    assert deg(g["dst"])[4] == 0 and deg(g["src"])[5] == 0
    assert np.bincount(g["pdf"], minlength=P)[[0, 1, P - 1]].tolist() == [64, 65, 0]
    return g


SETS = {"1-row": [chain(1, 1)], "63-rows": [chain(63, 2)], "64-rows": [chain(64, 3)], "65-rows": [chain(65, 4)], "edges": [edges()],
        "two-graphs": [chain(65, 7), edges()], "all": [chain(1, 1), edges(), chain(64, 3), chain(63, 2), chain(65, 4)]}


def build(at, graphs):
    """the tables of the set: ({"by_dst": (slots, heavy, arcs) ...} as [n, 4] int32, graphs [G, 14] int32, max_in_degree) and the stacked arrays"""
    sb = np.concatenate([[0], np.cumsum([g["S"] for g in graphs])]).astype(np.int32)
    ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]).astype(np.int32)
    src = np.concatenate([g["src"] + sb[i] for i, g in enumerate(graphs)]).astype(np.int32)
    dst = np.concatenate([g["dst"] + sb[i] for i, g in enumerate(graphs)]).astype(np.int32)
    pdf = np.concatenate([g["pdf"] for g in graphs]).astype(np.int32)
    lp = np.concatenate([g["lp"] for g in graphs]).astype(np.float32)
    at.at_build(len(graphs), P, p(sb), p(ab), p(src), p(dst), p(pdf), p(lp))
    tables = {}
    for k, name in enumerate(("by_dst", "by_src", "by_pdf")):
        arrays = []
        for which in range(3):
            a = np.zeros((at.at_size(k, which), 4), np.int32)
            at.at_copy(k, which, p(a))
            arrays.append(a)
        tables[name] = arrays
    gd = np.zeros((len(graphs), 14), np.int32)
    at.at_graphs(p(gd))
    return tables, gd, [at.at_max_in_degree(g) for g in range(len(graphs))], (sb, ab, src, dst, pdf, lp)


def expected_rows(name, k, stacked):
    """{row: [arc int4 ...]} of graph k in the caller's order"""
    sb, ab, src, dst, pdf, lp = stacked
    bits = lp.view(np.int32)
    rows = {}
    for a in range(ab[k], ab[k + 1]):
        s, d = int(src[a] - sb[k]), int(dst[a] - sb[k])
        row, arc = {"by_dst": (d, (s, pdf[a], bits[a], a)), "by_src": (s, (d, pdf[a], bits[a], a)), "by_pdf": (int(pdf[a]), (s, d, bits[a], a))}[name]
        rows.setdefault(row, []).append(tuple(int(v) for v in arc))
    return rows


@pytest.mark.parametrize("name", list(SETS))
def test_tables_decode_back_into_the_graphs(at, name):
    graphs = SETS[name]
    tables, gd, max_in, stacked = build(at, graphs)
    sb, ab = stacked[:2]
    for ti, tname in enumerate(("by_dst", "by_src", "by_pdf")):
        slots, heavy, arcs = tables[tname]
        used = np.zeros(len(arcs), bool)  # arc-table positions that belong to a row
        next_slot = next_heavy = 0
        seen = []
        for k, g in enumerate(graphs):
            assert gd[k, 0] == sb[k] and gd[k, 1] == g["S"]
            slot0, num_slots, heavy0, num_heavy = (int(v) for v in gd[k, 2 + 4 * ti:6 + 4 * ti])
            # each graph's ranges: a multiple of 64 slots, one behind the other without overlap
            assert slot0 == next_slot and heavy0 == next_heavy and num_slots % 64 == 0 and num_slots >= 0 and num_heavy >= 0
            next_slot, next_heavy = slot0 + num_slots, heavy0 + num_heavy
            rows, lengths = {}, []
            for row, length, pos, zero in slots[slot0:slot0 + num_slots].tolist():
                if row < 0:
                    assert (row, length, pos, zero) == (-1, 0, 0, 0)  # an empty lane
                    lengths.append(-1)
                    continue
                assert 0 <= length <= 64 and zero == 0 and row not in rows
                at_ = pos + 64 * np.arange(length)
                assert not used[at_].any()
                used[at_] = True
                rows[row] = [tuple(a) for a in arcs[at_].tolist()]
                lengths.append(length)
            # slices in non-increasing length, the empty lanes behind the last row only
            assert all(a >= b for a, b in zip(lengths, lengths[1:]))
            assert lengths.count(-1) < 64 or not lengths
            for s in range(0, num_slots, 64):  # the 64 rows of a slice start side by side
                live = [q for q in slots[slot0 + s:slot0 + s + 64].tolist() if q[0] >= 0]
                assert [q[2] for q in live] == list(range(live[0][2], live[0][2] + len(live)))
            for row, first, last, zero in heavy[heavy0:heavy0 + num_heavy].tolist():
                assert last - first > 64 and zero == 0 and row not in rows and not used[first:last].any()
                used[first:last] = True
                rows[row] = [tuple(a) for a in arcs[first:last].tolist()]
            want = expected_rows(tname, k, stacked)
            if tname == "by_pdf":  # no empty row: the pdfs that an arc names
                assert all(len(r) > 0 for r in rows.values())
            else:  # one row per state, empty or not
                assert sorted(rows) == list(range(g["S"]))
                want = {s: want.get(s, []) for s in range(g["S"])}
            assert rows == want  # every row's arcs, in the caller's order
            seen += [a[3] for r in rows.values() for a in r]
            if tname == "by_dst":
                assert max_in[k] == max(len(r) for r in rows.values())
        assert next_slot == len(slots) and next_heavy == len(heavy)
        assert sorted(seen) == list(range(ab[-1]))  # every arc exactly once
        assert (arcs[~used] == np.array([0, 0, 0, -1])).all()  # a slice's padding


def test_the_edges_are_where_they_should_be(at):
    tables, gd, max_in, _ = build(at, SETS["edges"])
    assert max_in == [65]
    for ti, tname in enumerate(("by_dst", "by_src", "by_pdf")):
        slots, heavy, _ = tables[tname]
        assert gd[0, 5 + 4 * ti] == 1 and heavy[0, 0] == {"by_dst": 1, "by_src": 3, "by_pdf": 1}[tname]  # the row of 65 arcs is heavy
        assert slots[0].tolist()[:2] == [{"by_dst": 0, "by_src": 2, "by_pdf": 0}[tname], 64]               # the row of 64 leads the light ones
    assert [int(gd[0, 3 + 4 * ti]) for ti in range(3)] == [128, 128, 64]  # 69 light states; P - 2 = 7 light pdfs
    counts = {n: [(len(g_[0]), int((g_[0][:, 0] < 0).sum())) for g_ in [build(at, SETS[n])[0]["by_dst"]]][0] for n in ("1-row", "63-rows", "64-rows", "65-rows")}
    assert counts == {"1-row": (64, 63), "63-rows": (64, 1), "64-rows": (64, 0), "65-rows": (128, 63)}


# ------------------------------------------------------------------------------------------------ plan
BUDGET = 150 * 1024  # kLdsBudget (chain_plan.h); below: 64 / 1024 states, kAlignRowRegs = 8 floats and kAlignFbAlphaRegs = 7 doubles a thread


def plan(at, S, pdfs, form, want_alpha):
    out = np.zeros(5, np.int64)
    err = C.create_string_buffer(256)
    if not at.at_plan(S, pdfs, form, int(want_alpha), C.c_longlong(BUDGET), p(out), err, 256):
        return err.value
    return tuple(int(v) for v in out)


# (states, pdfs, align_form, a third vector wanted): (threads, lds, alpha_in_lds, row_in_lds, lds_bytes)
PLANS = {
    # thread counts: 64 / 65 and 1024 / 1025 states
    (64, 40, 0, False): (64, 1, 0, 1, 2 * 8 * 64 + 2 * 4 * 40),
    (65, 40, 0, False): (256, 1, 0, 1, 2 * 8 * 65 + 2 * 4 * 40),
    (1024, 40, 0, False): (256, 1, 0, 1, 2 * 8 * 1024 + 2 * 4 * 40),
    (1025, 40, 0, False): (1024, 1, 0, 1, 2 * 8 * 1025 + 2 * 4 * 40),
    (64, 40, 1, False): (64, 1, 0, 1, 1344),
    (64, 40, 2, False): (64, 0, 0, 0, 0),
    (65, 40, 2, False): (256, 0, 0, 0, 0),
    (1025, 40, 2, True): (1024, 0, 0, 0, 0),
    (64, 40, 0, True): (64, 1, 1, 1, 3 * 8 * 64 + 2 * 4 * 40),
    (1025, 40, 1, True): (1024, 1, 1, 1, 3 * 8 * 1025 + 2 * 4 * 40),
    # three vectors: 3 * 8 * 6400 = 153 600 bytes is the budget, and no room is left for the rows
    (6400, 40, 0, True): (1024, 1, 1, 0, 153600),
    (6400, 40, 1, True): (1024, 1, 1, 0, 153600),
    (6401, 40, 0, True): (1024, 1, 0, 0, 2 * 8 * 6401),  # no staged alpha_t: with posteriors no staged rows either
    (6401, 40, 1, True): (1024, 1, 0, 0, 2 * 8 * 6401),
    (6401, 40, 0, False): (1024, 1, 0, 1, 2 * 8 * 6401 + 2 * 4 * 40),
    (6400, 40, 2, True): (1024, 0, 0, 0, 0),
    # two vectors: 2 * 8 * 9600 = 153 600
    (9600, 40, 0, False): (1024, 1, 0, 0, 153600),
    (9600, 40, 1, False): (1024, 1, 0, 0, 153600),
    (9600, 40, 0, True): (1024, 1, 0, 0, 153600),
    (9600, 40, 2, False): (1024, 0, 0, 0, 0),
    (9601, 40, 0, False): (1024, 0, 0, 0, 0),
    (9601, 40, 0, True): (1024, 0, 0, 0, 0),
    (9601, 40, 2, False): (1024, 0, 0, 0, 0),
    # rows: 8 floats a thread -- 512 pdfs at 64 threads, 2048 at 256
    (64, 512, 0, False): (64, 1, 0, 1, 2 * 8 * 64 + 2 * 4 * 512),
    (64, 513, 0, False): (64, 1, 0, 0, 2 * 8 * 64),
    (64, 512, 1, True): (64, 1, 1, 1, 3 * 8 * 64 + 2 * 4 * 512),
    (64, 513, 1, True): (64, 1, 1, 0, 3 * 8 * 64),
    (64, 512, 2, False): (64, 0, 0, 0, 0),
    (65, 2048, 0, False): (256, 1, 0, 1, 2 * 8 * 65 + 2 * 4 * 2048),
    (65, 2049, 0, False): (256, 1, 0, 0, 2 * 8 * 65),
    (65, 2048, 0, True): (256, 1, 1, 1, 3 * 8 * 65 + 2 * 4 * 2048),
    (65, 2049, 0, True): (256, 1, 1, 0, 3 * 8 * 65),
    (65, 2049, 2, True): (256, 0, 0, 0, 0),
}


@pytest.mark.parametrize("case", list(PLANS), ids=["S%d-P%d-form%d-%s" % (c[0], c[1], c[2], "alpha" if c[3] else "plain") for c in PLANS])
def test_form_plan_at_the_thresholds(at, case):
    assert plan(at, *case) == PLANS[case]


def test_form_plan_refusals(at):
    for want_alpha in (False, True):
        e = plan(at, 9601, 40, 1, want_alpha)  # forced into an LDS that two vectors do not fit
        assert isinstance(e, bytes) and e.startswith(b"who: ") and b"align_form = 1" in e and b"9601" in e
        assert isinstance(plan(at, 9600, 40, 1, want_alpha), tuple)
        for form in (-1, 3):
            e = plan(at, 64, 40, form, want_alpha)
            assert isinstance(e, bytes) and e.startswith(b"who: ") and b"align_form must be 0, 1 or 2" in e
