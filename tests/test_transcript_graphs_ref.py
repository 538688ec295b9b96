"""CPU: the definition of a transcript's graph (include/tdnnf_hip.h "transcript graphs"; tests/transcript_graphs_ref.py states it in numpy).
  - with context-independent units and entry_pdf == loop_pdf it is synth.make_alignment_graph(pdfs, optional=..., labels="unit");
  - its accepted (pdf sequence, weight) pairs are those of the model enumerated directly -- every choice of optional slots, every split of
    T frames over the taken slots, the left context the previous TAKEN slot -- in both contexts, with weights that sum exactly;
  - the host side of the compile (tdnn-f_nas_amd/csrc/align_transcripts.h, built with g++ as tests/test_align_tables_cpu.py builds its
    header: what tdnnf_transcript_graph_sizes and tdnnf_align_graphs_assign_transcripts run before anything reaches the device) gives the
    reference's sizes, in-degrees and column lists from the closed forms, and its refusals name the transcript and the slot."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import transcript_graphs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def synth(pkg):
    return pkg.synth


def test_context_independent_graph_is_make_alignment_graph(synth):
    rng = np.random.default_rng(0)
    cases = 0
    for trial in range(300):
        us = synth.make_unit_set(5, context=0, seed=trial)
        us["loop_pdf"] = us["entry_pdf"].copy()
        (units, opt), = synth.make_transcripts(1, 5, slots=(1, 8), optional_rate=float(rng.choice([0.0, 0.3, 0.6])), seed=1000 + trial)
        g = ref.transcript_graph(us, units, opt)
        want = synth.make_alignment_graph(us["entry_pdf"][units], optional=np.flatnonzero(opt).tolist(), labels="unit", num_pdfs=us["P"])
        for key in ("src", "dst", "pdf", "label", "init"):
            assert np.array_equal(g[key], want[key]), (trial, key, units, opt)
        assert g["S"] == want["S"] and g["L"] == want["L"]
        assert np.array_equal(np.isfinite(g["final"]), np.isfinite(want["final"])), (trial, units, opt)
        cases += 1
    assert cases == 300


def model_paths(us, units, opt, T):
    """The model, enumerated: sorted (pdf sequence, weight) over every set of skipped optional slots and every split of T frames over the
    taken slots, one frame each at least."""
    n, ctx = len(units), us["context"]
    pdf_of = lambda table, left, u: int(table[left + 1, u] if ctx else table[u])
    out = []
    optional = [k for k in range(n) if opt[k]]
    for r in range(len(optional) + 1):
        for skipped in itertools.combinations(optional, r):
            taken = [k for k in range(n) if k not in skipped]
            if len(taken) > T:
                continue
            for cuts in itertools.combinations(range(1, T), len(taken) - 1):
                durations = np.diff([0, *cuts, T])
                seq, w, left = [], float(len(skipped)) * us["skip_logprob"], -1
                for k, d in zip(taken, durations):
                    u = int(units[k])
                    seq += [pdf_of(us["entry_pdf"], left, u)] + [pdf_of(us["loop_pdf"], left, u)] * (int(d) - 1)
                    w += (us["take_logprob"] if opt[k] else 0.0) + (int(d) - 1) * float(us["loop_logprob"][u]) + float(us["leave_logprob"][u])
                    left = u
                out.append((tuple(seq), w))
    return sorted(out)


def graph_paths(g, T):
    """sorted (pdf sequence, weight) of every accepting path of T arcs"""
    by_src = {}
    for a in range(len(g["src"])):
        by_src.setdefault(int(g["src"][a]), []).append(a)
    out = []

    def walk(s, seq, w):
        if len(seq) == T:
            if np.isfinite(g["final"][s]):
                out.append((tuple(seq), w + float(g["final"][s])))
            return
        for a in by_src.get(s, ()):
            walk(int(g["dst"][a]), seq + [int(g["pdf"][a])], w + float(g["logprob"][a]))

    for s in np.flatnonzero(np.isfinite(g["init"])):
        walk(int(s), [], float(g["init"][s]))
    return sorted(out)


@pytest.mark.parametrize("context", [0, 1])
def test_accepted_paths_are_the_models(synth, context):
    kept = 0
    for trial in range(200):
        us = synth.make_unit_set(3, context=context, seed=trial, distinct=True)  # weights: multiples of 1/8, every sum exact
        (units, opt), = synth.make_transcripts(1, 3, slots=(1, 5), optional_rate=0.4, seed=500 + trial)
        if any(units[k] == units[k + 1] for k in range(len(units) - 1)) or any(units[k] == units[k + 2] for k in range(len(units) - 2)):
            continue  # the same unit twice within a skip's reach: two paths may share a pdf sequence
        g = ref.transcript_graph(us, units, opt)
        for T in (1, 3, 5):
            have, want = graph_paths(g, T), model_paths(us, units, opt, T)
            assert have == want, (trial, T, units, opt)
            assert len(set(p for p, _ in have)) == len(have)
        kept += 1
    assert kept >= 50, kept


SRC = r'''
#include "align_transcripts.h"
static tdnnf::TranscriptUnits U;
static tdnnf::TranscriptPlan P;
static std::string err;
extern "C" void tr_units(int units, int pdfs, int context, const int *entry, const int *loop) {
  const int n = context ? (units + 1) * units : units;
  U.U = units; U.P = pdfs; U.context = context;
  U.entry_pdf.assign(entry, entry + n);
  U.loop_pdf.assign(loop, loop + n);
}
extern "C" const char *tr_validate(int G, const int *begin, const int *unit, const int *opt) {
  err.clear();
  return tdnnf::transcripts_validate("who: ", U, G, begin, unit, opt, &err) ? "" : err.c_str();
}
extern "C" void tr_sizes(int n, const int *opt, int *out) { tdnnf::transcript_graph_size(U.context, n, opt, out, out + 1, out + 2); }
extern "C" int tr_plan(int G, const int *begin, const int *unit, const int *opt, int labelled) {
  return tdnnf::transcripts_plan("who: ", U, G, begin, unit, opt, labelled != 0, &P, &err) ? 1 : 0;
}
// which: 0 state_begin 1 arc_begin 2 num_arcs 3 max_in_degree 4 col_begin 5 col_pdfs 6 lcol_begin 7 col_labels 8 packed 9 the three maxima
extern "C" int tr_get(int which, int *out) {
  const int maxima[3] = {P.max_graph_arcs, P.max_graph_rows, P.max_slots};
  const std::vector<int> m(maxima, maxima + 3);
  const std::vector<int> *v[10] = {&P.state_begin, &P.arc_begin, &P.num_arcs, &P.max_in_degree, &P.col_begin, &P.col_pdfs, &P.lcol_begin, &P.col_labels, &P.packed, &m};
  if (out) std::copy(v[which]->begin(), v[which]->end(), out);
  return (int)v[which]->size();
}
'''


@pytest.fixture(scope="module")
def tr(tmp_path_factory):
    d = tmp_path_factory.mktemp("tr")
    (d / "tr.cc").write_text(SRC)
    so = str(d / "libtr.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), str(d / "tr.cc"),
                           "-o", so])
    lib = C.CDLL(so)
    lib.tr_validate.restype = C.c_char_p
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def stacked(transcripts):
    begin = i32(np.concatenate([[0], np.cumsum([len(u) for u, _ in transcripts])]))
    return begin, i32(np.concatenate([u for u, _ in transcripts])), i32(np.concatenate([o for _, o in transcripts]))


def get(tr, which):
    out = np.zeros(tr.tr_get(which, None), np.int32)
    tr.tr_get(which, p(out))
    return out


def set_units(tr, us):
    tr.tr_units(us["U"], us["P"], us["context"], p(i32(us["entry_pdf"]).reshape(-1)), p(i32(us["loop_pdf"]).reshape(-1)))


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("distinct", [True, False])
def test_host_plan_gives_the_references_sizes_and_lists(tr, synth, context, distinct):
    us = synth.make_unit_set(6, context=context, seed=3, distinct=distinct)
    set_units(tr, us)
    transcripts = synth.make_transcripts(60, 6, slots=(1, 12), optional_rate=0.35, seed=context)
    transcripts += [(np.asarray([2], np.int32), np.asarray([0], np.int32)), (np.asarray([1, 2], np.int32), np.asarray([1, 0], np.int32)),
                    (np.asarray([1, 2], np.int32), np.asarray([0, 1], np.int32)), (np.arange(9, dtype=np.int32) % 6, np.arange(9, dtype=np.int32) % 2),
                    (np.arange(9, dtype=np.int32) % 6, (np.arange(9, dtype=np.int32) + 1) % 2 * (np.arange(9) < 8))]
    graphs = [ref.transcript_graph(us, u, o) for u, o in transcripts]
    begin, unit, opt = stacked(transcripts)
    assert tr.tr_validate(len(transcripts), p(begin), p(unit), p(opt)) == b""
    assert tr.tr_plan(len(transcripts), p(begin), p(unit), p(opt), 1) == 1
    assert np.array_equal(get(tr, 0), np.concatenate([[0], np.cumsum([g["S"] for g in graphs])]))
    assert np.array_equal(get(tr, 1), np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])]))
    assert np.array_equal(get(tr, 2), [len(g["src"]) for g in graphs])
    in_degree = [int(np.bincount(g["dst"], minlength=g["S"]).max()) for g in graphs]
    assert np.array_equal(get(tr, 3), in_degree) and max(in_degree) == 3
    cols, lcols = [np.unique(g["pdf"]) for g in graphs], [np.unique(g["label"]) for g in graphs]
    assert np.array_equal(get(tr, 4), np.concatenate([[0], np.cumsum([len(c) for c in cols])]))
    assert np.array_equal(get(tr, 5), np.concatenate(cols))
    assert np.array_equal(get(tr, 6), np.concatenate([[0], np.cumsum([len(c) for c in lcols])]))
    assert np.array_equal(get(tr, 7), np.concatenate(lcols))
    assert np.array_equal(get(tr, 8), 2 * unit + opt)
    assert get(tr, 9).tolist() == [max(len(g["src"]) for g in graphs), max(max(g["S"], len(c), len(l)) for g, c, l in zip(graphs, cols, lcols)),
                                   max(len(u) for u, _ in transcripts)]
    for (u, o), g in zip(transcripts, graphs):
        out = np.zeros(3, np.int32)
        tr.tr_sizes(len(u), p(i32(o)), p(out))
        assert (int(out[0]), int(out[1])) == (g["S"], len(g["src"])) == ref.transcript_sizes(context, o)
        fast = ref.transcript_graph_vectorised(us, u, o)
        assert all(np.array_equal(np.asarray(fast[k]).view(np.int32) if k in ("logprob", "init", "final") else fast[k],
                                  np.asarray(g[k]).view(np.int32) if k in ("logprob", "init", "final") else g[k]) for k in g), (u, o)
    # an unlabelled plan has no label lists
    assert tr.tr_plan(len(transcripts), p(begin), p(unit), p(opt), 0) == 1
    assert get(tr, 6).tolist() == [0] and len(get(tr, 7)) == 0


def test_refusals_name_the_transcript_and_the_slot(tr, synth):
    set_units(tr, synth.make_unit_set(4, context=1, seed=0))
    ok = (np.asarray([0, 1, 2], np.int32), np.asarray([0, 1, 0], np.int32))

    def refusal(bad):
        begin, unit, opt = stacked([ok, bad, ok])
        return tr.tr_validate(3, p(begin), p(unit), p(opt)).decode()

    assert refusal(ok) == ""
    msg = refusal((np.asarray([0, 1, 4], np.int32), np.asarray([0, 0, 0], np.int32)))
    assert msg.startswith("who: transcript 1 slot 2: unit 4 outside [0, 4)"), msg
    msg = refusal((np.asarray([0, -1], np.int32), np.asarray([0, 0], np.int32)))
    assert msg.startswith("who: transcript 1 slot 1: unit -1 outside"), msg
    msg = refusal((np.asarray([0, 1, 2, 3], np.int32), np.asarray([0, 1, 1, 0], np.int32)))
    assert msg.startswith("who: transcript 1 slot 2: optional, as is slot 1 before it"), msg
    msg = refusal((np.asarray([3], np.int32), np.asarray([1], np.int32)))
    assert msg.startswith("who: transcript 1 slot 0: optional, and the transcript has no mandatory slot"), msg
    # a transcript without slots, and a batch without transcripts
    begin = i32([0, 3, 3])
    msg = tr.tr_validate(2, p(begin), p(i32([0, 1, 2])), p(i32([0, 0, 0]))).decode()
    assert msg.startswith("who: transcript 1 has 0 slots"), msg
    assert tr.tr_validate(0, p(begin), p(begin), p(begin)).decode().startswith("who: bad arguments")


def test_the_library_declares_and_exports_the_transcript_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_unit_set_create", "tdnnf_unit_set_destroy", "tdnnf_transcript_graph_sizes", "tdnnf_align_graphs_assign_transcripts",
                 "tdnnf_supervision_assign_e2e_transcripts"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    assert all(hasattr(pkg.hipabi, n) for n in ("UnitSet",)) and hasattr(pkg.hipabi.AlignGraphs, "assign_transcripts")
    assert hasattr(pkg.hipabi.Supervision, "assign_transcripts")
