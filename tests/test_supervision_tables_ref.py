"""CPU: the tables of a time-synchronous supervision as tests/supervision_tables_ref.py states them in numpy, pinned by brute force -- every
state's in-list is [a for a in arcs if dst[a] == state] in arc order, likewise its out-list, and every (sequence, frame)'s pf range is
sorted(range, key=pdf) with Python's stable sort.  And the host side of tdnnf_supervision_assign (tdnn-f_nas_amd/csrc/chain_sup_tables.h,
built with g++ as tests/test_transcript_graphs_ref.py builds its header): frame_state_begin and the widths are the statement's, its
refusals are tdnnf_supervision_create's words under the caller's name, and each capacity one short is refused by name with the excess.
The capacity excess is checked HERE, on the header: tdnnf_supervision_assign calls sup_check_capacity before it touches a device, and
tests/test_gpu_supervision_assign.py checks the entry's return value and message on a real handle as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import supervision_tables_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def minibatches(synth):
    lat = synth.make_supervision_lattice(2, 23, 40, tolerance=4, alternatives=2, seed=2)
    return {"one": synth.make_supervision(1, 1, 5, max_alt=1, seed=1),
            "narrow": synth.make_supervision(3, 7, 30, max_alt=3, seed=1),
            "lat-narrow": synth.make_supervision_lattice(2, 23, 40, tolerance=2, alternatives=1, seed=2),
            "lat-wide": lat,
            "lat-wide-permuted": ref.permuted_within_sequences(lat, seed=3),
            "P3": synth.make_supervision_lattice(2, 17, 3, tolerance=3, alternatives=2, seed=4),
            "dead": ref.dead_states()}


@pytest.fixture(scope="module")
def cases(pkg):
    return minibatches(pkg.synth)


@pytest.mark.parametrize("name", ["one", "narrow", "lat-narrow", "lat-wide", "lat-wide-permuted", "P3", "dead"])
def test_the_statement_is_the_brute_force_definition(cases, name):
    s = cases[name]
    B, T, ssb, sab, time, fin, src, dst, pdf, lp = ref.arrays(s)
    t = ref.tables(s)
    NS, NA = int(ssb[B]), int(sab[B])
    assert set(t) == set(ref.NAMES) and len(src) == NA and len(time) == NS
    arcs = list(range(NA))
    out_src = np.zeros(NA, np.int32)
    for st in range(NS):
        into = [a for a in arcs if dst[a] == st]
        i0, i1 = int(t["in_begin"][st]), int(t["in_begin"][st + 1])
        assert i1 - i0 == len(into)
        assert [(int(t["in_src"][i]), int(t["in_pdf"][i]), t["in_lp"][i].tobytes()) for i in range(i0, i1)] == \
               [(int(src[a]), int(pdf[a]), lp[a].tobytes()) for a in into], st
        outof = [a for a in arcs if src[a] == st]
        o0, o1 = int(t["out_begin"][st]), int(t["out_begin"][st + 1])
        assert o1 - o0 == len(outof)
        assert [(int(t["out_dst"][o]), int(t["out_pdf"][o]), t["out_lp"][o].tobytes()) for o in range(o0, o1)] == \
               [(int(dst[a]), int(pdf[a]), lp[a].tobytes()) for a in outof], st
        out_src[o0:o1] = st
    assert int(t["in_begin"][0]) == 0 == int(t["out_begin"][0]) and int(t["in_begin"][NS]) == NA == int(t["out_begin"][NS])
    fsb = t["frame_state_begin"].reshape(B, T + 2)
    covered = 0
    for q in range(B):
        for f in range(T + 2):
            want = [st for st in range(int(ssb[q]), int(ssb[q + 1])) if time[st] >= f]
            assert int(fsb[q, f]) == (want[0] if want else int(ssb[q + 1])), (q, f)
        for f in range(T + 1):
            o0, o1 = int(t["out_begin"][fsb[q, f]]), int(t["out_begin"][fsb[q, f + 1]])
            order = sorted(range(o0, o1), key=lambda o: int(t["out_pdf"][o]))  # (Python's sort is stable)
            have = [(int(t["pf_src"][o]), int(t["pf_dst"][o]), int(t["pf_pdf"][o]), int(t["pf_t"][o]), t["pf_lp"][o].tobytes()) for o in range(o0, o1)]
            assert have == [(int(out_src[o]), int(t["out_dst"][o]), int(t["out_pdf"][o]), f, t["out_lp"][o].tobytes()) for o in order], (q, f)
            covered += o1 - o0
            assert f < T or o1 == o0  # no arc leaves the last frame
    assert covered == NA
    if name in ("P3", "lat-wide-permuted"):  # pdf ties inside a frame, in an order the arc order does not already give
        ties = sum(int(t["pf_pdf"][o] == t["pf_pdf"][o + 1] and t["pf_t"][o] == t["pf_t"][o + 1]) for o in range(NA - 1))
        assert ties > NA // 10, ties


def test_the_set_has_the_shapes_it_is_meant_to_have(cases):
    w = {k: ref.widths(s) for k, s in cases.items()}
    assert (w["one"]["num_states"], w["one"]["num_arcs"], w["one"]["wide"]) == (2, 1, 0)
    assert (w["narrow"]["num_states"], w["narrow"]["num_arcs"], w["narrow"]["wide"], w["narrow"]["max_states_per_frame"], w["narrow"]["max_arcs_per_frame"]) == (48, 92, 0, 3, 9)
    assert (w["lat-narrow"]["num_states"], w["lat-narrow"]["num_arcs"], w["lat-narrow"]["wide"]) == (174, 277, 0)
    assert (w["lat-wide"]["num_states"], w["lat-wide"]["num_arcs"], w["lat-wide"]["wide"], w["lat-wide"]["max_states_per_frame"], w["lat-wide"]["max_arcs_per_frame"]) == (502, 855, 1, 18, 31)
    assert w["lat-wide-permuted"] == w["lat-wide"]
    # the permuted copy is the same set of arcs in another order, and its by-state lists differ from the original's somewhere
    a, b = ref.tables(cases["lat-wide"]), ref.tables(cases["lat-wide-permuted"])
    assert np.array_equal(a["in_begin"], b["in_begin"]) and np.array_equal(a["out_begin"], b["out_begin"])
    assert not np.array_equal(a["in_src"], b["in_src"]) or not np.array_equal(a["in_pdf"], b["in_pdf"])
    dead = ref.tables(cases["dead"])
    assert dead["in_begin"][2] == dead["in_begin"][3] and dead["out_begin"][3] == dead["out_begin"][4]  # no arc into state 2, none out of state 3


SRC = r'''
#include "chain_sup_tables.h"
static tdnnf::SupPlan P;
static std::string err;
extern "C" const char *sup_plan(int B, int T, const int *ssb, const int *sab, const int *time, const float *fin, const int *src, const int *dst,
                                const int *pdf, const float *lp) {
  err.clear();
  if (!tdnnf::sup_validate("who: ", true, B, T, ssb, sab, time, fin, src, dst, pdf, lp, &P, &err)) return err.c_str();
  tdnnf::sup_widths(B, T, src, &P);
  return "";
}
extern "C" const char *sup_capacity(int B, int T, int max_sequences, int max_frames, int max_states, int max_arcs) {
  err.clear();
  tdnnf::sup_check_capacity("who: ", B, T, P, max_sequences, max_frames, max_states, max_arcs, &err);
  return err.c_str();
}
extern "C" int sup_get(int *widths, int *fsb) {
  const int w[6] = {P.num_states, P.num_arcs, P.max_states_per_seq, P.max_states_per_frame, P.max_arcs_per_frame, P.wide ? 1 : 0};
  if (widths) std::copy(w, w + 6, widths);
  if (fsb) std::copy(P.frame_state_begin.begin(), P.frame_state_begin.end(), fsb);
  return (int)P.frame_state_begin.size();
}
extern "C" long long sup_stage(int a, int b, int c, int d) { return (long long)tdnnf::sup_stage_bytes(a, b, c, d); }
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("sup")
    (d / "sup.cc").write_text(SRC)
    so = str(d / "libsup.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), str(d / "sup.cc"),
                           "-o", so])
    lib = C.CDLL(so)
    lib.sup_plan.restype = lib.sup_capacity.restype = C.c_char_p
    lib.sup_stage.restype = C.c_longlong
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def plan(host, s, **changed):
    B, T, *arr = ref.arrays(dict(s, **changed))
    return host.sup_plan(B, T, *[p(a) for a in arr]).decode()


def test_the_host_side_gives_the_statements_frames_and_widths(host, cases, pkg):
    more = dict(cases, **{"lat-128": pkg.synth.make_supervision_lattice(1, 40, 200, tolerance=8, alternatives=8, seed=2),
                          "lat-430": pkg.synth.make_supervision_lattice(1, 40, 200, tolerance=10, alternatives=12, seed=2)})
    for name, s in more.items():
        assert plan(host, s) == "", name
        w = np.zeros(6, np.int32)
        fsb = np.zeros(host.sup_get(None, None), np.int32)
        host.sup_get(p(w), p(fsb))
        want = ref.widths(s)
        assert w.tolist() == [want[k] for k in ("num_states", "num_arcs", "max_states_per_seq", "max_states_per_frame", "max_arcs_per_frame", "wide")], name
        assert np.array_equal(fsb, ref.tables(s)["frame_state_begin"]), name
        B, T = int(s["B"]), int(s["T"])
        assert host.sup_stage(B, T, int(w[0]), int(w[1])) == 4 * (2 * (B + 1) + B * (T + 2) + 2 * int(w[0]) + 4 * int(w[1]))
    assert (ref.widths(more["lat-128"])["max_states_per_frame"], ref.widths(more["lat-128"])["max_arcs_per_frame"]) == (126, 241)
    assert (ref.widths(more["lat-430"])["max_states_per_frame"], ref.widths(more["lat-430"])["max_arcs_per_frame"]) == (223, 430)


def bad_inputs(s):
    """(changed arrays, the words of tdnnf_supervision_create's refusal) for every condition it checks; s: the `narrow` minibatch"""
    ssb, time, src, dst, pdf = (np.array(s[k], dtype=np.int32) for k in ("seq_state_begin", "state_time", "arc_src", "arc_dst", "arc_pdf"))
    at = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(a.dtype)
    s1 = int(ssb[1])
    return [({"B": 0}, "bad arguments"),
            ({"T": 0}, "bad arguments"),
            ({"state_time": at(time, s1, 1)}, "sequence 1 must start with its time-0 start state"),
            ({"seq_state_begin": at(ssb, 2, int(ssb[1]))}, "sequence 1 must start with its time-0 start state"),  # (no state at all)
            ({"state_time": at(time, s1 + 2, 0)}, "states must be sorted by time"),
            ({"state_time": at(time, len(time) - 1, int(s["T"]) + 1)}, "states must be sorted by time"),
            ({"state_time": at(time, 1, 0)}, "exactly one time-0 state per sequence"),
            ({"arc_src": at(src, 0, s1)}, "arc 0 must advance exactly one frame inside its sequence"),
            ({"arc_dst": at(dst, 3, -1)}, "arc 3 must advance exactly one frame inside its sequence"),
            ({"arc_pdf": at(pdf, 5, -2)}, "arc 5 must advance exactly one frame inside its sequence"),
            ({"arc_dst": at(dst, 0, int(src[0]))}, "arc 0 must advance exactly one frame inside its sequence")]


def test_refusals_are_creates_words_under_the_callers_name(host, cases):
    s = cases["narrow"]
    assert plan(host, s) == ""
    for changed, words in bad_inputs(s):
        msg = plan(host, s, **changed)
        assert msg == "who: " + words, (changed.keys(), msg)
    # on top of tdnnf_supervision_create's: arrays it would read out of bounds
    sab = np.array(s["seq_arc_begin"], dtype=np.int32)
    assert plan(host, s, seq_arc_begin=np.concatenate([[1], sab[1:]])) == "who: seq_state_begin and seq_arc_begin must start at 0"
    assert plan(host, s, seq_arc_begin=np.asarray([0, sab[2], sab[1], sab[3]])) == "who: sequence 1 has a negative arc count"


def test_each_capacity_one_short_is_refused_by_name(host, cases):
    s = cases["lat-wide"]
    assert plan(host, s) == ""
    B, T, NS, NA = int(s["B"]), int(s["T"]), 502, 855
    assert host.sup_capacity(B, T, B, T, NS, NA) == b""
    assert host.sup_capacity(B, T, B - 1, T, NS, NA) == b"who: 2 sequences exceed the capacity max_sequences = 1 by 1"
    assert host.sup_capacity(B, T, B, T - 1, NS, NA) == b"who: 23 frames exceed the capacity max_frames = 22 by 1"
    assert host.sup_capacity(B, T, B, T, NS - 1, NA) == b"who: 502 states exceed the capacity max_states = 501 by 1"
    assert host.sup_capacity(B, T, B, T, NS, NA - 3) == b"who: 855 arcs exceed the capacity max_arcs = 852 by 3"


def test_the_library_declares_and_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_supervision_reserve", "tdnnf_supervision_assign", "tdnnf_supervision_capacity", "tdnnf_supervision_dump"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    assert all(hasattr(pkg.hipabi.Supervision, n) for n in ("reserve", "assign", "capacity", "tables"))
