"""CPU: the plan of the forward-backward pass's alpha checkpointing (tdnn-f_nas_amd/csrc/align_tables.h: align_checkpoint_plan and
AlignCheckpointPlan -- the interval from option align_checkpoint and the call's longest utterance, the vectors of alpha an utterance keeps,
the segments) built with g++ and set against the schedule written down here: which alphas the kernel has live, and when."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "align_tables.h"
// out: C, V(T, C), checkpoints, buffer, segments; seg: (begin, end) per segment, at most seg_cap of them.  0 and err for a refused option.
extern "C" int ck_plan(int option, int max_frames, int T, long long *out, int *seg, int seg_cap, char *err, int err_len) {
  tdnnf::AlignCheckpointPlan p;
  std::string e;
  if (!tdnnf::align_checkpoint_plan(option, max_frames, "who: ", &p, &e)) {
    snprintf(err, err_len, "%s", e.c_str());
    return 0;
  }
  out[0] = p.C; out[1] = (long long)p.vectors(T); out[2] = (long long)p.checkpoints(T); out[3] = (long long)p.buffer(T); out[4] = p.segments(T);
  for (int k = 0; k < p.segments(T) && k < seg_cap; k++) {
    seg[2 * k] = p.segment_begin(k);
    seg[2 * k + 1] = p.segment_end(T, k);
  }
  return 1;
}
'''


@pytest.fixture(scope="module")
def ck(tmp_path_factory):
    d = tmp_path_factory.mktemp("ck")
    (d / "ck.cc").write_text(SRC)
    so = str(d / "libck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"),
                           str(d / "ck.cc"), "-o", so])
    return C.CDLL(so)


def plan(ck, option, max_frames, T):
    """(C, V, checkpoints, buffer, [(begin, end)]) or the refusal's message"""
    out = (C.c_longlong * 5)()
    seg = (C.c_int * 200)()
    err = C.create_string_buffer(300)
    if not ck.ck_plan(option, max_frames, T, out, seg, 100, err, 300):
        return err.value
    return int(out[0]), int(out[1]), int(out[2]), int(out[3]), [(seg[2 * k], seg[2 * k + 1]) for k in range(min(out[4], 100))]


def schedule(T, Cint):
    """The kernel's schedule for T frames at interval Cint >= 1, written down: (the greatest number of alpha vectors that are live in
    the workspace at any moment, the segments).  The forward pass writes alpha_0 and, of alpha_1 .. alpha_T, those alpha_t with t % Cint == 0
    and t < T (the posteriors of frame t read alpha_t, so alpha_T has no reader); they stay to the end.  The backward pass takes the
    segments [k Cint, min(k Cint + Cint, T)) from the last to the first; for each it recomputes alpha_begin+1 .. alpha_end-1, which are
    live until the segment's frames have been walked."""
    kept = {0} | {t for t in range(1, T) if t % Cint == 0}
    segments = [(b, min(b + Cint, T)) for b in range(0, T, Cint)]
    most = len(kept)
    for b, e in reversed(segments):
        assert b in kept  # a segment starts at a checkpoint
        most = max(most, len(kept | set(range(b + 1, e))))
    return most, segments


def test_vectors_segments_and_interval(ck):
    for T in range(0, 41):
        for Cint in range(1, 42):
            c, V, nck, buf, segs = plan(ck, Cint, 40, T)
            assert c == min(Cint, 40)  # (an interval beyond the longest utterance is that utterance's length: the same cut of every utterance)
            live, want_segs = schedule(T, Cint)
            assert segs == want_segs == schedule(T, c)[1], (T, Cint)
            assert V == nck + buf == live, (T, Cint, V, nck, buf, live)
            assert V <= T + 1
            if T >= 1:
                assert V == -(-T // Cint) + min(Cint, T) - 1 and V <= T  # the formula of include/tdnnf_hip.h
            # the segments partition [0, T)
            assert [b for b, _ in segs] == [0] + [e for _, e in segs[:-1]] if segs else T == 0
            assert all(b < e for b, e in segs) and (not segs or segs[-1][1] == T)
        # automatic: one interval for the call from its longest utterance, T here
        c, V, _, _, segs = plan(ck, -1, T, T)
        assert c == max(1, math.isqrt(T - 1) + 1 if T > 1 else 1) == max(1, math.ceil(math.sqrt(T)))
        assert V == schedule(T, c)[0] and V <= T + 1 and segs == schedule(T, c)[1]
        # and for a shorter utterance of the same call
        for t in range(0, T + 1):
            assert plan(ck, -1, T, t)[1] == schedule(t, c)[0]


def test_automatic_interval_of_long_utterances(ck):
    for T, c in ((500, 23), (20000, 142), (10 ** 6, 1000), (10 ** 6 + 1, 1001), (2 ** 31 - 1, 46341)):
        assert plan(ck, -1, T, 0)[0] == c
        assert (c - 1) ** 2 < T <= c * c
    c, V, nck, buf, _ = plan(ck, -1, 20000, 20000)
    assert (V, nck, buf) == (282, 141, 141)
    assert plan(ck, -1, 500, 500)[1] == 44


def test_off_keeps_every_frame(ck):
    for T in range(0, 41):
        c, V, nck, buf, segs = plan(ck, 0, 40, T)
        assert (c, V, nck, buf, segs) == (0, T + 1, T + 1, 0, [])


@pytest.mark.parametrize("value", [-2, -3, -1000, -2 ** 31])
def test_refusals(ck, value):
    e = plan(ck, value, 40, 10)
    assert isinstance(e, bytes) and e.startswith(b"who: ") and b"align_checkpoint" in e and str(value).encode() in e
