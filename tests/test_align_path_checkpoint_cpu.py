"""CPU: the plan of the best path's back-pointer checkpointing (tdnn-f_nas_amd/csrc/align_tables.h: align_path_checkpoint_plan and
AlignPathCheckpointPlan -- the interval from option align_path_checkpoint and the call's longest utterance, the checkpoints and the frames
of back-pointers an utterance keeps, the segments, the ints of its region) built with g++ and set against the schedule written down here:
which alpha_kC the kernel stores, and how many frames of back-pointers are live at once."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "align_tables.h"
// out: C, checkpoints, buffer frames, segments, ints of the region at S states; seg: (begin, end) per segment, at most seg_cap of them.
// 0 and err for a refused option.
extern "C" int pk_plan(int option, int max_frames, int T, int S, long long *out, int *seg, int seg_cap, char *err, int err_len) {
  tdnnf::AlignPathCheckpointPlan p;
  std::string e;
  if (!tdnnf::align_path_checkpoint_plan(option, max_frames, "who: ", &p, &e)) {
    snprintf(err, err_len, "%s", e.c_str());
    return 0;
  }
  out[0] = p.C; out[1] = (long long)p.checkpoints(T); out[2] = (long long)p.buffer_frames(T); out[3] = p.segments(T); out[4] = (long long)p.ints(T, S);
  for (int k = 0; k < p.segments(T) && k < seg_cap; k++) {
    seg[2 * k] = p.segment_begin(k);
    seg[2 * k + 1] = p.segment_end(T, k);
  }
  return 1;
}
// the message of the forward-backward pass's option, which shares the interval's rules, is what it was
extern "C" int fb_refusal(int option, char *err, int err_len) {
  tdnnf::AlignCheckpointPlan p;
  std::string e;
  if (tdnnf::align_checkpoint_plan(option, 40, "who: ", &p, &e)) return 0;
  snprintf(err, err_len, "%s", e.c_str());
  return 1;
}
'''


@pytest.fixture(scope="module")
def pk(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk")
    (d / "pk.cc").write_text(SRC)
    so = str(d / "libpk.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"),
                           str(d / "pk.cc"), "-o", so])
    return C.CDLL(so)


def plan(pk, option, max_frames, T, S=7):
    """(C, checkpoints, buffer frames, [(begin, end)], ints) or the refusal's message"""
    out = (C.c_longlong * 5)()
    seg = (C.c_int * 200)()
    err = C.create_string_buffer(300)
    if not pk.pk_plan(option, max_frames, T, S, out, seg, 100, err, 300):
        return err.value
    return int(out[0]), int(out[1]), int(out[2]), [(seg[2 * k], seg[2 * k + 1]) for k in range(min(out[3], 100))], int(out[4])


def schedule(T, Cint):
    """The kernel's schedule for T frames at interval Cint >= 1, written down: (the alpha_t it stores, the greatest number of frames whose
    back-pointers are live at once, the segments).  The forward pass stores alpha_t at every segment start t = k Cint < T and keeps the
    back-pointers of the frames of the segment it is in -- a new segment starts over the one before.  The trace-back walks the last
    segment as the forward pass left it, then takes the segments before it from the last to the first: it reloads alpha_begin (which
    must have been stored), reruns the frames [begin, end) -- their back-pointers are live until the segment has been walked."""
    segments = [(b, min(b + Cint, T)) for b in range(0, T, Cint)]
    kept = {b for b, _ in segments}
    live = 0
    for t in range(T):  # forward: frame t's back-pointers join those of its segment's earlier frames
        live = max(live, t % Cint + 1)
    for b, e in reversed(segments[:-1]):
        assert b in kept
        live = max(live, e - b)
    return kept, live, segments


def test_segments_counts_and_interval(pk):
    for T in range(0, 41):
        for Cint in range(1, 42):
            c, nck, buf, segs, ints = plan(pk, Cint, 40, T)
            assert c == min(Cint, 40)  # (an interval beyond the longest utterance is that utterance's length: the same cut of every utterance)
            kept, live, want_segs = schedule(T, Cint)
            assert segs == want_segs == schedule(T, c)[2] == [(b, min(b + Cint, T)) for b in range(0, T, Cint)], (T, Cint)
            assert nck == len(kept) == -(-T // Cint) and buf == live == min(Cint, T), (T, Cint, nck, buf)
            # the region of include/tdnnf_hip.h, in ints: 8 K S + 4 roundup(B S, 2) + 4 roundup(T, 2) bytes
            for S in (1, 7, 10):
                assert plan(pk, Cint, 40, T, S)[4] == 2 * nck * S + -(-buf * S // 2) * 2 + -(-T // 2) * 2
            assert ints % 2 == 0
            assert all(b < e for b, e in segs) and (not segs or (segs[0][0] == 0 and segs[-1][1] == T))
            assert [b for b, _ in segs[1:]] == [e for _, e in segs[:-1]]
        # automatic: one interval for the call from its longest utterance, T here
        c, nck, buf, segs, _ = plan(pk, -1, T, T)
        assert c == max(1, math.isqrt(T - 1) + 1 if T > 1 else 1) == max(1, math.ceil(math.sqrt(T)))
        assert (nck, buf, segs) == (len(schedule(T, c)[0]), schedule(T, c)[1], schedule(T, c)[2])
        # and for a shorter utterance of the same call
        for t in range(0, T + 1):
            got = plan(pk, -1, T, t)
            assert got[0] == c and (got[1], got[2]) == (len(schedule(t, c)[0]), schedule(t, c)[1])


def test_automatic_interval_of_long_utterances(pk):
    for T, c in ((500, 23), (4000, 64), (20000, 142), (10 ** 6, 1000), (10 ** 6 + 1, 1001), (2 ** 31 - 1, 46341)):
        assert plan(pk, -1, T, 0)[0] == c
        assert (c - 1) ** 2 < T <= c * c
    c, nck, buf, _, ints = plan(pk, -1, 20000, 20000, 3001)
    assert (c, nck, buf) == (142, 141, 142)
    assert 4 * ints == 8 * 141 * 3001 + 4 * 142 * 3001 + 4 * 20000 and 4 * ints < 5.2e6  # against 4 * 20 000 * 3 001 = 240 MB


def test_off_keeps_every_frame(pk):
    for T in range(0, 41):
        c, nck, buf, segs, ints = plan(pk, 0, 40, T)
        assert (c, nck, buf, segs, ints) == (0, 0, T, [], -(-T * 7 // 2) * 2)


@pytest.mark.parametrize("value", [-2, -3, -1000, -2 ** 31])
def test_refusals(pk, value):
    e = plan(pk, value, 40, 10)
    assert isinstance(e, bytes) and e.startswith(b"who: ") and b"align_path_checkpoint" in e and str(value).encode() in e
    err = C.create_string_buffer(300)
    assert pk.fb_refusal(value, err, 300) == 1
    assert err.value == b"who: option align_checkpoint must be 0 (off), an interval >= 1 or -1 (automatic), not %d" % value
