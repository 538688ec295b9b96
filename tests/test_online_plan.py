"""Step schedule of streaming inference (tdnnf_online_schedule, include/tdnnf_hip.h "inference (forward only, streaming)") against a
numpy restatement of the contract.  Host only: no GPU."""
import ctypes as C

import numpy as np
import pytest


def schedule_ref(F, fsf, left, right, T):
    """The contract: latency D = right rounded up to fsf, warm-up W = left rounded up to F; steps at clock = -W, -W + F, ... while
    clock - D < T.  A step passes the real frames of its window [clock, clock + F) -- frame 0 alone before the utterance, the last
    frame alone after it -- and keeps the outputs at frames clock - D, clock - D + fsf, ... < clock - D + F that lie in [0, T)."""
    D, W = -(-right // fsf) * fsf, -(-left // F) * F
    steps, clock = [], -W
    while clock - D < T:
        real = [t for t in range(clock, clock + F) if 0 <= t < T]
        if real:
            first, n = real[0], len(real)
        else:
            first, n = (0, 1) if clock < 0 else (T - 1, 1)
        kept = [t // fsf for t in range(clock - D, clock - D + F, fsf) if 0 <= t < T]
        steps.append((clock, first, n, kept[0] if kept else max((clock - D) // fsf, 0), len(kept)))
        clock += F
    return np.asarray(steps, np.int32).reshape(-1, 5)


def schedule(pkg, F, fsf, left, right, T, capacity=4096):
    lib = pkg.hipabi.load()
    n = C.c_int()
    out = np.full((max(capacity, 1), 5), -7, np.int32)
    rc = lib.tdnnf_online_schedule(F, fsf, left, right, T, out.ctypes.data_as(C.POINTER(C.c_int)), capacity, C.byref(n))
    return rc, n.value, out


CONTEXTS = [(9, 9), (9, 7), (4, 0), (40, 10), (0, 2), (1, 1)]  # right = 0, left > F, contexts that are no multiple of fsf


@pytest.mark.parametrize("F", [3, 24, 30])
@pytest.mark.parametrize("left,right", CONTEXTS)
def test_schedule_matches_the_contract(pkg, F, left, right):
    fsf = 3
    D = -(-right // fsf) * fsf
    for T in sorted({1, 2, F - 1, F, F + 1, 3 * F + 2}):
        rc, n, out = schedule(pkg, F, fsf, left, right, T)
        ref = schedule_ref(F, fsf, left, right, T)
        assert rc == 0 and n == len(ref), (T, n, len(ref))
        assert np.array_equal(out[:n], ref), (T, out[:n], ref)
        s = out[:n]
        # the kept output rows are exactly 0 .. ceil(T / fsf) - 1, each once and in order
        rows = np.concatenate([np.arange(a, a + k) for a, k in zip(s[:, 3], s[:, 4])])
        assert np.array_equal(rows, np.arange(-(-T // fsf))), (T, rows)
        # the first step starts at least `left` frames before the utterance, on a multiple of F
        assert s[0, 0] <= -left and s[0, 0] % F == 0 and np.array_equal(np.diff(s[:, 0]), np.full(n - 1, F))
        for clock, first, rows_passed, out0, kept in s:
            final = clock >= 0 and clock + F >= T
            if not final:
                # no window needs a frame >= T before `final`: it passes real frames only, and the last output it keeps
                # reaches no further right than its own last frame
                assert first + rows_passed <= T
                if clock >= 0:
                    assert rows_passed == F and first == clock
                if kept:
                    assert clock >= 0 and (out0 + kept - 1) * fsf + right <= clock + F - 1
            else:
                assert 1 <= rows_passed <= F and first + rows_passed == T
            # a frame is passed once, except frame 0 (warm-up) and the last one (flush) as clamp sources
            assert (first, rows_passed) in ((0, 1), (T - 1, 1)) or first == clock
        # the slot is done right after the last step
        assert s[-1, 0] - D < T <= s[-1, 0] + F - D


@pytest.mark.parametrize("F", [31, 0, -3])
def test_schedule_step_width_must_be_a_multiple_of_the_subsampling(pkg, F):
    lib = pkg.hipabi.load()
    rc, n, out = schedule(pkg, F, 3, 9, 9, 100)
    assert rc == 1
    assert b"frame_subsampling" in lib.tdnnf_last_error()


def test_schedule_capacity_error(pkg):
    lib = pkg.hipabi.load()
    ref = schedule_ref(30, 3, 9, 9, 200)
    rc, n, out = schedule(pkg, 30, 3, 9, 9, 200, capacity=len(ref) - 1)
    assert rc == 1 and n == len(ref)
    assert np.array_equal(out[:len(ref) - 1], ref[:-1])
    assert b"capacity" in lib.tdnnf_last_error()
    # the Python wrapper sizes the array itself
    assert np.array_equal(pkg.infer.online_schedule(30, 3, 9, 9, 200), ref)
