"""Chunk plan of forward-only inference (tdnnf_chunk_plan / tdnnf_infer_plan, include/tdnnf_hip.h "inference") against a
Python restatement of the contract, and the Kaldi float-matrix archive writer.  Host only: no GPU."""
import ctypes as C
import struct

import numpy as np
import pytest


def plan_ref(F, fsf, frames, ivector_rows, period):
    """The contract: chunk k of utterance u covers input frames [kF, kF + F); n_k of its Tout = F / fsf output rows lie inside
    O_u = ceil(T_u / fsf); its i-vector row is min(((kF / fsf) + n_k / 2) * fsf / period, R_u - 1) (0 for period <= 0)."""
    Tout, out = F // fsf, []
    for u, T in enumerate(frames):
        O = (T + fsf - 1) // fsf
        R = ivector_rows[u] if period > 0 else 1
        k = 0
        while k * Tout < O:
            n = min(Tout, O - k * Tout)
            row = min(((k * F // fsf) + n // 2) * fsf // period, R - 1) if period > 0 else 0
            out.append((u, k * F, row, n))
            k += 1
    return np.asarray(out, np.int32).reshape(-1, 4)


def chunk_plan(pkg, F, fsf, frames, ivector_rows, period, capacity=None):
    lib = pkg.hipabi.load()
    fr, frp = pkg.hipabi.iarr(frames)
    ivr, ivp = pkg.hipabi.iarr(ivector_rows)
    n = C.c_int()
    cap = 4096 if capacity is None else capacity
    out = np.full((max(cap, 1), 4), -7, np.int32)
    rc = lib.tdnnf_chunk_plan(F, fsf, len(fr), frp, ivp, period, out.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n))
    return rc, n.value, out


def ivector_rows_for(frames, period):
    return [max(1, -(-t // period)) for t in frames]


@pytest.mark.parametrize("F", [51, 150])
@pytest.mark.parametrize("period", [10, 0, -1])
def test_plan_matches_the_contract(pkg, F, period):
    fsf = 3
    frames = [1, fsf - 1, F - 1, F, F + 1, int(3.5 * F), 7, 2 * F + 2]
    rows = ivector_rows_for(frames, 10)
    rc, n, out = chunk_plan(pkg, F, fsf, frames, rows, period)
    assert rc == 0
    ref = plan_ref(F, fsf, frames, rows, period)
    assert n == len(ref)
    assert np.array_equal(out[:n], ref)
    # every output row of every utterance is covered exactly once
    for u, T in enumerate(frames):
        mine = ref[ref[:, 0] == u]
        assert mine[:, 3].sum() == -(-T // fsf)
        assert np.array_equal(mine[:, 1], np.arange(len(mine)) * F)


def test_plan_many_utterances(pkg):
    rng = np.random.default_rng(5)
    frames = rng.integers(1, 1600, size=300).tolist()
    rows = [r + int(rng.integers(0, 3)) for r in ivector_rows_for(frames, 10)]  # (extra rows are never chosen past the middle)
    rc, n, out = chunk_plan(pkg, 150, 3, frames, rows, 10, capacity=20000)
    ref = plan_ref(150, 3, frames, rows, 10)
    assert rc == 0 and n == len(ref) and np.array_equal(out[:n], ref)


def test_plan_ivector_row_is_the_middle_of_the_chunk(pkg):
    # one utterance of 400 frames, F = 150, period 10: chunks at 0, 150, 300 with 50, 50, 34 output rows
    rc, n, out = chunk_plan(pkg, 150, 3, [400], [40], 10)
    assert rc == 0 and n == 3
    assert out[:3].tolist() == [[0, 0, 7, 50], [0, 150, 22, 50], [0, 300, 35, 34]]
    # fewer i-vector rows than the middle asks for: the last one
    rc, n, out = chunk_plan(pkg, 150, 3, [400], [30], 10)
    assert out[2].tolist() == [0, 300, 29, 34]


def test_plan_capacity_error(pkg):
    lib = pkg.hipabi.load()
    frames = [500, 500]
    ref = plan_ref(51, 3, frames, [50, 50], 10)
    rc, n, out = chunk_plan(pkg, 51, 3, frames, [50, 50], 10, capacity=len(ref) - 1)
    assert rc == 1 and n == len(ref)
    assert np.array_equal(out[:len(ref) - 1], ref[:-1])
    assert b"capacity" in lib.tdnnf_last_error()


@pytest.mark.parametrize("F", [50, 0, -3])
def test_plan_chunk_width_must_be_a_multiple_of_the_subsampling(pkg, F):
    lib = pkg.hipabi.load()
    rc, n, out = chunk_plan(pkg, F, 3, [100], [10], 10)
    assert rc == 1
    assert b"frame_subsampling" in lib.tdnnf_last_error()


def test_plan_needs_ivector_rows(pkg):
    lib = pkg.hipabi.load()
    fr, frp = pkg.hipabi.iarr([100, 200])
    n = C.c_int()
    out = np.zeros((16, 4), np.int32)
    assert lib.tdnnf_chunk_plan(150, 3, 2, frp, None, 10, out.ctypes.data_as(C.POINTER(C.c_int)), 16, C.byref(n)) == 1
    assert lib.tdnnf_chunk_plan(150, 3, 2, frp, None, 0, out.ctypes.data_as(C.POINTER(C.c_int)), 16, C.byref(n)) == 0
    assert n.value == 3 and out[:3, 2].tolist() == [0, 0, 0]


def read_matrix_archive(path):
    """Kaldi binary archive of float matrices, read back independently of the writer."""
    raw = open(path, "rb").read()
    items, pos = [], 0
    while pos < len(raw):
        sp = raw.index(b" ", pos)
        key = raw[pos:sp].decode()
        pos = sp + 1
        assert raw[pos:pos + 2] == b"\0B"
        pos += 2
        assert raw[pos:pos + 3] == b"FM "
        pos += 3
        s1, rows, s2, cols = struct.unpack("<bibi", raw[pos:pos + 10])
        assert s1 == 4 and s2 == 4
        pos += 10
        m = np.frombuffer(raw[pos:pos + 4 * rows * cols], dtype="<f4").reshape(rows, cols)
        pos += 4 * rows * cols
        items.append((key, m))
    return items


def test_matrix_archive_round_trip(pkg, tmp_path):
    rng = np.random.default_rng(1)
    items = [("utt-a", rng.standard_normal((17, 50)).astype(np.float32)), ("utt-b", np.zeros((1, 50), np.float32)),
             ("utt_c", rng.standard_normal((334, 6)).astype(np.float32))]
    path = tmp_path / "out.ark"
    pkg.infer.write_matrix_archive(path, items)
    back = read_matrix_archive(path)
    assert [k for k, _ in back] == [k for k, _ in items]
    for (_, a), (_, b) in zip(items, back):
        assert np.array_equal(a, b)
    # the project's own Kaldi matrix reader takes one entry of it (a lone binary matrix = the archive entry without its key)
    single = tmp_path / "one.mat"
    open(single, "wb").write(open(path, "rb").read()[len(b"utt-a "):len(b"utt-a ") + 15 + 4 * 17 * 50])
    assert np.array_equal(pkg.trainer.read_kaldi_matrix(single), items[0][1])
