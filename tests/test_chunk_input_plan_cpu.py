"""CPU: the host half of the chunk minibatch inputs (include/tdnnf_hip.h, "CHUNK INPUTS"; tdnn-f_nas_amd/csrc/chunk_input_plan.h).
tdnnf_chunk_input_plan gives the table of the numpy statement (tests/chunk_input_ref.py) for random small minibatches -- each with a chunk at
begin 0 and one ending at O_u, every frame_shift in -(fsf - 1) .. fsf - 1, ivector_period 10 and <= 0 --, every refusal of the definition
is raised by name, and the same header runs as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/chunk_input_driver.cc) on the same minibatches.  Then the chunk order of egs.minibatches_from_utterances, which is host arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from tests import chunk_input_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    """(fsf, T, seq_utt, begins, frames, ivector_rows or None, period, frame_shift)"""
    rng = np.random.default_rng(11)
    out = []
    for fsf, T in ((3, 4), (1, 5), (2, 1), (3, 50)):
        for period in (10, 0, -1):
            for shift in range(-(fsf - 1), fsf):
                for with_rows in ((True, False) if period > 0 else (True,)):
                    seq_utt, begins, frames, rows = ref.random_case(rng, fsf, T, period, with_rows)
                    out.append((fsf, T, seq_utt, begins, frames, rows, period, shift))
    return out


def test_plan_is_the_numpy_table(pkg):
    plan = pkg.hipabi.ChunkInput.plan
    seen = set()
    for fsf, T, seq_utt, begins, frames, rows, period, shift in cases():
        O = [ref.output_frames(f, fsf) for f in frames]
        assert 0 in begins and any(o + T == O[u] for u, o in zip(seq_utt, begins))
        want = ref.table(fsf, T, seq_utt, begins, frames, rows, period, shift)
        got = plan(fsf, T, seq_utt, begins, frames, rows, period, shift)
        assert got.dtype == np.int32 and np.array_equal(got, want), (fsf, T, period, shift)
        seen.add((fsf, shift, period > 0))
    assert {(3, s, p) for s in range(-2, 3) for p in (True, False)} <= seen
    # period <= 0 reads no row counts: one row an utterance
    assert np.array_equal(plan(3, 4, [2, 0], [0, 1], [13, 30, 12], None, 0)[:, 3], [2, 0])
    # the middle of the chunk, and the last row where the middle lies behind it
    assert plan(3, 4, [1, 1, 1], [0, 2, 6], [13, 30, 12], [1, 2, 3], 10)[:, 3].tolist() == [1 + 0, 1 + 1, 1 + 1]


def test_every_refusal_names_what_it_refuses(pkg):
    plan = pkg.hipabi.ChunkInput.plan
    frames, rows, utt, begin = [13, 30, 12], [1, 2, 3], [0, 1, 2], [1, 6, 0]  # O = 5, 10, 4
    at = lambda a, i, v: list(a[:i]) + [v] + list(a[i + 1:])

    def refused(words, *args):
        with pytest.raises(pkg.hipabi.HipAbiError) as e:
            plan(*args)
        assert "tdnnf error 1:" in str(e.value) and "chunk_input_plan: " + words in str(e.value), str(e.value)

    plan(3, 4, utt, begin, frames, rows, 10, 0)
    refused("sequence 1: the chunk begins at frame -1", 3, 4, utt, at(begin, 1, -1), frames, rows, 10, 0)
    refused("sequence 0: the chunk of 4 frames from frame 2 ends behind the 5 output frames of the utterance", 3, 4, utt, at(begin, 0, 2), frames, rows, 10, 0)
    refused("sequence 2: the chunk of 4 frames from frame 1 ends behind the 4 output frames", 3, 4, utt, at(begin, 2, 1), frames, rows, 10, 0)
    refused("sequence 2: utterance 3 outside [0, 3)", 3, 4, at(utt, 2, 3), begin, frames, rows, 10, 0)
    refused("sequence 0: utterance -1 outside [0, 3)", 3, 4, at(utt, 0, -1), begin, frames, rows, 10, 0)
    refused("utterance 1 has 0 frames", 3, 4, utt, begin, at(frames, 1, 0), rows, 10, 0)
    refused("utterance 2 has no i-vector rows (0)", 3, 4, utt, begin, frames, at(rows, 2, 0), 10, 0)
    for shift in (3, -3, 7):
        refused("frame_shift %d: its magnitude must be below frame_subsampling 3" % shift, 3, 4, utt, begin, frames, rows, 10, shift)
    # without i-vectors (period > 0, no row counts) and with one row an utterance the counts are not looked at
    assert plan(3, 4, utt, begin, frames, None, 10, 0)[:, 3].tolist() == [0, 0, 0]
    assert plan(3, 4, utt, begin, frames, at(rows, 2, 0), 0, 0)[:, 3].tolist() == [0, 1, 2]
    with pytest.raises(pkg.hipabi.HipAbiError, match="3 seq_utt and 2 chunk_begins"):
        plan(3, 4, utt, begin[:2], frames, rows, 10, 0)


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "chunk_input_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "chunk_input_driver.cc"), "-o", str(exe)])
    all_cases = cases()
    with open(tmp_path / "minibatches.txt", "w") as f:
        for fsf, T, seq_utt, begins, frames, rows, period, shift in all_cases:
            f.write("%d %d %d %d %d %d %d\n" % (fsf, T, len(seq_utt), len(frames), shift, period, rows is not None))
            for a in (seq_utt, begins, frames, rows or [], ref.table(fsf, T, seq_utt, begins, frames, rows, period, shift).reshape(-1)):
                f.write(" ".join("%d" % x for x in a) + "\n")
    out = subprocess.run([str(exe), str(tmp_path / "minibatches.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failures" and lines[0] == "plans: %d minibatches" % len(all_cases) and len(all_cases) >= 40, out.stdout
    assert sum(line.startswith("refusal: driver: ") for line in lines) == 11, out.stdout


def test_chunk_order_of_an_epoch(pkg):
    E = pkg.egs
    out_frames = [8, 20, 5, 17, 16]  # T = 8: 1 + 3 + 0 + 3 + 2 chunks
    chunks = E.utterance_chunks(out_frames, 8)
    assert chunks == [(0, 0), (1, 0), (1, 6), (1, 12), (3, 0), (3, 4), (3, 9), (4, 0), (4, 8)]
    assert all(o in pkg.infer.chunk_begins(out_frames[u], 8) for u, o in chunks) and not any(u == 2 for u, _ in chunks)
    a, b, c = (E.chunk_minibatches(chunks, 3, seed) for seed in (0, 0, 1))
    assert a == b and a != c and [len(m) for m in a] == [3, 3, 3]
    assert sorted(ch for m in a for ch in m) == sorted(chunks) == sorted(ch for m in c for ch in m)
    assert E.chunk_minibatches(chunks, 3, 0, discard_partial=False) == a
    # 9 chunks in fours: the partial minibatch is dropped, or refused
    four = E.chunk_minibatches(chunks, 4, 0)
    assert [len(m) for m in four] == [4, 4] and len({ch for m in four for ch in m}) == 8
    with pytest.raises(ValueError, match="the last 1 chunks do not fill a minibatch of 4"):
        E.chunk_minibatches(chunks, 4, 0, discard_partial=False)
