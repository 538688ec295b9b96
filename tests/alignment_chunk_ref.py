"""The supervision lattice of a chunk of an utterance (include/tdnnf_hip.h, "ALIGNMENT CHUNKS") stated from its definition: build the
utterance's lattice U with alignment_supervision_ref.sequence, keep the states of the times [o + 1, o + T], re-time them, add the start
and its arcs, set the finals.  No closed form of tdnn-f_nas_amd/csrc/chain_sup_alignment.h.  lattice() returns the supervision dict of
synth.make_supervision, which Supervision.assign takes.  Also the minibatches the tests of the feature share
(tests/test_alignment_chunk_ref.py, tests/test_alignment_chunk_plan_cpu.py, tests/test_gpu_assign_alignment_chunks.py).
A chunk is a triple (alignment, utt_frames, chunk_begin), alignment the (units, starts) pair of the whole utterance."""
import numpy as np

from tests import alignment_supervision_ref as ali

UTT_FRAMES = (2, 7, 40)
CHUNK_FRAMES = (1, 2, 7)


def tolerances(utt_frames):
    return (0, 1, 2, 5, utt_frames + 3)


def begins(utt_frames, T):
    """0, 1, the middle and the last begin there is, those that exist"""
    return sorted({o for o in (0, 1, (utt_frames - T) // 2, utt_frames - T) if 0 <= o <= utt_frames - T})


def utterance_states(units, starts, utt_frames, tol):
    """the (time, kind, unit) triples of U in its state order, as alignment_supervision_ref.sequence numbers them: kind -1 the start, 0 E, 1 L"""
    n = len(units)
    lo, hi = ali.windows(starts, utt_frames, tol)
    states = [(0, -1, 0)]
    states += [(t, 0, k) for k in range(n) for t in range(lo[k] + 1, hi[k] + 2)]
    states += [(t, 1, k) for k in range(n) for t in range(lo[k] + 2, hi[k + 1] + 1)]
    return sorted(states)


def kept_states(units, starts, utt_frames, o, T, tol):
    """the numbers in U of the states a chunk keeps, in order: the chunk's state 1 + j is U's state kept[j]"""
    return [i for i, (t, _, _) in enumerate(utterance_states(units, starts, utt_frames, tol)) if o + 1 <= t <= o + T]


def sequence(us, units, starts, utt_frames, o, T, tol):
    """(state_time, final, [(src, dst, pdf)]) of one chunk, states numbered from 0"""
    assert 0 <= o and o + T <= utt_frames and T >= 1
    time, _, arcs = ali.sequence(us, units, starts, utt_frames, tol)
    states = utterance_states(units, starts, utt_frames, tol)
    assert [s[0] for s in states] == list(time)
    kept = kept_states(units, starts, utt_frames, o, T, tol)
    new = {i: 1 + j for j, i in enumerate(kept)}
    out = []
    for i in kept:  # the start's arcs, in state order
        t, kind, k = states[i]
        if t == o + 1:
            left = units[k - 1] if k else -1
            out.append((0, new[i], ali.entry_pdf(us, left, units[k]) if kind == 0 else ali.loop_pdf(us, left, units[k])))
    out += [(new[s], new[d], p) for s, d, p in arcs if s in new and d in new]
    assert out == sorted(out, key=lambda a: (a[0], a[1]))
    new_time = [0] + [states[i][0] - o for i in kept]
    final = [0.0 if t == T else -np.inf for t in new_time]
    return new_time, final, out


def lattice(us, chunks, T, tol, weight=1.0):
    """The supervision dict of a minibatch of chunks: [((units, starts), utt_frames, chunk_begin)], us a unit set dict"""
    time, final, src, dst, pdf = [], [], [], [], []
    ssb, sab = [0], [0]
    for (units, starts), utt_frames, o in chunks:
        t, f, arcs = sequence(us, [int(u) for u in units], [int(b) for b in starts], int(utt_frames), int(o), T, tol)
        base = ssb[-1]
        time += t
        final += f
        src += [base + a[0] for a in arcs]
        dst += [base + a[1] for a in arcs]
        pdf += [a[2] for a in arcs]
        ssb.append(base + len(t))
        sab.append(len(src))
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": len(chunks), "T": int(T), "seq_state_begin": i32(ssb), "seq_arc_begin": i32(sab), "state_time": i32(time),
            "final_logprob": np.asarray(final, dtype=np.float32), "arc_src": i32(src), "arc_dst": i32(dst), "arc_pdf": i32(pdf),
            "arc_logprob": np.zeros(len(src), np.float32), "weight": float(weight)}


def small_batch(utt_frames, T):
    """every begin of begins() in each utterance of alignment_supervision_ref.small_batch: one unit; units of one frame each; a random
    segmentation"""
    return [(al, utt_frames, o) for al in ali.small_batch(utt_frames) for o in begins(utt_frames, T)]


def small_batches():
    """[(chunks, T, tolerance)]"""
    return [(small_batch(Tu, T), T, tol) for Tu in UTT_FRAMES for T in CHUNK_FRAMES if T <= Tu for tol in tolerances(Tu)]


def narrow_batch():
    """B = 4, T = 150 from 400-frame utterances, tolerance 5: narrow (`wide` false)"""
    rng = np.random.default_rng(17)
    return [(ali.random_alignment(rng, 400, mean_dur=8.0), 400, int(rng.integers(0, 251))) for _ in range(4)], 150, 5


def wide_batch():
    """B = 2, T = 60 from 150-frame utterances, mean duration 1.5, tolerance 40: `wide` true"""
    rng = np.random.default_rng(18)
    return [(ali.random_alignment(rng, 150, mean_dur=1.5), 150, o) for o in (31, 90)], 60, 40


def minibatches():
    return small_batches() + [narrow_batch(), wide_batch()]


def flat(chunks):
    """(unit_begin, units, starts, utt_frames, chunk_begin) int32 arrays as the C entries take them"""
    begin, units, starts = ali.flat([c[0] for c in chunks])
    return begin, units, starts, np.asarray([c[1] for c in chunks], np.int32), np.asarray([c[2] for c in chunks], np.int32)


def named_units(units, starts, utt_frames, o, T, tol):
    """the numbers in the utterance of the units a chunk's lattice names: of its states, and the left neighbours their pdfs are read at"""
    states = utterance_states(units, starts, utt_frames, tol)
    ks = {k for t, kind, k in states if kind >= 0 and o + 1 <= t <= o + T}
    return ks | {k - 1 for k in ks if k > 0}
