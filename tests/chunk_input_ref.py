"""The net's input for a minibatch of chunks of whole utterances (include/tdnnf_hip.h, "CHUNK INPUTS") stated from its definition in plain
numpy, one row at a time: the table tdnnf_chunk_input_plan reports, feats_out and ivectors_out.  utts: a list of (feats [frames, feat_dim],
ivectors [R_u, ivector_dim] or None) host arrays; a sequence is (utterance, begin) with begin in output frames."""
import numpy as np


def output_frames(frames, fsf):
    return (int(frames) + fsf - 1) // fsf


def ivector_row(begin, T, fsf, period, R):
    """the row within the utterance: the middle of the chunk, integer divisions; one per utterance for period <= 0"""
    return min(((begin + T // 2) * fsf) // period, R - 1) if period > 0 else 0


def table(fsf, T, seq_utt, begins, frames, ivector_rows, period, frame_shift):
    """int32 (B, 4): first stacked feature row of the utterance, its frames, the window start, the stacked i-vector row (ivector_rows None
    with period > 0: no i-vectors, 0)"""
    use_iv = period <= 0 or ivector_rows is not None
    R = [(int(ivector_rows[u]) if period > 0 else 1) if use_iv else 0 for u in range(len(frames))]
    feat0 = np.concatenate([[0], np.cumsum(frames)])
    iv0 = np.concatenate([[0], np.cumsum(R)])
    rows = []
    for u, o in zip(seq_utt, begins):
        rows.append([feat0[u], frames[u], o * fsf - frame_shift, iv0[u] + ivector_row(o, T, fsf, period, R[u]) if use_iv else 0])
    return np.asarray(rows, np.int32).reshape(-1, 4)


def gather(first_t, num_t, fsf, T, seq_utt, begins, utts, period, frame_shift):
    """(feats_out [num_t * B, feat_dim] t-major, ivectors_out [B, ivector_dim] or None)"""
    B = len(seq_utt)
    D = utts[0][0].shape[1]
    out = np.zeros((num_t * B, D), np.float32)
    with_iv = utts[0][1] is not None and utts[0][1].shape[1] > 0
    iv_out = np.zeros((B, utts[0][1].shape[1]), np.float32) if with_iv else None
    for b, (u, o) in enumerate(zip(seq_utt, begins)):
        f, iv = utts[u]
        assert 0 <= o and o + T <= output_frames(len(f), fsf) and abs(frame_shift) < fsf
        for t in range(first_t, first_t + num_t):
            out[(t - first_t) * B + b] = f[min(max(o * fsf + t - frame_shift, 0), len(f) - 1)]
        if with_iv:
            iv_out[b] = iv[ivector_row(o, T, fsf, period, len(iv) if period > 0 else 1)]
    return out, iv_out


def stacked(utts, period):
    """(feats, ivectors or None, frames, ivector_rows) as the C entries take them: period <= 0 keeps every utterance's first i-vector row"""
    with_iv = utts[0][1] is not None and utts[0][1].shape[1] > 0
    ivs = [(iv if period > 0 else iv[:1]) for _, iv in utts] if with_iv else None
    return (np.concatenate([f for f, _ in utts]), np.concatenate(ivs) if with_iv else None, [len(f) for f, _ in utts],
            [len(iv) for iv in ivs] if with_iv else None)


def random_case(rng, fsf, T, period, with_ivector_rows=True):
    """(seq_utt, begins, frames, ivector_rows or None) of a small random minibatch that holds a chunk at begin 0 and one ending at O_u"""
    U = int(rng.integers(2, 5))
    frames = [int(rng.integers((T - 1) * fsf + 1, (T + 9) * fsf)) for _ in range(U)]
    rows = [int(rng.integers(1, 5)) for _ in range(U)] if with_ivector_rows else None
    seq_utt, begins = [0, U - 1], [0, output_frames(frames[U - 1], fsf) - T]
    for _ in range(int(rng.integers(1, 6))):
        u = int(rng.integers(0, U))
        seq_utt.append(u)
        begins.append(int(rng.integers(0, output_frames(frames[u], fsf) - T + 1)))
    order = rng.permutation(len(seq_utt))
    return [seq_utt[i] for i in order], [begins[i] for i in order], frames, rows
