"""ctypes plumbing of the egs reader / writer / merge in csrc/egs_io.hip (include/tdnnf_hip.h, "egs" section): chain
example archives in Kaldi's binary format (restated, see the header of egs_io.hip) to and from numpy, and the merge of
single-sequence examples into the minibatch the trainer takes.  Host only, no GPU needed -- but for the minibatch generators, which
hand device objects to the trainer: from an archive (minibatches), or straight from aligned utterances with the features gathered and
the supervisions compiled on the device (minibatches_from_utterances; write_chunk_egs is its host route into an archive), or with the
features held as Kaldi's compressed codes (minibatches_from_store; read_feature_archive / write_feature_archive: feature archives)."""
import ctypes as C

import numpy as np

from . import hipabi


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Eg:
    """One NnetChainExample read from an archive."""

    def __init__(self, handle):
        self.lib = hipabi.load()
        self.h = handle
        self.key = self.lib.tdnnf_eg_key(self.h).decode()

    def close(self):
        if self.h:
            self.lib.tdnnf_eg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def input(self, name="input"):
        """(matrix rows x cols, time of the first row)"""
        r, c, t0 = C.c_int(), C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_eg_input_info(self.h, name.encode(), C.byref(r), C.byref(c), C.byref(t0)))
        out = np.zeros((r.value, c.value), np.float32)
        hipabi.check(self.lib.tdnnf_eg_input_copy(self.h, name.encode(), _p(out)))
        return out, t0.value

    def supervision_info(self):
        w = C.c_float()
        v = [C.c_int() for _ in range(7)]
        hipabi.check(self.lib.tdnnf_eg_supervision_info(self.h, C.byref(w), *[C.byref(x) for x in v]))
        keys = ("num_sequences", "frames_per_seq", "label_dim", "num_states", "num_arcs", "first_t", "t_step")
        return dict(weight=w.value, **{k: x.value for k, x in zip(keys, v)})


class Reader:
    """Iterates over the examples of one archive:  for eg in Reader(path): ..."""

    def __init__(self, path):
        self.lib = hipabi.load()
        self.h = C.c_void_p()
        hipabi.check(self.lib.tdnnf_egs_reader_open(str(path).encode(), C.byref(self.h)))

    def __iter__(self):
        return self

    def __next__(self):
        eg = C.c_void_p()
        hipabi.check(self.lib.tdnnf_egs_reader_next(self.h, C.byref(eg)))
        if not eg.value:
            self.close()
            raise StopIteration
        return Eg(eg)

    def close(self):
        if self.h:
            self.lib.tdnnf_egs_reader_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge(egs, first_t, num_t, frame_shift=0, with_ivectors=True):
    """nnet3-chain-merge-egs (+ --frame-shift of nnet3-chain-copy-egs) for single-sequence examples: returns
    (feats (num_t * n) x D t-major, ivectors n x Di or None, supervision dict in the form hipabi.Supervision takes)."""
    lib = hipabi.load()
    n = len(egs)
    arr = (C.c_void_p * n)(*[e.h for e in egs])
    ns, na, T, D, Di = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    hipabi.check(lib.tdnnf_egs_merge_sizes(arr, n, C.byref(ns), C.byref(na), C.byref(T), C.byref(D), C.byref(Di)))
    feats = np.zeros((num_t * n, D.value), np.float32)
    iv = np.zeros((n, Di.value), np.float32) if with_ivectors and Di.value else None
    sup = dict(B=n, T=T.value, seq_state_begin=np.zeros(n + 1, np.int32), seq_arc_begin=np.zeros(n + 1, np.int32),
               state_time=np.zeros(ns.value, np.int32), final_logprob=np.zeros(ns.value, np.float32), arc_src=np.zeros(na.value, np.int32),
               arc_dst=np.zeros(na.value, np.int32), arc_pdf=np.zeros(na.value, np.int32), arc_logprob=np.zeros(na.value, np.float32))
    w = C.c_float()
    hipabi.check(lib.tdnnf_egs_merge(arr, n, int(first_t), int(num_t), int(frame_shift), _p(feats), _p(iv) if iv is not None else None,
                                     _p(sup["seq_state_begin"]), _p(sup["seq_arc_begin"]), _p(sup["state_time"]), _p(sup["final_logprob"]),
                                     _p(sup["arc_src"]), _p(sup["arc_dst"]), _p(sup["arc_pdf"]), _p(sup["arc_logprob"]), C.byref(w)))
    sup["weight"] = float(w.value)
    return feats, iv, sup


def sequence_of(sup, b):
    """Sequence b of a minibatch supervision dict (synth.make_supervision) as one sequence's local arrays, state 0 = start."""
    s0, s1 = int(sup["seq_state_begin"][b]), int(sup["seq_state_begin"][b + 1])
    a0, a1 = int(sup["seq_arc_begin"][b]), int(sup["seq_arc_begin"][b + 1])
    assert sup["state_time"][s0] == 0 and (sup["state_time"][s0 + 1:s1] > 0).all(), "state 0 of the sequence must be its start state"
    return dict(final_logprob=np.ascontiguousarray(sup["final_logprob"][s0:s1], np.float32), arc_src=np.ascontiguousarray(sup["arc_src"][a0:a1] - s0, np.int32),
                arc_dst=np.ascontiguousarray(sup["arc_dst"][a0:a1] - s0, np.int32), arc_pdf=np.ascontiguousarray(sup["arc_pdf"][a0:a1], np.int32),
                arc_logprob=np.ascontiguousarray(sup["arc_logprob"][a0:a1], np.float32), frames=int(sup["T"]), weight=float(sup.get("weight", 1.0)))


class Writer:
    def __init__(self, path):
        self.lib = hipabi.load()
        self.h = C.c_void_p()
        hipabi.check(self.lib.tdnnf_egs_writer_open(str(path).encode(), C.byref(self.h)))

    def write(self, key, feats, first_t, seq, label_dim, ivector=None, compress=True, t_step=3):
        """seq: one sequence's supervision (sequence_of)."""
        feats = np.ascontiguousarray(feats, np.float32)
        iv = np.ascontiguousarray(ivector, np.float32).reshape(-1) if ivector is not None else None
        hipabi.check(self.lib.tdnnf_egs_writer_write(
            self.h, key.encode(), _p(feats), feats.shape[0], feats.shape[1], int(first_t), _p(iv) if iv is not None else None, iv.size if iv is not None else 0,
            int(bool(compress)), float(seq["weight"]), int(seq["frames"]), int(t_step), int(label_dim), seq["final_logprob"].size, seq["arc_src"].size,
            _p(seq["final_logprob"]), _p(seq["arc_src"]), _p(seq["arc_dst"]), _p(seq["arc_pdf"]), _p(seq["arc_logprob"])))

    def close(self):
        if self.h:
            h, self.h = self.h, None
            hipabi.check(self.lib.tdnnf_egs_writer_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ReusedSupervision:
    """One reserved hipabi.Supervision (tdnnf_supervision_reserve) that takes minibatch after minibatch by assign: no allocation, no
    device-wide wait per minibatch.  It is sized from the first minibatch -- its sequences and frames, its states and arcs with HEADROOM --
    and reserved again, larger, when a minibatch exceeds a capacity (the old handle is destroyed, which waits for the device once).
    .reserves counts the reserves; the handle carries the same number as its .reserves attribute."""
    HEADROOM = 1.25

    def __init__(self):
        self.sup, self.caps, self.reserves = None, (0, 0, 0, 0), 0

    def _room_for(self, need):
        """a handle of at least `need` = (sequences, frames, states, arcs): the one there is, or a new one with HEADROOM"""
        if self.sup is None or any(n > c for n, c in zip(need, self.caps)):
            room = (need[0], need[1], int(need[2] * self.HEADROOM) + 1, int(need[3] * self.HEADROOM) + 1)
            self.caps = tuple(max(c, r) for c, r in zip(self.caps, room))
            self.sup = None  # (the old handle goes first: its memory is free for the new one)
            self.sup = hipabi.Supervision.reserve(*self.caps)
            self.reserves += 1
        self.sup.reserves = self.reserves

    def assign(self, s):
        """The handle holding supervision dict `s`; valid until the next assign."""
        self._room_for((int(s["B"]), int(s["T"]), len(s["state_time"]), len(s["arc_src"])))
        self.sup.assign(s)
        return self.sup

    def assign_alignment_chunks(self, unit_set, alignments, utt_frames, chunk_begins, frames_per_sequence, tolerance, weight=1.0):
        """The handle holding the chunks' supervisions, compiled on the device (hipabi.Supervision.assign_alignment_chunks); it is sized
        with UnitSet.alignment_chunk_sizes, host arithmetic.  Valid until the next assign."""
        states, arcs = unit_set.alignment_chunk_sizes(alignments, utt_frames, chunk_begins, frames_per_sequence, tolerance)
        self._room_for((len(states), int(frames_per_sequence), int(states.sum()), int(arcs.sum())))
        self.sup.assign_alignment_chunks(unit_set, alignments, utt_frames, chunk_begins, frames_per_sequence, tolerance, weight)
        return self.sup


def minibatches(path, net, frame_shift=0, discard_partial=True, prefetch=0, reuse=False):
    """Reads an archive and yields (feats, ivectors, hipabi.Supervision) device objects for ChainNet.forward_backward, merging
    net.cfg.num_sequences examples at a time in archive order (nnet3-chain-merge-egs --minibatch-size; the archive is expected to
    be shuffled already, as nnet3-chain-shuffle-egs leaves it).  prefetch > 0: reading, decompression and the merge run on a
    worker thread that many minibatches ahead (the C calls release the GIL), the copy to the device stays on the caller.
    reuse: every item carries the SAME supervision handle, a reserved one that is assigned the minibatch on the current stream
    (ReusedSupervision: its tables are built on the device, nothing is allocated or freed per minibatch; .reserves on the handle says how
    often it had to be reserved).  A yielded supervision is then valid until the next item is requested: work enqueued on the current
    stream before that still sees it, a reference kept beyond it sees the next minibatch.  Default: a new hipabi.Supervision per item."""
    import torch
    B = net.cfg.num_sequences
    first_t, num_t, with_iv = net.first_t, net.num_t_in, net.cfg.ivector_dim > 0
    chunk, sub = net.cfg.frames_per_chunk, net.cfg.frame_subsampling

    def host_batches():
        group = []
        reader = Reader(path)
        try:
            for eg in reader:
                group.append(eg)
                if len(group) == B:
                    f, iv, sup = merge(group, first_t, num_t, frame_shift, with_ivectors=with_iv)
                    for e in group:
                        e.close()
                    group = []
                    if sup["T"] * sub != chunk:
                        raise ValueError("examples of %d output frames, the net was built for %d" % (sup["T"], chunk // sub))
                    yield f, iv, sup
            if group and not discard_partial:
                raise ValueError("the last %d examples do not fill a minibatch of %d" % (len(group), B))
        finally:  # also when the consumer stops early: no example handle or open archive is left behind
            for e in group:
                e.close()
            if hasattr(reader, "close"):
                reader.close()

    reused = ReusedSupervision() if reuse else None

    def to_device(f, iv, sup):
        return (torch.from_numpy(f).cuda(), torch.from_numpy(iv).cuda() if iv is not None else None,
                reused.assign(sup) if reuse else hipabi.Supervision(sup))

    if prefetch <= 0:
        for item in host_batches():
            yield to_device(*item)
        return
    import queue
    import threading
    q = queue.Queue(maxsize=prefetch)
    stop = threading.Event()

    def put(item):
        """hand `item` to the consumer unless it has stopped listening (generator closed, exception in to_device)"""
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def worker():
        gen = host_batches()
        try:
            for item in gen:
                if not put(item):
                    return
            put(None)
        except BaseException as e:  # handed to the consumer
            put(e)
        finally:
            gen.close()  # closes the Reader and the examples of an unfinished group (host_batches' own finally)

    th = threading.Thread(target=worker, daemon=True)
    th.start()
    try:
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            yield to_device(*item)
    finally:
        stop.set()
        th.join(timeout=5)


def minibatches_by_width(path, nets, frame_shift=0, reuse=False):
    """An archive with examples of several chunk widths (--egs.chunk-width 150,110,100) and one ChainNet per width
    (ChainNet(cfg, share=primary)): examples are binned by their number of output frames and a minibatch is emitted for a
    width as soon as its bin holds that net's num_sequences examples (nnet3-chain-merge-egs).  Yields (net, feats, ivectors,
    hipabi.Supervision); what is left in the bins at the end of the archive is dropped.
    reuse: one reserved supervision per net (ReusedSupervision), assigned per minibatch as minibatches(reuse=True) does; a yielded
    supervision is valid until the next item is requested."""
    import torch
    reused = {id(n): ReusedSupervision() for n in nets} if reuse else None
    by_frames = {n.cfg.frames_per_chunk // n.cfg.frame_subsampling: n for n in nets}
    bins = {k: [] for k in by_frames}
    for eg in Reader(path):
        T = eg.supervision_info()["frames_per_seq"]
        if T not in by_frames:
            raise ValueError("example %s has %d output frames, nets were given for %s" % (eg.key, T, sorted(by_frames)))
        net, group = by_frames[T], bins[T]
        group.append(eg)
        if len(group) == net.cfg.num_sequences:
            f, iv, sup = merge(group, net.first_t, net.num_t_in, frame_shift, with_ivectors=net.cfg.ivector_dim > 0)
            for e in group:
                e.close()
            bins[T] = []
            yield (net, torch.from_numpy(f).cuda(), torch.from_numpy(iv).cuda() if iv is not None else None,
                   reused[id(net)].assign(sup) if reuse else hipabi.Supervision(sup))


def utterance_chunks(out_frames, frames_per_sequence):
    """Every chunk of frames_per_sequence output frames of utterances of out_frames[u] output frames, as (utterance, begin) in utterance
    order: the begins of infer.chunk_begins; an utterance shorter than a chunk contributes none."""
    from . import infer
    return [(u, o) for u, n in enumerate(out_frames) for o in infer.chunk_begins(n, frames_per_sequence)]


def chunk_minibatches(chunks, num_sequences, seed=0, discard_partial=True):
    """One epoch's minibatches of `chunks`: permuted with numpy.random.default_rng(seed), taken num_sequences at a time; what is left
    over is dropped, or with discard_partial false refused (ValueError).  Host arithmetic: a list of lists of chunks."""
    order = np.random.default_rng(seed).permutation(len(chunks))
    full = len(chunks) - len(chunks) % num_sequences
    if full < len(chunks) and not discard_partial:
        raise ValueError("the last %d chunks do not fill a minibatch of %d" % (len(chunks) - full, num_sequences))
    return [[chunks[i] for i in order[k:k + num_sequences]] for k in range(0, full, num_sequences)]


def _stack_utterances(utterances, feat_dim, ivector_dim, ivector_period):
    """(feats, ivectors or None, frames, ivector_rows) on the device: the utterances' rows stacked as AcousticModel.compute stacks them"""
    import torch
    feats, ivs = [], []
    for f, iv in utterances:
        feats.append(torch.as_tensor(f, dtype=torch.float32).cuda().reshape(-1, feat_dim))
        if ivector_dim > 0:
            iv = torch.as_tensor(iv, dtype=torch.float32).cuda().reshape(-1, ivector_dim)
            ivs.append(iv if ivector_period > 0 else iv[:1])
    return (torch.cat(feats).contiguous(), torch.cat(ivs).contiguous() if ivs else None, [int(f.shape[0]) for f in feats],
            [int(iv.shape[0]) for iv in ivs] if ivs else None)


def minibatches_from_utterances(utterances, alignments, net, unit_set, tolerance, frame_shift=0, ivector_period=10, seed=0, weight=1.0,
                                discard_partial=True):
    """One epoch of training minibatches straight from aligned utterances -- no archive, no host-built array of features.  utterances: the
    list of (feats T_u x feat_dim, ivectors R_u x ivector_dim) that AcousticModel.compute takes (numpy or torch; stacked on the device
    once); alignments[u]: the (units, starts) of utterance u over its O_u = ceil(T_u / fsf) output frames (infer.alignment_from_path);
    unit_set: a hipabi.UnitSet.  The chunks of net.cfg.frames_per_chunk / fsf output frames of every utterance (utterance_chunks) are
    permuted with seed and taken net.cfg.num_sequences at a time (chunk_minibatches).  Yields (feats, ivectors, supervision) as
    minibatches(..., reuse=True) does: the features and i-vectors gathered on the device (hipabi.ChunkInput: include/tdnnf_hip.h, "CHUNK
    INPUTS"; frame_shift and ivector_period as there), the supervision ONE reserved handle compiled on the device by
    assign_alignment_chunks (ReusedSupervision: sized with UnitSet.alignment_chunk_sizes plus headroom, reserved again, larger, when a
    minibatch exceeds it) whose .chunks lists the minibatch's (utterance, begin).  All three are valid until the next item is requested:
    work enqueued on the current stream before that still sees them."""
    import torch
    cfg = net.cfg
    fsf, B = int(cfg.frame_subsampling), int(cfg.num_sequences)
    T = int(cfg.frames_per_chunk) // fsf
    if len(alignments) != len(utterances):
        raise ValueError("%d utterances and %d alignments" % (len(utterances), len(alignments)))
    feats, ivs, frames, iv_rows = _stack_utterances(utterances, int(cfg.feat_dim), int(cfg.ivector_dim), ivector_period)
    out_frames = [(t + fsf - 1) // fsf for t in frames]
    batches = chunk_minibatches(utterance_chunks(out_frames, T), B, seed, discard_partial)
    if not batches:
        return
    gatherer, reused = hipabi.ChunkInput(B), ReusedSupervision()
    out = (torch.empty(net.num_t_in * B, feats.shape[1], dtype=torch.float32, device=feats.device),
           torch.empty(B, ivs.shape[1], dtype=torch.float32, device=feats.device) if ivs is not None else None)
    for chunks in batches:
        utt, begins = [u for u, _ in chunks], [o for _, o in chunks]
        f, iv = gatherer.gather(net, T, utt, begins, frames, feats, iv_rows, ivs, ivector_period, frame_shift, out=out)
        sup = reused.assign_alignment_chunks(unit_set, [alignments[u] for u in utt], [out_frames[u] for u in utt], begins, T, tolerance, weight)
        sup.chunks = list(chunks)
        yield f, iv, sup


def minibatches_from_store(store, ivectors, alignments, net, unit_set, tolerance, frame_shift=0, ivector_period=10, seed=0, weight=1.0, discard_partial=True):
    """minibatches_from_utterances with the features taken from a hipabi.FeatureStore (include/tdnnf_hip.h, "FEATURE STORES"): the
    utterances are the store's, in append order, their features decoded inside the gather (ChunkInput.gather_stored) -- no float copy of
    them exists.  ivectors[u]: the i-vector rows R_u x ivector_dim of utterance u (numpy or torch; stacked on the device once, float), not
    read by a net without i-vectors; alignments[u] as there.  The same chunk order for a seed, the same reserved supervision and the same
    validity rule: what it yields is, minibatch for minibatch, what minibatches_from_utterances yields for store.expand's features."""
    import torch
    cfg = net.cfg
    fsf, B = int(cfg.frame_subsampling), int(cfg.num_sequences)
    T = int(cfg.frames_per_chunk) // fsf
    frames = list(store.frames)
    if len(alignments) != len(frames):
        raise ValueError("%d utterances and %d alignments" % (len(frames), len(alignments)))
    if store.feat_dim != int(cfg.feat_dim):
        raise ValueError("a store of feat_dim %d for a net of feat_dim %d" % (store.feat_dim, int(cfg.feat_dim)))
    ivs = iv_rows = None
    if cfg.ivector_dim > 0:
        if len(ivectors) != len(frames):
            raise ValueError("%d utterances and %d i-vector matrices" % (len(frames), len(ivectors)))
        rows = [torch.as_tensor(iv, dtype=torch.float32).cuda().reshape(-1, int(cfg.ivector_dim)) for iv in ivectors]
        rows = [iv if ivector_period > 0 else iv[:1] for iv in rows]
        ivs, iv_rows = torch.cat(rows).contiguous(), [int(iv.shape[0]) for iv in rows]
    out_frames = [(t + fsf - 1) // fsf for t in frames]
    batches = chunk_minibatches(utterance_chunks(out_frames, T), B, seed, discard_partial)
    if not batches:
        return
    gatherer, reused = hipabi.ChunkInput(B), ReusedSupervision()
    out = (torch.empty(net.num_t_in * B, store.feat_dim, dtype=torch.float32, device="cuda"),
           torch.empty(B, ivs.shape[1], dtype=torch.float32, device="cuda") if ivs is not None else None)
    for chunks in batches:
        utt, begins = [u for u, _ in chunks], [o for _, o in chunks]
        f, iv = gatherer.gather_stored(net, T, utt, begins, store, iv_rows, ivs, ivector_period, frame_shift, out=out)
        sup = reused.assign_alignment_chunks(unit_set, [alignments[u] for u in utt], [out_frames[u] for u in utt], begins, T, tolerance, weight)
        sup.chunks = list(chunks)
        yield f, iv, sup


_MATRIX_TOKENS = {b"CM": 1, b"CM2": 2, b"CM3": 3}


def read_feature_archive(path):
    """Iterates over a Kaldi binary archive of matrices (what copy-feats writes to ark:path; per entry `key ' ' \\0B` then a GeneralMatrix)
    and yields (key, item).  A CompressedMatrix (token CM, CM2 or CM3) comes as the item dict hipabi.FeatureStore.append takes, its codes
    UNTOUCHED, in Kaldi's order: {"format": 1 | 2 | 3, "min", "range" (numpy float32), "rows", "cols", "codes": uint8 [cols, rows]
    (format 1, column-major), uint16 [rows, cols] (2) or uint8 [rows, cols] (3), and for format 1 "percentiles": uint16 [cols, 4]}.  A full
    matrix (FM, DM) comes as a float32 array.  Host only."""
    with open(path, "rb") as f:
        data = f.read()
    at = 0

    def take(n, what):
        nonlocal at
        if at + n > len(data):
            raise ValueError("%s: unexpected end of file in %s" % (path, what))
        at += n
        return data[at - n:at]

    def token():
        end = data.find(b" ", at)
        if end < 0:
            raise ValueError("%s: unexpected end of file in a token" % path)
        return take(end + 1 - at, "a token")[:-1]

    def i32():
        if take(1, "an integer") != b"\x04":
            raise ValueError("%s: expected a 4-byte integer" % path)
        return int(np.frombuffer(take(4, "an integer"), "<i4")[0])

    while at < len(data):
        key = token().decode()
        if take(2, "the binary mark") != b"\0B":
            raise ValueError("%s: entry %s is not in binary mode" % (path, key))
        tok = token()
        if tok in _MATRIX_TOKENS:
            fmt = _MATRIX_TOKENS[tok]
            mn, rg = np.frombuffer(take(8, "a matrix header"), "<f4")
            rows, cols = (int(x) for x in np.frombuffer(take(8, "a matrix header"), "<i4"))
            if rows < 0 or cols < 0:
                raise ValueError("%s: entry %s has a compressed matrix of %d x %d" % (path, key, rows, cols))
            item = dict(format=fmt, min=np.float32(mn), range=np.float32(rg), rows=rows, cols=cols)
            if fmt == 1:
                item["percentiles"] = np.frombuffer(take(8 * cols, "the percentiles"), "<u2").reshape(cols, 4).copy()
                item["codes"] = np.frombuffer(take(rows * cols, "the codes"), np.uint8).reshape(cols, rows).copy()
            elif fmt == 2:
                item["codes"] = np.frombuffer(take(2 * rows * cols, "the codes"), "<u2").reshape(rows, cols).copy()
            else:
                item["codes"] = np.frombuffer(take(rows * cols, "the codes"), np.uint8).reshape(rows, cols).copy()
            yield key, item
        elif tok in (b"FM", b"DM"):
            rows, cols = i32(), i32()
            if rows < 0 or cols < 0:
                raise ValueError("%s: entry %s has a matrix of %d x %d" % (path, key, rows, cols))
            width, kind = (4, "<f4") if tok == b"FM" else (8, "<f8")
            yield key, np.frombuffer(take(width * rows * cols, "a matrix"), kind).reshape(rows, cols).astype(np.float32)
        else:
            raise ValueError("%s: entry %s holds %r, not a matrix (FM, DM, CM, CM2, CM3)" % (path, key, tok))


def write_feature_archive(path, items):
    """The inverse for compressed items: (key, item dict as read_feature_archive yields it) back into Kaldi's bytes -- reading an archive
    of compressed matrices and writing it gives the file again.  Float matrices go through infer.write_matrix_archive."""
    tokens = {v: k for k, v in _MATRIX_TOKENS.items()}
    with open(path, "wb") as f:
        for key, item in items:
            fmt, rows, cols = int(item["format"]), int(item["rows"]), int(item["cols"])
            if fmt not in tokens or not key or " " in key:
                raise ValueError("%s: entry %r of format %r: a key without spaces and format 1, 2 or 3 are needed" % (path, key, fmt))
            codes = np.ascontiguousarray(item["codes"], dtype="<u2" if fmt == 2 else np.uint8)
            if rows < 0 or cols < 0 or codes.size != rows * cols:
                raise ValueError("%s: entry %s is %d x %d with %d codes" % (path, key, rows, cols, codes.size))
            f.write(key.encode() + b" \0B" + tokens[fmt] + b" ")
            f.write(np.asarray([item["min"], item["range"]], "<f4").tobytes() + np.asarray([rows, cols], "<i4").tobytes())
            if fmt == 1:
                pct = np.ascontiguousarray(item["percentiles"], dtype="<u2")
                if pct.size != 4 * cols:
                    raise ValueError("%s: entry %s has %d columns and %d percentiles" % (path, key, cols, pct.size))
                f.write(pct.tobytes())
            f.write(codes.tobytes())


def write_chunk_egs(path, utterances, alignments, net, unit_set, tolerance, chunks, margin=None, compress=False, ivector_period=10, weight=1.0):
    """The host route to the same chunks: one single-sequence example per (utterance, begin) of `chunks` into the archive `path` (Writer),
    for Kaldi's tools or for minibatches(path, net, frame_shift=s).  utterances, alignments as minibatches_from_utterances takes them, on
    the host; unit_set: the unit set DICT (synth.make_unit_set), since the supervision is the host lattice
    synth.supervision_lattice_from_alignment_chunks through sequence_of.  An example's input rows cover the times
    net.first_t - margin .. net.first_t + net.num_t_in - 1 + margin relative to begin * fsf, clamped to the utterance (nnet3's edge
    padding); margin defaults to fsf - 1, so that every legal frame shift can be merged.  Its i-vector is the row of "CHUNK INPUTS".
    Keys are utt<u>-<begin>.  Returns the number of examples written."""
    from . import synth
    cfg = net.cfg
    fsf = int(cfg.frame_subsampling)
    T = int(cfg.frames_per_chunk) // fsf
    margin = fsf - 1 if margin is None else int(margin)
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    with Writer(path) as w:
        for u, o in chunks:
            f = host(utterances[u][0]).astype(np.float32, copy=False).reshape(-1, int(cfg.feat_dim))
            out_frames = (len(f) + fsf - 1) // fsf
            times = np.clip(o * fsf + np.arange(net.first_t - margin, net.first_t + net.num_t_in + margin), 0, len(f) - 1)
            iv = None
            if cfg.ivector_dim > 0:
                rows = host(utterances[u][1]).astype(np.float32, copy=False).reshape(-1, int(cfg.ivector_dim))
                iv = rows[min(((o + T // 2) * fsf) // ivector_period, len(rows) - 1) if ivector_period > 0 else 0]
            sup = synth.supervision_lattice_from_alignment_chunks(unit_set, [alignments[u]], [out_frames], [o], T, tolerance, weight=weight)
            w.write("utt%d-%d" % (u, o), f[times], net.first_t - margin, sequence_of(sup, 0), int(cfg.num_pdfs), ivector=iv, compress=compress, t_step=fsf)
    return len(chunks)
