"""The model's output for decoding (include/tdnnf_hip.h, "inference"): plumbing around tdnnf_infer_* and tdnnf_online_*.

AcousticModel computes, for whole utterances of any length, what nnet3's DecodableNnetSimple hands to
latgen-faster-mapped (steps/nnet3/decode.sh --acwt 1.0, run_tdnn_fbk_40_iv_sp_7q.sh:254-258); write_matrix_archive
stores it as a Kaldi binary float-matrix archive.  OnlineAcousticModel computes the same rows for streams whose frames arrive a
few at a time (nnet3's looped decodable).  Every computation is a call into the HIP library.
"""
import ctypes as C
import struct

import numpy as np

from . import hipabi, trainer

OUTPUTS = {"output": 0, "output-xent": 1}
ARITHMETICS = {"f32": 0, "f16x3": 3}  # name -> gemm_precision of tdnnf_infer_create_arith


def arithmetic_precision(name):
    """gemm_precision of an arithmetic name; ValueError for any other (no library call)."""
    if not isinstance(name, str) or name not in ARITHMETICS:
        raise ValueError("arithmetic must be one of %s, not %r" % (sorted(ARITHMETICS), name))
    return ARITHMETICS[name]


class AcousticModel:
    """Forward-only view of a ChainNet's model: reads its parameters and BatchNorm statistics at every compute.
    arithmetic "f32" (default): exact f32 GEMMs; "f16x3": every GEMM on the 16-bit matrix cores from operands split into two
    scaled f16 planes (three products, f32 accumulation), whatever arithmetic the model was trained in."""

    def __init__(self, net, frames_per_chunk=150, max_chunks=256, output="output", arithmetic="f32"):
        precision = arithmetic_precision(arithmetic)
        self.arithmetic = arithmetic
        self.lib = hipabi.load()
        self.net = net  # keeps the model alive
        self.frames_per_chunk, self.max_chunks, self.output = int(frames_per_chunk), int(max_chunks), output
        self.fsf = int(net.cfg.frame_subsampling)
        self.num_pdfs = int(net.cfg.num_pdfs)
        self.h = C.c_void_p()
        if precision == 0:
            hipabi.check(self.lib.tdnnf_infer_create(net.h, self.frames_per_chunk, self.max_chunks, OUTPUTS[output], C.byref(self.h)))
        else:
            hipabi.check(self.lib.tdnnf_infer_create_arith(net.h, self.frames_per_chunk, self.max_chunks, OUTPUTS[output], precision,
                                                           C.byref(self.h)))

    @classmethod
    def from_model_file(cls, path, frames_per_chunk=150, max_chunks=256, output="output", arithmetic="f32"):
        """A model read from an nnet3 raw model file (tdnnf_net_config_from_model + tdnnf_net_read_model)."""
        arithmetic_precision(arithmetic)
        cfg = trainer.config_from_model(path, frames_per_chunk=frames_per_chunk, num_sequences=1)
        cfg.cv_update = 1  # (no dropout masks; the statistics are only read)
        net = trainer.ChainNet(cfg)
        net.read_model(path)
        return cls(net, frames_per_chunk, max_chunks, output, arithmetic)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tdnnf_infer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self, frames, ivector_rows=None, ivector_period=10):
        """The chunk plan (host only): int array (num_chunks, 4) of (utterance, first input frame, i-vector row, valid rows)."""
        fr, frp = hipabi.iarr(frames)
        ivr, ivp = hipabi.iarr(ivector_rows if ivector_rows is not None else np.ones(len(fr), np.int32))
        n = C.c_int()
        self.lib.tdnnf_infer_plan(self.h, len(fr), frp, ivp, int(ivector_period), None, 0, C.byref(n))
        out = np.zeros((max(n.value, 1), 4), np.int32)
        hipabi.check(self.lib.tdnnf_infer_plan(self.h, len(fr), frp, ivp, int(ivector_period),
                                               out.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
        return out[:n.value]

    def compute(self, utterances, ivector_period=10):
        """utterances: list of (feats T_u x feat_dim, ivectors R_u x ivector_dim) (numpy or torch).  ivector_period <= 0: one
        i-vector per utterance (its first row).  Returns a list of torch CUDA tensors, O_u = ceil(T_u / fsf) x num_pdfs."""
        import torch
        out, outs = self._compute_stacked(utterances, ivector_period)
        return list(torch.split(out, outs)) if outs else []

    def _compute_stacked(self, utterances, ivector_period):
        """compute's work: (the outputs of all utterances stacked in one matrix, rows per utterance)"""
        import torch
        feats, ivs, frames, ivrows = [], [], [], []
        for f, iv in utterances:
            f = torch.as_tensor(f, dtype=torch.float32).cuda()
            iv = torch.as_tensor(iv, dtype=torch.float32).cuda().reshape(-1, self.net.cfg.ivector_dim)
            if ivector_period <= 0:
                iv = iv[:1]
            feats.append(f)
            ivs.append(iv)
            frames.append(f.shape[0])
            ivrows.append(iv.shape[0])
        F = torch.cat(feats).contiguous() if feats else torch.zeros(0, self.net.cfg.feat_dim, device="cuda")
        IV = torch.cat(ivs).contiguous() if ivs else torch.zeros(0, self.net.cfg.ivector_dim, device="cuda")
        outs = [(t + self.fsf - 1) // self.fsf for t in frames]
        out = torch.zeros(sum(outs), self.num_pdfs, dtype=torch.float32, device="cuda")
        fr, frp = hipabi.iarr(frames)
        ivr, ivp = hipabi.iarr(ivrows)
        hipabi.check(self.lib.tdnnf_infer_compute(self.h, len(frames), frp, hipabi.pmat(F), ivp, hipabi.pmat(IV), int(ivector_period),
                                                  hipabi.pmat(out), hipabi.stream()))
        return out, outs

    def align(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, ivector_period=10, checkpoint=None):
        """compute, then the best path of every utterance through its graph (align below); the output stays on the device in between."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _align_stacked(out, outs, graphs, utt_graph, acoustic_scale, checkpoint=checkpoint) if outs else []

    def posteriors(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, ivector_period=10, checkpoint=None):
        """compute, then forward-backward of every utterance through its graph (posteriors below): [(post [O_u, num_pdfs] CUDA tensor,
        logprob, ok)]; the output stays on the device in between."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _posteriors_stacked(out, outs, graphs, utt_graph, acoustic_scale, weight, checkpoint=checkpoint) if outs else []

    def posteriors_compact(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, ivector_period=10, checkpoint=None):
        """compute, then forward-backward of every utterance through its graph in the compact form (posteriors_compact below):
        [(pdf_ids [D] int32, post [O_u, D] CUDA tensor, logprob, ok)]; the output stays on the device in between."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _posteriors_compact_stacked(out, outs, graphs, utt_graph, acoustic_scale, weight, checkpoint=checkpoint) if outs else []

    def posteriors_sparse(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, min_post=0.01, max_per_frame=16,
                          ivector_period=10, checkpoint=None):
        """compute, then forward-backward of every utterance through its graph in the sparse form (posteriors_sparse below):
        [(pdf [O_u, K] int32, post [O_u, K], count [O_u] int32 CUDA tensors, logprob, ok, truncated_frames)]; the output stays on the
        device in between."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _posteriors_sparse_stacked(out, outs, graphs, utt_graph, acoustic_scale, weight, min_post, max_per_frame, checkpoint=checkpoint) if outs else []

    def align_labels(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, ivector_period=10, checkpoint=None):
        """compute, then the labelled best path of every utterance through its graph (align_labels below)."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _align_stacked(out, outs, graphs, utt_graph, acoustic_scale, labels=True, checkpoint=checkpoint) if outs else []

    def label_posteriors_compact(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, ivector_period=10, checkpoint=None):
        """compute, then the compact posteriors per label (label_posteriors_compact below): [(labels [L] int32, post [O_u, L] CUDA tensor,
        logprob, ok)]."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _posteriors_compact_stacked(out, outs, graphs, utt_graph, acoustic_scale, weight, labels=True, checkpoint=checkpoint) if outs else []

    def label_posteriors_sparse(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, min_post=0.01, max_per_frame=16,
                                ivector_period=10, checkpoint=None):
        """compute, then the sparse posteriors per label (label_posteriors_sparse below): [(label [O_u, K] int32, post [O_u, K], count [O_u]
        int32 CUDA tensors, logprob, ok, truncated_frames)]."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _posteriors_sparse_stacked(out, outs, graphs, utt_graph, acoustic_scale, weight, min_post, max_per_frame, labels=True, checkpoint=checkpoint) if outs else []

    def logprob(self, utterances, graphs, utt_graph=None, acoustic_scale=1.0, ivector_period=10):
        """compute, then the total log-likelihood of every utterance through its graph (logprob below): [(logprob, ok)]."""
        out, outs = self._compute_stacked(utterances, ivector_period)
        return _logprob_stacked(out, outs, graphs, utt_graph, acoustic_scale) if outs else []

    def counts(self):
        """(fused_layers, fallback_passes) of the last compute."""
        a, b = C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_infer_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def gemm_counts(self):
        """(plane_gemms, f32_gemms) of the last compute: GEMM launches that ran from f16 planes / on the f32 kernels."""
        a, b = C.c_longlong(), C.c_longlong()
        hipabi.check(self.lib.tdnnf_infer_gemm_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def online_schedule(frames_per_step, frame_subsampling, left, right, frames):
    """The steps of one streamed utterance (tdnnf_online_schedule, host only): int array (num_steps, 5) of (clock, first passed
    frame, passed rows, first output row, kept output rows)."""
    lib = hipabi.load()
    n = C.c_int()
    lib.tdnnf_online_schedule(int(frames_per_step), int(frame_subsampling), int(left), int(right), int(frames), None, 0, C.byref(n))
    out = np.zeros((max(n.value, 1), 5), np.int32)
    hipabi.check(lib.tdnnf_online_schedule(int(frames_per_step), int(frame_subsampling), int(left), int(right), int(frames),
                                           out.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
    return out[:n.value]


class OnlineAcousticModel:
    """Streaming view of a ChainNet's model (include/tdnnf_hip.h, "inference (forward only, streaming)"): num_slots concurrent
    streams, each fed a few frames at a time; a step advances every stream that has a window ready by frames_per_step input
    frames and returns its new output rows.  Plumbing only: queues of device tensors and the calls into tdnnf_online_*."""

    def __init__(self, net, frames_per_step=30, num_slots=16, output="output"):
        self.lib = hipabi.load()
        self.net = net  # keeps the model alive
        self.frames_per_step, self.num_slots, self.output = int(frames_per_step), int(num_slots), output
        self.fsf = int(net.cfg.frame_subsampling)
        self.num_pdfs = int(net.cfg.num_pdfs)
        self.h = C.c_void_p()
        hipabi.check(self.lib.tdnnf_online_create(net.h, self.frames_per_step, self.num_slots, OUTPUTS[output], C.byref(self.h)))
        left, right, lat = C.c_int(), C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_online_context(self.h, C.byref(left), C.byref(right), C.byref(lat)))
        self.left, self.right, self.latency = left.value, right.value, lat.value
        self.free = list(range(self.num_slots))
        self.streams = {}  # slot -> dict(buf: unconsumed frames (device), base: frame index of buf[0], total: frames pushed, final, last, iv)

    @classmethod
    def from_model_file(cls, path, frames_per_step=30, num_slots=16, output="output"):
        """A model read from an nnet3 raw model file (tdnnf_net_config_from_model + tdnnf_net_read_model)."""
        cfg = trainer.config_from_model(path, frames_per_chunk=frames_per_step, num_sequences=1)
        cfg.cv_update = 1  # (no dropout masks; the statistics are only read)
        net = trainer.ChainNet(cfg)
        net.read_model(path)
        return cls(net, frames_per_step, num_slots, output)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tdnnf_online_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def context(self):
        """(left, right, latency) in input frames (tdnnf_online_context)."""
        return self.left, self.right, self.latency

    def slot_state(self, slot):
        """(clock, T) of a slot; T = -1 until its last frame has been stepped."""
        a, b = C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_online_slot(self.h, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    def open(self):
        """Starts a new utterance in a free slot (tdnnf_online_reset) and returns the slot."""
        if not self.free:
            raise RuntimeError("OnlineAcousticModel: all %d slots are in use" % self.num_slots)
        slot = self.free.pop(0)
        hipabi.check(self.lib.tdnnf_online_reset(self.h, slot, hipabi.stream()))
        self.streams[slot] = dict(buf=None, base=0, total=0, final=False, last=None, iv=None)
        return slot

    def push(self, slot, feats, ivector, final=False):
        """Queues the stream's next frames (n x feat_dim, numpy or torch; n may be 0) on the device; `ivector` is the stream's
        i-vector from the next step on.  final: these are the utterance's last frames -- it must come with at least one frame
        that no step has consumed yet (the window in which an utterance ends is marked when it is stepped)."""
        import torch
        st = self.streams[slot]
        if st["final"]:
            raise ValueError("push: slot %d has had its final frames" % slot)
        f = torch.as_tensor(feats, dtype=torch.float32).cuda().reshape(-1, self.net.cfg.feat_dim)
        st["buf"] = f if st["buf"] is None else torch.cat([st["buf"], f])
        st["total"] += f.shape[0]
        st["iv"] = torch.as_tensor(ivector, dtype=torch.float32).cuda().reshape(1, self.net.cfg.ivector_dim)
        if final:
            clock = self.slot_state(slot)[0]
            if st["total"] == 0 or st["total"] <= clock:
                raise ValueError("push: final must come with a frame that has not been stepped yet")
            st["final"] = True

    def finished(self, slot):
        """True once every output row of the slot's utterance has been returned."""
        clock, T = self.slot_state(slot)
        return T >= 0 and clock - self.latency >= T

    def release(self, slot):
        del self.streams[slot]
        self.free.append(slot)

    def _window(self, slot):
        """(rows to pass, final) of the slot's next window, or None while it has to wait for frames."""
        st = self.streams[slot]
        F = self.frames_per_step
        clock, T = self.slot_state(slot)
        if st["total"] == 0 or self.finished(slot):
            return None
        if T >= 0:  # flush
            return st["last"], True
        if clock < 0:  # warm-up
            return st["buf"][:1], False
        have = st["total"] - clock
        if st["final"]:
            n = min(F, have)
        elif have >= F:
            n = F
        else:
            return None
        lo = clock - st["base"]
        rows = st["buf"][lo:lo + n]
        return rows, st["final"] and have <= F

    def step(self, slots=None):
        """One tdnnf_online_step over every open slot (or those of `slots`, in that order) that has a full window or is
        finishing -- warm-up and flush windows included.  Returns {slot: new output rows (torch CUDA, k x num_pdfs, k >= 0)}."""
        import torch
        order = list(self.streams) if slots is None else list(slots)
        act, feats, ivs, rows, fins = [], [], [], [], []
        for slot in order:
            w = self._window(slot)
            if w is None:
                continue
            act.append(slot)
            feats.append(w[0])
            rows.append(w[0].shape[0])
            fins.append(int(w[1]))
            ivs.append(self.streams[slot]["iv"])
        if not act:
            return {}
        first, count, out = self.step_raw(act, rows, fins, torch.cat(feats).contiguous(), torch.cat(ivs).contiguous())
        Tout = self.frames_per_step // self.fsf
        res = {}
        for i, slot in enumerate(act):
            st = self.streams[slot]
            clock = self.slot_state(slot)[0]  # (already advanced)
            if clock > 0 and st["buf"].shape[0]:  # frames before the clock are consumed: keep the last of them for the flush windows
                used = min(clock, st["total"]) - st["base"]
                if used > 0:
                    st["last"] = st["buf"][used - 1:used]
                    st["buf"] = st["buf"][used:]
                    st["base"] += used
            res[slot] = out[i * Tout:i * Tout + count[i]]
        return res

    def step_raw(self, slots, rows, finals, feats, ivectors):
        """tdnnf_online_step as it is: the active slots, their passed row counts and final flags, the passed rows stacked and one
        i-vector row per slot.  Returns (first output index per slot, kept rows per slot, out of len(slots) * F / fsf rows)."""
        import torch
        B = len(slots)
        out = torch.zeros(B * (self.frames_per_step // self.fsf), self.num_pdfs, dtype=torch.float32, device="cuda")
        sl, slp = hipabi.iarr(slots)
        rw, rwp = hipabi.iarr(rows)
        fn, fnp = hipabi.iarr(finals)
        first, firstp = hipabi.iarr(np.zeros(max(B, 1), np.int32))
        count, countp = hipabi.iarr(np.zeros(max(B, 1), np.int32))
        hipabi.check(self.lib.tdnnf_online_step(self.h, B, slp, rwp, fnp, hipabi.pmat(feats), hipabi.pmat(ivectors), hipabi.pmat(out),
                                                firstp, countp, hipabi.stream()))
        return first[:B], count[:B], out

    def counts(self):
        """(gemm_rows, carried_rows, fused, fallback) of the last step (tdnnf_online_counts)."""
        a, b, c, d = C.c_longlong(), C.c_longlong(), C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_online_counts(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value


def write_matrix_archive(path, items):
    """Kaldi binary archive of float matrices: per item `key ' ' \\0B FM ' ' \\4 rows \\4 cols` then row-major float32
    (the encodings include/tdnnf_kaldi_io.h restates); what latgen-faster-mapped or copy-matrix read with ark:path.
    items: iterable of (key, matrix) with numpy or torch matrices."""
    with open(path, "wb") as f:
        for key, m in items:
            if hasattr(m, "detach"):
                m = m.detach().cpu().numpy()
            m = np.ascontiguousarray(m, dtype="<f4")
            assert m.ndim == 2 and " " not in key and key
            f.write(key.encode() + b" \0BFM ")
            f.write(struct.pack("<bibi", 4, m.shape[0], 4, m.shape[1]))
            f.write(m.tobytes())


def align(outputs, graphs, utt_graph=None, acoustic_scale=1.0, checkpoint=None):
    """Best-path alignment (include/tdnnf_hip.h, "best-path alignment") of the model's outputs, a list of O_u x num_pdfs CUDA tensors as
    AcousticModel.compute returns them, through `graphs` (hipabi.AlignGraphs): utterance u takes graph utt_graph[u] -- None: the one
    graph there is, or graph u.  Returns a list of (pdf-ids as torch int32 CUDA tensor, score, ok); an utterance without an accepting
    path of its length has score -inf, ok False and pdf-ids of -1.  What ali-to-pdf would print; no beam, no lattice.  checkpoint (here,
    on align_labels and on the AcousticModel methods): AlignGraphs.best_path's keyword -- None leaves option align_path_checkpoint as it
    stands, an int sets it for the call (back-pointers of C frames at a time, -1 automatic: a workspace of O(sqrt(frames)) vectors for
    whole recordings, the same path)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _align_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, checkpoint=checkpoint)


def align_labels(outputs, graphs, utt_graph=None, acoustic_scale=1.0, checkpoint=None):
    """align with the identity of the path's arcs, through labelled graphs (hipabi.AlignGraphs of graph dicts with "label": a transition-id,
    a phone, a word position per arc).  Returns a list of (pdf-ids, labels, arcs, score, ok): three torch int32 CUDA tensors of O_u
    elements -- per frame the pdf, the label and the index (in the utterance's graph dict) of the arc taken -- all -1 without an accepting
    path.  With transition-ids as labels `labels` is what nnet3-align-compiled writes (write_int_vector_archive), with phones what
    ali-to-phones --per-frame prints."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _align_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, labels=True, checkpoint=checkpoint)


def _align_stacked(y, frames, graphs, utt_graph, acoustic_scale, labels=False, checkpoint=None):
    """align on the utterances' rows stacked in one matrix (what tdnnf_infer_compute writes): row_stride 1"""
    import torch
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    if labels:
        pdfs, _, results, lab, arcs = graphs.best_path_labels(y, frames, rows, 1, utt_graph, acoustic_scale, checkpoint=checkpoint)
        res = results.cpu().numpy()  # (waits for the stream)
        return [(p, l, a, float(res[u, 0]), bool(res[u, 1] == 1.0))
                for u, (p, l, a) in enumerate(zip(torch.split(pdfs, frames), torch.split(lab, frames), torch.split(arcs, frames)))]
    pdfs, _, results = graphs.best_path(y, frames, rows, 1, utt_graph, acoustic_scale, checkpoint=checkpoint)
    res = results.cpu().numpy()  # (waits for the stream)
    return [(p, float(res[u, 0]), bool(res[u, 1] == 1.0)) for u, p in enumerate(torch.split(pdfs, frames))]


def alignment_from_path(slots_per_frame, transcript):
    """The segmentation of one utterance from its labelled best path, for Supervision.assign_alignments: slots_per_frame, one int per
    frame, is the label output of align_labels / AlignGraphs.best_path_labels through a handle whose graphs were compiled from transcripts
    (AlignGraphs.assign_transcripts: an arc's label is the slot it enters, so a frame's label is the slot it was spent in); transcript the
    utterance's (units, optional) pair.  Returns (units, starts), int32 arrays with one entry per run of equal labels: the slot's unit and
    the run's first frame -- an optional slot the path skipped has no run and is dropped.  Pure numpy; ValueError for a path that is not
    one (no frames, a -1 of an utterance without an accepting path, slots that do not increase or lie outside the transcript)."""
    slots = np.asarray(slots_per_frame.detach().cpu().numpy() if hasattr(slots_per_frame, "detach") else slots_per_frame, dtype=np.int64).reshape(-1)
    units = np.asarray(transcript[0], dtype=np.int64).reshape(-1)
    if len(slots) == 0:
        raise ValueError("alignment_from_path: no frames")
    starts = np.concatenate([[0], 1 + np.flatnonzero(slots[1:] != slots[:-1])])
    runs = slots[starts]
    if runs.min() < 0 or runs.max() >= len(units) or np.any(runs[1:] <= runs[:-1]):
        raise ValueError(f"alignment_from_path: the slots of the runs, {runs.tolist()}, are not an increasing walk through {len(units)} slots")
    return units[runs].astype(np.int32), starts.astype(np.int32)


def chunk_begins(utt_frames, T):
    """The first frames of the chunks of T output frames that cover an utterance of utt_frames, for Supervision.assign_alignment_chunks:
    none for an utterance shorter than T; else n = ceil(utt_frames / T) chunks spread evenly, round(i * (utt_frames - T) / (n - 1)) --
    the first at 0, the last ending with the utterance, neighbours overlapping where T does not divide utt_frames -- or [0] for n = 1."""
    utt_frames, T = int(utt_frames), int(T)
    if T < 1:
        raise ValueError(f"chunk_begins: chunks of {T} frames")
    if utt_frames < T:
        return []
    n = -(-utt_frames // T)
    return [0] if n == 1 else [int(round(i * (utt_frames - T) / (n - 1))) for i in range(n)]


def alignment_from_pronunciation_path(entries_per_frame, transcript):
    """alignment_from_path for a transcript with pronunciation alternatives: entries_per_frame, one int per frame, is the label output of
    AlignGraphs.best_path_labels through a handle assigned with assign_pronunciations (an arc's label is the entry it enters, the entries
    numbered in flat order: position, alternative, unit); transcript the utterance's (positions, optional[, alt_logprob]).  Returns (units,
    starts, chosen): int32 arrays with one entry per run of equal labels -- the entry's unit and the run's first frame, ready for
    Supervision.assign_alignments -- and chosen[p], the alternative the path took at position p, -1 for a skipped optional position.
    Pure numpy; ValueError for a path that is not one: no frames, a -1 of an utterance without an accepting path, an entry outside the
    transcript, an alternative entered elsewhere than at its first unit or left before its last, positions that do not increase or that
    skip a mandatory one."""
    entries = np.asarray(entries_per_frame.detach().cpu().numpy() if hasattr(entries_per_frame, "detach") else entries_per_frame, dtype=np.int64).reshape(-1)
    positions, optional = transcript[0], transcript[1]
    of_entry = [(p, a, j, int(u), len(alt)) for p, pos in enumerate(positions) for a, alt in enumerate(pos) for j, u in enumerate(alt)]
    if len(entries) == 0:
        raise ValueError("alignment_from_pronunciation_path: no frames")
    starts = np.concatenate([[0], 1 + np.flatnonzero(entries[1:] != entries[:-1])])
    runs = entries[starts]
    if runs.min() < 0 or runs.max() >= len(of_entry):
        raise ValueError(f"alignment_from_pronunciation_path: the entries of the runs, {runs.tolist()}, are not all among the transcript's {len(of_entry)}")
    chosen = np.full(len(positions), -1, np.int32)
    before = None  # the entry of the run before
    for e in runs:
        p, a, j, _, _ = of_entry[e]
        inside = before is not None and before[:2] == (p, a) and before[2] + 1 == j
        enters = j == 0 and (before is None or (before[2] + 1 == before[4] and before[0] < p))
        if not (inside or enters):
            raise ValueError(f"alignment_from_pronunciation_path: the entries of the runs, {runs.tolist()}, are not a walk through the transcript "
                             f"(at entry {int(e)}: position {p}, alternative {a}, unit {j})")
        chosen[p] = a
        before = of_entry[e]
    if before[2] + 1 != before[4] or any(chosen[p] < 0 and not optional[p] for p in range(len(positions))):
        raise ValueError(f"alignment_from_pronunciation_path: the path ends inside an alternative or skips a mandatory position (chosen {chosen.tolist()})")
    return np.asarray([of_entry[e][3] for e in runs], np.int32), starts.astype(np.int32), chosen


def write_int_vector_archive(path, items):
    """Kaldi binary archive of vector<int32>: per item `key ' ' \\0B \\4 n` then n little-endian int32 (WriteIntegerVector; the intvec
    encoding of include/tdnnf_kaldi_io.h, what the egs reader takes for <AlignmentPdfs>); what ali-to-pdf writes and copy-int-vector
    reads with ark:path.  items: iterable of (key, ints) with sequences, numpy arrays or torch tensors."""
    with open(path, "wb") as f:
        for key, v in items:
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            v = np.ascontiguousarray(v, dtype="<i4").reshape(-1)
            assert " " not in key and key
            f.write(key.encode() + b" \0B")
            f.write(struct.pack("<bi", 4, v.shape[0]))
            f.write(v.tobytes())


def posteriors(outputs, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, checkpoint=None):
    """Forward-backward (include/tdnnf_hip.h, "forward-backward") of the model's outputs, a list of O_u x num_pdfs CUDA tensors as
    AcousticModel.compute returns them, through `graphs` (hipabi.AlignGraphs; utt_graph as for align).  Returns a list of (post float32
    [O_u, num_pdfs] CUDA tensor = weight x the per-frame pdf posteriors, logprob, ok): logprob is the log-sum over all paths of the
    utterance's length; without a finite one ok is False and post all zeros.  Soft alignments and the flat-start numerator's derivative;
    no beam, pdf level.  checkpoint (here and on the other posterior functions and AcousticModel methods): AlignGraphs' keyword -- None
    leaves option align_checkpoint as it stands, an int sets it for the call (alpha of every C-th frame only, -1 automatic: a workspace
    of O(sqrt(frames)) vectors, the same bits)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _posteriors_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, weight, checkpoint=checkpoint)


def posteriors_compact(outputs, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, checkpoint=None):
    """posteriors in the compact form (include/tdnnf_hip.h, "compact posteriors"): only the columns an utterance's graph can fill.  Returns a
    list of (pdf_ids numpy int32 [D] = graphs.pdfs(the utterance's graph), ascending; post float32 [O_u, D] CUDA tensor, a view of the
    call's one output, with post[t, k] = what posteriors gives for [t, pdf_ids[k]], bit for bit; logprob; ok).  Every pdf outside pdf_ids
    has posterior 0.  What write_posterior_archive takes as (key, pdf_ids, post)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _posteriors_compact_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, weight, checkpoint=checkpoint)


def posteriors_sparse(outputs, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, min_post=0.01, max_per_frame=16, checkpoint=None):
    """posteriors in the sparse form (include/tdnnf_hip.h, "sparse posteriors"): per frame the at most K = max_per_frame pairs whose value
    -- what posteriors_compact gives, bit for bit, not renormalised -- is above min_post; of more than K candidates the K greatest, among
    equal values the lower pdf.  Returns a list of (pdf int32 [O_u, K], post float32 [O_u, K], count int32 [O_u], views of the call's three
    CUDA outputs: the first count[t] slots of frame t hold its pairs in ascending pdf order, the others (-1, 0); logprob; ok;
    truncated_frames, how many of its frames had more than K candidates).  What write_posterior_archive takes as (key, pdf, post, count)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _posteriors_sparse_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, weight, min_post, max_per_frame, checkpoint=checkpoint)


def label_posteriors_compact(outputs, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, checkpoint=None):
    """posteriors_compact per label (include/tdnnf_hip.h, "label posteriors"), through labelled graphs.  Returns a list of (labels numpy
    int32 [L] = graphs.labels(the utterance's graph), ascending; post float32 [O_u, L] CUDA tensor with post[t, k] = weight x the summed
    posterior of the arcs that carry labels[k]; logprob; ok).  What write_posterior_archive takes as (key, labels, post): with
    transition-ids as labels, the Posterior archive ali-to-post and its relatives exchange."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _posteriors_compact_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, weight, labels=True, checkpoint=checkpoint)


def label_posteriors_sparse(outputs, graphs, utt_graph=None, acoustic_scale=1.0, weight=1.0, min_post=0.01, max_per_frame=16, checkpoint=None):
    """posteriors_sparse per label: the selection over label_posteriors_compact's values and the graphs' label lists.  Returns a list of
    (label int32 [O_u, K], post float32 [O_u, K], count int32 [O_u], logprob, ok, truncated_frames) as posteriors_sparse does.  What
    write_posterior_archive takes as (key, label, post, count)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _posteriors_sparse_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale, weight, min_post, max_per_frame,
                                      labels=True, checkpoint=checkpoint)


def logprob(outputs, graphs, utt_graph=None, acoustic_scale=1.0):
    """The total log-likelihood alone (the forward recursion, no per-frame memory): a list of (logprob, ok)."""
    import torch
    if not outputs:
        return []
    frames = [int(o.shape[0]) for o in outputs]
    return _logprob_stacked(torch.cat(list(outputs)).contiguous(), frames, graphs, utt_graph, acoustic_scale)


def _posteriors_stacked(y, frames, graphs, utt_graph, acoustic_scale, weight, checkpoint=None):
    """posteriors on the utterances' rows stacked in one matrix (what tdnnf_infer_compute writes): row_stride 1"""
    import torch
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    post, results = graphs.posteriors(y, frames, rows, 1, utt_graph, acoustic_scale, weight, checkpoint=checkpoint)
    res = results.cpu().numpy()  # (waits for the stream)
    return [(p, float(res[u, 0]), bool(res[u, 1] == 1.0)) for u, p in enumerate(torch.split(post, frames))]


def _posteriors_compact_stacked(y, frames, graphs, utt_graph, acoustic_scale, weight, labels=False, checkpoint=None):
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    call, column_list = (graphs.label_posteriors_compact, graphs.labels) if labels else (graphs.posteriors_compact, graphs.pdfs)
    values, begin, results = call(y, frames, rows, 1, utt_graph, acoustic_scale, weight, checkpoint=checkpoint)
    res = results.cpu().numpy()  # (waits for the stream)
    lists, out = {}, []
    for u, T in enumerate(frames):
        gi = int(utt_graph[u]) if utt_graph is not None else (0 if graphs.G == 1 else u)
        if gi not in lists:
            lists[gi] = column_list(gi)
        post = values[int(begin[u]):int(begin[u + 1])].view(T, len(lists[gi]))
        out.append((lists[gi], post, float(res[u, 0]), bool(res[u, 1] == 1.0)))
    return out


def _posteriors_sparse_stacked(y, frames, graphs, utt_graph, acoustic_scale, weight, min_post, max_per_frame, labels=False, checkpoint=None):
    import torch
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    pdf, post, count, results = (graphs.label_posteriors_sparse if labels else graphs.posteriors_sparse)(y, frames, rows, 1, utt_graph, acoustic_scale, weight, min_post,
                                                                                                       max_per_frame, checkpoint=checkpoint)
    res = results.cpu().numpy()  # (waits for the stream)
    return [(a, b, c, float(res[u, 0]), bool(res[u, 1] == 1.0), int(res[u, 2]))
            for u, (a, b, c) in enumerate(zip(torch.split(pdf, frames), torch.split(post, frames), torch.split(count, frames)))]


def _logprob_stacked(y, frames, graphs, utt_graph, acoustic_scale):
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    res = graphs.logprob(y, frames, rows, 1, utt_graph, acoustic_scale).cpu().numpy()  # (waits for the stream)
    return [(float(res[u, 0]), bool(res[u, 1] == 1.0)) for u in range(len(frames))]


def write_posterior_archive(path, items, min_post=0.0):
    """Kaldi binary archive of Posterior (vector<vector<pair<int32, BaseFloat>>>): per item `key ' ' \\0B`, then the frame count, and per
    frame the pair count and the (pdf-id, posterior) pairs -- every int32 and float as `\\4` + 4 little-endian bytes, the size-prefixed
    basic-type encoding include/tdnnf_kaldi_io.h restates; what ali-to-post writes and copy-post reads with ark:path.  The layout is
    written AS RECALLED (hmm/posterior.cc WritePosterior), not checked against a Kaldi build.  items: iterable of (key, post [frames,
    num_pdfs]) with numpy or torch matrices; entries with post <= min_post are dropped, pdf-ids ascend within a frame.  An item may also be
    (key, pdf_ids [D], post [frames, D]), the compact form of posteriors_compact: column k holds pdf pdf_ids[k], ascending, and every other
    pdf 0 -- the same bytes as the dense matrix gives, without forming it.  Or (key, pdf [frames, K], post [frames, K], count [frames]), the
    sparse form of posteriors_sparse: of frame t the first count[t] pairs with post > min_post are written, in their order (ascending pdf).
    Where no frame was truncated and min_post is at least the call's, these are the dense matrix's bytes again."""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
    with open(path, "wb") as f:
        for item in items:
            if len(item) == 4:
                _write_sparse_posterior(f, item[0], *[np.asarray(host(a)) for a in item[1:]], min_post)
                continue
            key, m = item[0], item[-1]
            if hasattr(m, "detach"):
                m = m.detach().cpu().numpy()
            m = np.asarray(m, dtype=np.float32)
            assert m.ndim == 2 and " " not in key and key
            pdf_ids = None
            if len(item) == 3:
                pdf_ids = np.asarray(item[1].detach().cpu().numpy() if hasattr(item[1], "detach") else item[1], dtype=np.int32).reshape(-1)
                assert len(pdf_ids) == m.shape[1] and (np.diff(pdf_ids) > 0).all()
                assert min_post >= 0  # (below 0 the dense form writes the zeros of the pdfs outside the list)
            f.write(key.encode() + b" \0B")
            f.write(struct.pack("<bi", 4, m.shape[0]))
            for row in m:
                ids = np.nonzero(row > min_post)[0]
                f.write(struct.pack("<bi", 4, len(ids)))
                pairs = np.zeros(len(ids), dtype=[("a", "i1"), ("pdf", "<i4"), ("b", "i1"), ("post", "<f4")])
                pairs["a"], pairs["b"], pairs["pdf"], pairs["post"] = 4, 4, ids if pdf_ids is None else pdf_ids[ids], row[ids]
                f.write(pairs.tobytes())


def _write_sparse_posterior(f, key, pdf, post, count, min_post):
    """one (key, pdf, post, count) item of write_posterior_archive: no row is searched -- one mask over frames x K slots"""
    pdf, post, count = pdf.astype("<i4", copy=False), post.astype("<f4", copy=False), count.reshape(-1)
    assert pdf.ndim == 2 and pdf.shape == post.shape and len(count) == len(pdf) and " " not in key and key
    keep = (np.arange(pdf.shape[1])[None, :] < count[:, None]) & (post > min_post)
    f.write(key.encode() + b" \0B")
    f.write(struct.pack("<bi", 4, len(pdf)))
    head = np.zeros(len(pdf), dtype=[("a", "i1"), ("n", "<i4")])
    head["a"], head["n"] = 4, keep.sum(1)
    pairs = np.zeros(int(head["n"].sum()), dtype=[("a", "i1"), ("pdf", "<i4"), ("b", "i1"), ("post", "<f4")])
    pairs["a"], pairs["b"], pairs["pdf"], pairs["post"] = 4, 4, pdf[keep], post[keep]  # (row-major: frame after frame, slots ascending)
    ends = np.cumsum(head["n"])
    hb, pb = head.tobytes(), pairs.tobytes()
    for t in range(len(pdf)):
        f.write(hb[5 * t:5 * t + 5])
        f.write(pb[10 * (ends[t] - head["n"][t]):10 * ends[t]])


def read_posterior_archive(path):
    """What write_posterior_archive wrote: {key: [frames][(pdf-id, posterior)]} (tests)."""
    data, pos, out = open(path, "rb").read(), 0, {}

    def basic(fmt):
        nonlocal pos
        assert data[pos] == 4, (pos, data[pos])
        v, = struct.unpack_from(fmt, data, pos + 1)
        pos += 5
        return v

    while pos < len(data):
        end = data.index(b" ", pos)
        key = data[pos:end].decode()
        assert data[end + 1:end + 3] == b"\0B", key
        pos = end + 3
        frames = []
        for _ in range(basic("<i")):
            n = basic("<i")
            frames.append([(basic("<i"), basic("<f")) for _ in range(n)])
        out[key] = frames
    return out
