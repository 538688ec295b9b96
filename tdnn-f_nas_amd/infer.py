"""The model's output for decoding (include/tdnnf_hip.h, "inference"): plumbing around tdnnf_infer_*.

AcousticModel computes, for whole utterances of any length, what nnet3's DecodableNnetSimple hands to
latgen-faster-mapped (steps/nnet3/decode.sh --acwt 1.0, run_tdnn_fbk_40_iv_sp_7q.sh:254-258); write_matrix_archive
stores it as a Kaldi binary float-matrix archive.  Every computation is a call into the HIP library.
"""
import ctypes as C
import struct

import numpy as np

from . import hipabi, trainer

OUTPUTS = {"output": 0, "output-xent": 1}


class AcousticModel:
    """Forward-only view of a ChainNet's model: reads its parameters and BatchNorm statistics at every compute."""

    def __init__(self, net, frames_per_chunk=150, max_chunks=256, output="output"):
        self.lib = hipabi.load()
        self.net = net  # keeps the model alive
        self.frames_per_chunk, self.max_chunks, self.output = int(frames_per_chunk), int(max_chunks), output
        self.fsf = int(net.cfg.frame_subsampling)
        self.num_pdfs = int(net.cfg.num_pdfs)
        self.h = C.c_void_p()
        hipabi.check(self.lib.tdnnf_infer_create(net.h, self.frames_per_chunk, self.max_chunks, OUTPUTS[output], C.byref(self.h)))

    @classmethod
    def from_model_file(cls, path, frames_per_chunk=150, max_chunks=256, output="output"):
        """A model read from an nnet3 raw model file (tdnnf_net_config_from_model + tdnnf_net_read_model)."""
        cfg = trainer.config_from_model(path, frames_per_chunk=frames_per_chunk, num_sequences=1)
        cfg.cv_update = 1  # (no dropout masks; the statistics are only read)
        net = trainer.ChainNet(cfg)
        net.read_model(path)
        return cls(net, frames_per_chunk, max_chunks, output)

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
        return list(torch.split(out, outs)) if outs else []

    def counts(self):
        """(fused_layers, fallback_passes) of the last compute."""
        a, b = C.c_int(), C.c_int()
        hipabi.check(self.lib.tdnnf_infer_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


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
