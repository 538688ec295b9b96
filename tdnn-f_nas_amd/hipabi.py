"""ctypes binding of libtdnnf_hip.so (the C-ABI in include/tdnnf_hip.h) for torch tensors.

Plumbing only: torch provides device memory and streams; every computation is a
call into the HIP library.  Fails loudly if the library is missing -- there is no
CPU or PyTorch fallback for any op.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtdnnf_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "tdnnf_hip.h")
MAX_OFFSETS = 16
OBJECTIVE_STORE_BATCHNORM_STATS = 1  # TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS (tdnnf_net_objective's flags)

_lib = None


class Mat(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("stride", C.c_int)]


class TdnnIndexes(C.Structure):
    _fields_ = [("row_stride", C.c_int), ("num_offsets", C.c_int), ("row_offsets", C.c_int * MAX_OFFSETS)]


class HipAbiError(RuntimeError):
    pass


def _prototypes():
    """{name: (restype, [argtypes])} parsed from include/tdnnf_hip.h, so that floats, size_t and
    pointers are marshalled with their C types (ctypes' defaults would pass float as double)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(tdnnf_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()

        def ctype(decl):
            decl = decl.strip()
            if "*" in decl or decl.startswith("tdnnf_stream"):
                return C.c_void_p
            if decl.startswith("size_t"):
                return C.c_size_t
            if decl.startswith("float"):
                return C.c_float
            if decl.startswith("double"):
                return C.c_double
            if decl.startswith("long long"):
                return C.c_longlong
            if decl.startswith("int") or decl.startswith("unsigned"):
                return C.c_int
            raise HipAbiError(f"cannot marshal parameter '{decl}' of {name}")

        args = [] if params in ("", "void") else [ctype(p) for p in params.split(",")]
        if "*" in ret:
            res = C.c_char_p if "char" in ret else C.c_void_p
        elif ret.startswith("void"):
            res = None
        elif ret.startswith("size_t"):
            res = C.c_size_t
        elif ret.startswith("long long"):
            res = C.c_longlong
        else:
            res = C.c_int
        protos[name] = (res, args)
    return protos


def declared_symbols():
    """Every function name declared in include/tdnnf_hip.h."""
    return sorted(_prototypes())


def load():
    """dlopen the library and check that it exports every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipAbiError(f"{LIB_PATH} is not built: run `python __graft_entry__.py` (hipcc --offload-arch=gfx950)")
    # torch first: its wheel carries a libamdhip64 of its own (soname libamdhip64.so.7), which the library's NEEDED entry
    # then resolves to.  The other order maps /opt/rocm's runtime as well, and the second HIP runtime of a process finds no
    # device (hipErrorNoDevice in the first launch).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    missing = []
    for s in declared_symbols():
        try:
            getattr(lib, s)
        except AttributeError:
            missing.append(s)
    if missing:
        raise HipAbiError(f"libtdnnf_hip.so does not export: {missing}")
    for name, (res, args) in _prototypes().items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise HipAbiError(f"tdnnf error {rc}: {load().tdnnf_last_error().decode()}")


def mat(t):
    """torch 2-D float32 CUDA tensor (unit column stride) -> tdnnf_mat by value."""
    import torch
    assert t.dtype == torch.float32 and t.dim() == 2 and t.is_cuda, (t.dtype, t.shape, t.device)
    assert t.shape[1] <= 1 or t.stride(1) == 1
    stride = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    return Mat(t.data_ptr(), t.shape[0], t.shape[1], stride)


def pmat(t):
    return C.byref(mat(t)) if t is not None else None


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def indexes(row_stride, row_offsets):
    ix = TdnnIndexes()
    ix.row_stride = int(row_stride)
    ix.num_offsets = len(row_offsets)
    for i, o in enumerate(row_offsets):
        ix.row_offsets[i] = int(o)
    return ix


def iarr(a):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def farr(a):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def workspace(nbytes, device="cuda"):
    import torch
    return torch.empty((int(nbytes) + 3) // 4 + 4, dtype=torch.float32, device=device)


class option:
    """`with option("ng_fuse", 0): ...` -- a tuning option of the library (tdnnf_set_option) for the duration of a block."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        lib = load()
        old = C.c_int()
        check(lib.tdnnf_get_option(self.name, C.byref(old)))
        self.old = old.value
        check(lib.tdnnf_set_option(self.name, self.value))
        return self

    def __exit__(self, *exc):
        check(load().tdnnf_set_option(self.name, self.old))
        return False


def _checkpoint(value):
    """The scope of a `checkpoint=` keyword (AlignGraphs): None leaves option align_checkpoint as it is, an int sets it for the block."""
    import contextlib
    return contextlib.nullcontext() if value is None else option("align_checkpoint", value)


def _path_checkpoint(value):
    """The same for the best-path methods' `checkpoint=` keyword and option align_path_checkpoint."""
    import contextlib
    return contextlib.nullcontext() if value is None else option("align_path_checkpoint", value)


def launch_forms(reset=False):
    """{name: value} of the non-zero GEMM launch-form counters (tdnnf_gemm_launch_forms); reset: clear them all afterwards."""
    lib = load()
    n = lib.tdnnf_gemm_launch_forms(None, 0, 0)
    counts = (C.c_longlong * n)()
    lib.tdnnf_gemm_launch_forms(counts, n, 1 if reset else 0)
    return {lib.tdnnf_gemm_launch_form_name(i).decode(): int(counts[i]) for i in range(n) if counts[i]}


def fused_forms(reset=False):
    """{name: count} of the non-zero counters of the fused BatchNorm / ReLU sweeps' forms (tdnnf_fused_launch_forms); reset: clear them
    all afterwards."""
    lib = load()
    n = lib.tdnnf_fused_launch_forms(None, 0, 0)
    counts = (C.c_longlong * n)()
    lib.tdnnf_fused_launch_forms(counts, n, 1 if reset else 0)
    return {lib.tdnnf_fused_launch_form_name(i).decode(): int(counts[i]) for i in range(n) if counts[i]}


def chain_split_region_bytes(den_graph, num_sequences, frames_per_sequence):
    """Diagnostics (tdnnf_chain_split_region_bytes): the bytes at the end of the chain workspace that only the denominator's side-by-side
    recursions and their occupancy pass touch -- what a trainer under option den_split 0 leaves out.  Follows tdnnf_chain_set_denominator_mode."""
    return int(load().tdnnf_chain_split_region_bytes(den_graph.h, int(num_sequences), int(frames_per_sequence)))


class DenGraph:
    def __init__(self, g):
        lib = load()
        self.h = C.c_void_p()
        self._keep = [iarr(g["src"]), iarr(g["dst"]), iarr(g["pdf"]), farr(g["prob"]), farr(g["init"])]
        check(lib.tdnnf_den_graph_create(int(g["H"]), len(g["src"]), int(g["P"]), self._keep[0][1], self._keep[1][1],
                                         self._keep[2][1], self._keep[3][1], self._keep[4][1], 0, C.byref(self.h)))
        self.H, self.P = int(g["H"]), int(g["P"])

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_den_graph_destroy(self.h)
            self.h = None


def _slots(transcripts):
    """A batch of transcripts -- each a (units, optional) pair of int sequences of one length -- as the three arrays of the C entries:
    (slot_begin, slot_unit, slot_optional), each an (array, pointer) pair of iarr."""
    import numpy as np
    transcripts = [(np.asarray(u, dtype=np.int64).reshape(-1), np.asarray(o, dtype=np.int64).reshape(-1)) for u, o in transcripts]
    for g, (u, o) in enumerate(transcripts):
        if len(u) != len(o):
            raise HipAbiError(f"transcript {g}: {len(u)} units and {len(o)} optional flags")
    begin = np.concatenate([[0], np.cumsum([len(u) for u, _ in transcripts])])
    cat = lambda i: np.concatenate([t[i] for t in transcripts]) if transcripts else np.zeros(0, np.int64)
    return iarr(begin), iarr(cat(0)), iarr(cat(1) != 0)


def _pronunciations(transcripts):
    """A batch of transcripts with pronunciation alternatives -- each (positions, optional[, alt_logprob]): positions[p] a list of unit
    sequences, optional[p] a flag, alt_logprob[p] a list of floats (default 0) -- as the six arrays of the C entries: (pos_begin,
    pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units), each an (array, pointer) pair of iarr / farr."""
    pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units = [0], [], [0], [], [0], []
    for g, t in enumerate(transcripts):
        positions, optional = t[0], t[1]
        logprob = t[2] if len(t) > 2 and t[2] is not None else [[0.0] * len(pos) for pos in positions]
        if len(positions) != len(optional) or len(logprob) != len(positions):
            raise HipAbiError(f"transcript {g}: {len(positions)} positions, {len(optional)} optional flags and {len(logprob)} rows of alt_logprob")
        for p, (pos, row) in enumerate(zip(positions, logprob)):
            if len(pos) != len(row):
                raise HipAbiError(f"transcript {g} position {p}: {len(pos)} alternatives and {len(row)} alt_logprob")
            for alt, lp in zip(pos, row):
                alt_units.extend(int(u) for u in alt)
                alt_unit_begin.append(len(alt_units))
                alt_logprob.append(float(lp))
            pos_alt_begin.append(len(alt_logprob))
            pos_optional.append(1 if optional[p] else 0)
        pos_begin.append(len(pos_optional))
    return iarr(pos_begin), iarr(pos_optional), iarr(pos_alt_begin), farr(alt_logprob), iarr(alt_unit_begin), iarr(alt_units)


def _alignments(alignments):
    """A minibatch of alignments -- each a (units, starts) pair of int sequences of one length: the units of a sequence and the output
    frames they start at -- as the three arrays of the C entries: (unit_begin, units, starts), each an (array, pointer) pair of iarr."""
    import numpy as np
    alignments = [(np.asarray(u, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)) for u, b in alignments]
    for s, (u, b) in enumerate(alignments):
        if len(u) != len(b):
            raise HipAbiError(f"alignment {s}: {len(u)} units and {len(b)} starts")
    begin = np.concatenate([[0], np.cumsum([len(u) for u, _ in alignments])])
    cat = lambda i: np.concatenate([a[i] for a in alignments]) if alignments else np.zeros(0, np.int64)
    return iarr(begin), iarr(cat(0)), iarr(cat(1))


def _chunks(num_sequences, utt_frames, chunk_begins):
    """(utt_frames, chunk_begin) of a minibatch of chunks as (array, pointer) pairs of iarr: one int a sequence each."""
    import numpy as np
    frames, first = np.asarray(utt_frames, dtype=np.int64).reshape(-1), np.asarray(chunk_begins, dtype=np.int64).reshape(-1)
    if len(frames) != num_sequences or len(first) != num_sequences:
        raise HipAbiError(f"{num_sequences} alignments, {len(frames)} utt_frames and {len(first)} chunk_begins")
    return iarr(frames), iarr(first)


class UnitSet:
    """Device-resident unit set for transcript graphs (tdnnf_unit_set): U units over num_pdfs pdfs, one state per unit with an entry pdf on
    its first frame and a loop pdf on every later one.  entry_pdf / loop_pdf: shape (U,) -- context 0, context-independent -- or (U + 1, U)
    -- context 1, left-biphone: row left + 1, row 0 for "nothing before it".  loop_logprob / leave_logprob: U floats, the weight of the
    self-loop and of every arc that leaves the unit.  take_logprob / skip_logprob: an optional slot taken or skipped.  A transcript is a
    (units, optional) pair of int sequences; AlignGraphs.assign_transcripts and Supervision.assign_transcripts take a list of them."""

    def __init__(self, entry_pdf, loop_pdf, loop_logprob, leave_logprob, num_pdfs, take_logprob=0.0, skip_logprob=0.0):
        import numpy as np
        entry, loop = np.asarray(entry_pdf), np.asarray(loop_pdf)
        self.h = C.c_void_p()
        if entry.ndim not in (1, 2) or entry.shape != loop.shape or (entry.ndim == 2 and entry.shape[0] != entry.shape[1] + 1):
            raise HipAbiError(f"UnitSet: entry_pdf {entry.shape} and loop_pdf {loop.shape} must both be (U,) or (U + 1, U)")
        self.context, self.U, self.P = entry.ndim - 1, int(entry.shape[-1]), int(num_pdfs)
        if len(loop_logprob) != self.U or len(leave_logprob) != self.U:
            raise HipAbiError(f"UnitSet: loop_logprob and leave_logprob must have U = {self.U} entries")
        k = [iarr(entry.reshape(-1)), iarr(loop.reshape(-1)), farr(loop_logprob), farr(leave_logprob)]
        check(load().tdnnf_unit_set_create(self.U, self.P, self.context, k[0][1], k[1][1], k[2][1], k[3][1], float(take_logprob), float(skip_logprob),
                                           C.byref(self.h)))

    def sizes(self, transcripts):
        """tdnnf_transcript_graph_sizes (host only): (states, arcs), numpy int32 arrays with one entry per transcript -- what a reserve
        must cover.  Refuses (HipAbiError) what assign_transcripts refuses."""
        import numpy as np
        begin, unit, opt = _slots(transcripts)
        states, arcs = np.zeros(len(begin[0]) - 1, np.int32), np.zeros(len(begin[0]) - 1, np.int32)
        check(load().tdnnf_transcript_graph_sizes(self.h, len(states), begin[1], unit[1], opt[1], states.ctypes.data_as(C.c_void_p),
                                                  arcs.ctypes.data_as(C.c_void_p)))
        return states, arcs

    def pronunciation_sizes(self, transcripts):
        """tdnnf_pronunciation_graph_sizes (host only): (states, arcs), numpy int32 arrays with one entry per transcript with pronunciation
        alternatives ((positions, optional[, alt_logprob])) -- what a reserve must cover.  Refuses (HipAbiError) what assign_pronunciations
        refuses."""
        import numpy as np
        k = _pronunciations(transcripts)
        states, arcs = np.zeros(len(k[0][0]) - 1, np.int32), np.zeros(len(k[0][0]) - 1, np.int32)
        check(load().tdnnf_pronunciation_graph_sizes(self.h, len(states), *[x[1] for x in k], states.ctypes.data_as(C.c_void_p),
                                                     arcs.ctypes.data_as(C.c_void_p)))
        return states, arcs

    def alignment_sizes(self, alignments, frames_per_sequence, tolerance):
        """tdnnf_alignment_supervision_sizes (host only): (states, arcs), numpy int32 arrays with one entry per alignment -- the lattice
        of each (units, starts) pair with every boundary free to move by +-tolerance frames; what a Supervision.reserve must cover.
        Refuses (HipAbiError) what Supervision.assign_alignments refuses."""
        import numpy as np
        begin, unit, start = _alignments(alignments)
        states, arcs = np.zeros(len(begin[0]) - 1, np.int32), np.zeros(len(begin[0]) - 1, np.int32)
        check(load().tdnnf_alignment_supervision_sizes(self.h, len(states), int(frames_per_sequence), begin[1], unit[1], start[1], int(tolerance),
                                                       states.ctypes.data_as(C.c_void_p), arcs.ctypes.data_as(C.c_void_p)))
        return states, arcs

    def alignment_chunk_sizes(self, alignments, utt_frames, chunk_begins, frames_per_sequence, tolerance):
        """tdnnf_alignment_chunk_supervision_sizes (host only): (states, arcs), numpy int32 arrays with one entry per chunk -- the lattice
        of the frames [chunk_begins[s], chunk_begins[s] + frames_per_sequence) of the utterance of utt_frames[s] frames whose whole
        alignment is alignments[s]; what a Supervision.reserve must cover.  Refuses (HipAbiError) what
        Supervision.assign_alignment_chunks refuses."""
        import numpy as np
        begin, unit, start = _alignments(alignments)
        frames, first = _chunks(len(begin[0]) - 1, utt_frames, chunk_begins)
        states, arcs = np.zeros(len(begin[0]) - 1, np.int32), np.zeros(len(begin[0]) - 1, np.int32)
        check(load().tdnnf_alignment_chunk_supervision_sizes(self.h, len(states), int(frames_per_sequence), begin[1], unit[1], start[1], frames[1], first[1],
                                                             int(tolerance), states.ctypes.data_as(C.c_void_p), arcs.ctypes.data_as(C.c_void_p)))
        return states, arcs

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_unit_set_destroy(self.h)
            self.h = None


class Supervision:
    """Device-resident numerator graphs of one minibatch (tdnnf_supervision).  `s`: a time-synchronous supervision dict
    (synth.make_supervision ...), or -- with a "graphs" key -- an end-to-end one (synth.make_e2e_supervision: {B, T, P, weight, graphs}),
    which goes through from_graphs.  .kind: 0 time-synchronous, 1 end-to-end."""

    def __init__(self, s):
        lib = load()
        self.h = C.c_void_p()
        if "graphs" in s:
            self._create_e2e(s["graphs"], int(s["T"]), float(s.get("weight", 1.0)), s.get("P"))
            return
        k = [iarr(s["seq_state_begin"]), iarr(s["seq_arc_begin"]), iarr(s["state_time"]), farr(s["final_logprob"]),
             iarr(s["arc_src"]), iarr(s["arc_dst"]), iarr(s["arc_pdf"]), farr(s["arc_logprob"])]
        check(lib.tdnnf_supervision_create(int(s["B"]), int(s["T"]), k[0][1], k[1][1], k[2][1], k[3][1], k[4][1], k[5][1],
                                           k[6][1], k[7][1], float(s.get("weight", 1.0)), C.byref(self.h)))
        self.B, self.T = int(s["B"]), int(s["T"])

    @classmethod
    def from_graphs(cls, graphs, frames_per_sequence, weight=1.0, num_pdfs=None):
        """End-to-end supervision (tdnnf_supervision_create_e2e): one cyclic pdf-labelled graph per sequence, each a dict {S, P, src, dst,
        pdf, logprob, init, final} with states numbered from 0, stacked as AlignGraphs stacks them.  num_pdfs: default the graphs' largest P."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self._create_e2e(graphs, int(frames_per_sequence), float(weight), num_pdfs)
        return self

    @staticmethod
    def _stack_e2e(graphs):
        """(graphs as a list, the eight arrays of tdnnf_supervision_create_e2e stacked as AlignGraphs stacks them)"""
        import numpy as np
        graphs = [graphs] if isinstance(graphs, dict) else list(graphs)
        sb = np.concatenate([[0], np.cumsum([int(g["S"]) for g in graphs])])
        ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])])
        cat = lambda key, off=None: np.concatenate([np.asarray(g[key]) + (0 if off is None else off[i]) for i, g in enumerate(graphs)])
        return graphs, [iarr(sb), iarr(ab), iarr(cat("src", sb)), iarr(cat("dst", sb)), iarr(cat("pdf")), farr(cat("logprob")), farr(cat("init")),
                        farr(cat("final"))]

    def _create_e2e(self, graphs, T, weight, num_pdfs):
        graphs, k = self._stack_e2e(graphs)
        P = int(num_pdfs if num_pdfs is not None else max(int(g["P"]) for g in graphs))
        check(load().tdnnf_supervision_create_e2e(len(graphs), T, P, *[x[1] for x in k], weight, C.byref(self.h)))
        self.B, self.T, self.P = len(graphs), T, P

    @classmethod
    def reserve_e2e(cls, max_sequences, max_frames, num_pdfs, max_states, max_arcs):
        """A reusable end-to-end supervision (tdnnf_supervision_reserve_e2e): every allocation is made here, for minibatches of at most
        max_sequences graphs with max_states states and max_arcs arcs between them and max_frames frames per sequence.  It holds no
        minibatch until assign (B = T = 0) and is refused until then."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.B, self.T, self.P = 0, 0, int(num_pdfs)
        check(load().tdnnf_supervision_reserve_e2e(int(max_sequences), int(max_frames), self.P, int(max_states), int(max_arcs), C.byref(self.h)))
        return self

    @classmethod
    def reserve(cls, max_sequences, max_frames, max_states, max_arcs):
        """A reusable time-synchronous supervision (tdnnf_supervision_reserve): every allocation is made here, for minibatches of at most
        max_sequences sequences of max_frames frames with max_states states and max_arcs arcs between them.  It holds no minibatch until
        assign (B = T = 0) and is refused until then."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.B, self.T = 0, 0
        check(load().tdnnf_supervision_reserve(int(max_sequences), int(max_frames), int(max_states), int(max_arcs), C.byref(self.h)))
        return self

    def assign(self, graphs, frames_per_sequence=None, weight=None):
        """The reserved supervision's next minibatch, on the current stream.  Nothing is allocated or synchronised; B and T follow.  A
        refused minibatch (HipAbiError) leaves the previous one.
        A supervision of reserve: assign(s), s the dict of synth.make_supervision that Supervision(s) takes (tdnnf_supervision_assign:
        the tables are built on the device); weight overrides the dict's.
        A supervision of reserve_e2e: assign(graphs, frames_per_sequence, weight=1.0) (tdnnf_supervision_assign_e2e: graphs, frames and
        weight may all change)."""
        if isinstance(graphs, dict) and "seq_state_begin" in graphs:
            s = graphs
            if self.kind != 0:
                raise HipAbiError("Supervision.assign: a time-synchronous supervision dict given to an end-to-end supervision "
                                  "(reserve_e2e); its assign takes (graphs, frames_per_sequence, weight)")
            if frames_per_sequence is not None:
                raise HipAbiError("Supervision.assign: a supervision dict carries its frames (\"T\"); frames_per_sequence belongs to the end-to-end form")
            k = [iarr(s["seq_state_begin"]), iarr(s["seq_arc_begin"]), iarr(s["state_time"]), farr(s["final_logprob"]),
                 iarr(s["arc_src"]), iarr(s["arc_dst"]), iarr(s["arc_pdf"]), farr(s["arc_logprob"])]
            w = float(s.get("weight", 1.0) if weight is None else weight)
            check(load().tdnnf_supervision_assign(self.h, int(s["B"]), int(s["T"]), *[x[1] for x in k], w, stream()))
            self.B, self.T = int(s["B"]), int(s["T"])
            return
        if self.kind != 1:
            raise HipAbiError("Supervision.assign: graphs and frames_per_sequence given to a time-synchronous supervision (reserve); its "
                              "assign takes the dict of synth.make_supervision")
        if frames_per_sequence is None:
            raise HipAbiError("Supervision.assign: the end-to-end form needs frames_per_sequence")
        weight = 1.0 if weight is None else weight
        graphs, k = self._stack_e2e(graphs)
        check(load().tdnnf_supervision_assign_e2e(self.h, len(graphs), int(frames_per_sequence), *[x[1] for x in k], float(weight), stream()))
        self.B, self.T = len(graphs), int(frames_per_sequence)

    def assign_transcripts(self, unit_set, transcripts, frames_per_sequence, weight=1.0):
        """tdnnf_supervision_assign_e2e_transcripts on the current stream: assign with the graphs compiled on the device from one
        (units, optional) transcript per sequence (UnitSet).  A refused minibatch (HipAbiError) leaves the previous one."""
        begin, unit, opt = _slots(transcripts)
        check(load().tdnnf_supervision_assign_e2e_transcripts(self.h, unit_set.h, len(begin[0]) - 1, int(frames_per_sequence), begin[1], unit[1], opt[1],
                                                              float(weight), stream()))
        self.B, self.T = len(begin[0]) - 1, int(frames_per_sequence)

    def assign_pronunciations(self, unit_set, transcripts, frames_per_sequence, weight=1.0):
        """tdnnf_supervision_assign_e2e_pronunciations on the current stream: assign with the graphs compiled on the device from one
        (positions, optional[, alt_logprob]) transcript per sequence, positions[p] the list of unit sequences that pronounce position p
        (UnitSet).  A refused minibatch (HipAbiError) leaves the previous one."""
        k = _pronunciations(transcripts)
        check(load().tdnnf_supervision_assign_e2e_pronunciations(self.h, unit_set.h, len(k[0][0]) - 1, int(frames_per_sequence), *[x[1] for x in k],
                                                                 float(weight), stream()))
        self.B, self.T = len(k[0][0]) - 1, int(frames_per_sequence)

    def assign_alignments(self, unit_set, alignments, frames_per_sequence, tolerance, weight=1.0):
        """tdnnf_supervision_assign_alignments on the current stream: the next minibatch of a supervision of reserve, its lattices compiled
        on the device from one (units, starts) alignment per sequence (UnitSet; starts in output frames, the first 0) with every unit
        boundary free to move by +-tolerance frames.  A refused minibatch (HipAbiError) leaves the previous one."""
        begin, unit, start = _alignments(alignments)
        check(load().tdnnf_supervision_assign_alignments(self.h, unit_set.h, len(begin[0]) - 1, int(frames_per_sequence), begin[1], unit[1], start[1],
                                                         int(tolerance), float(weight), stream()))
        self.B, self.T = len(begin[0]) - 1, int(frames_per_sequence)

    def assign_alignment_chunks(self, unit_set, alignments, utt_frames, chunk_begins, frames_per_sequence, tolerance, weight=1.0):
        """tdnnf_supervision_assign_alignment_chunks on the current stream: the next minibatch of a supervision of reserve, sequence s
        the frames [chunk_begins[s], chunk_begins[s] + frames_per_sequence) of an utterance of utt_frames[s] output frames, its lattice
        compiled on the device from the (units, starts) alignment of the WHOLE utterance, alignments[s], with every unit boundary free to
        move by +-tolerance frames (infer.chunk_begins spreads chunks over an utterance; two chunks of one utterance repeat its
        alignment).  A refused minibatch (HipAbiError) leaves the previous one."""
        begin, unit, start = _alignments(alignments)
        frames, first = _chunks(len(begin[0]) - 1, utt_frames, chunk_begins)
        check(load().tdnnf_supervision_assign_alignment_chunks(self.h, unit_set.h, len(begin[0]) - 1, int(frames_per_sequence), begin[1], unit[1], start[1],
                                                               frames[1], first[1], int(tolerance), float(weight), stream()))
        self.B, self.T = len(begin[0]) - 1, int(frames_per_sequence)

    @property
    def kind(self):
        return int(load().tdnnf_supervision_kind(self.h))

    def e2e_form(self):
        """{threads, vectors_in_lds, rows_in_lds}: the launch form of an end-to-end supervision's recursion (tdnnf_supervision_e2e_form)."""
        v = [C.c_int() for _ in range(3)]
        check(load().tdnnf_supervision_e2e_form(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("threads", "vectors_in_lds", "rows_in_lds"), (x.value for x in v)))

    TABLES = ("seq_state_begin", "state_time", "final_logprob", "frame_state_begin", "in_begin", "in_src", "in_pdf", "in_lp", "out_begin",
              "out_dst", "out_pdf", "out_lp", "pf_src", "pf_dst", "pf_pdf", "pf_t", "pf_lp")

    def capacity(self):
        """{max_sequences, max_frames, max_states, max_arcs, assigns, allocations, device_bytes} of a supervision of reserve
        (tdnnf_supervision_capacity); allocations: device and pinned allocations since reserve returned."""
        v = [C.c_int() for _ in range(6)] + [C.c_longlong()]
        check(load().tdnnf_supervision_capacity(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("max_sequences", "max_frames", "max_states", "max_arcs", "assigns", "allocations", "device_bytes"), (int(x.value) for x in v)))

    def tables(self):
        """The device tables of a time-synchronous supervision, created or assigned, as numpy arrays by name (tdnnf_supervision_dump; waits
        for the current stream): Supervision.TABLES, int32 but for final_logprob and the *_lp (float32).  A table the supervision does not
        carry (pf_* of a narrow created one) is empty."""
        import numpy as np
        lib, t = load(), {}
        for name in self.TABLES:
            n = C.c_longlong()
            check(lib.tdnnf_supervision_dump(self.h, name.encode(), None, 0, C.byref(n), stream()))
            out = np.zeros(n.value, np.float32 if name.endswith("_lp") or name == "final_logprob" else np.int32)
            check(lib.tdnnf_supervision_dump(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), stream()))
            t[name] = out
        return t

    def info(self):
        """{num_states, num_arcs, max_states_per_frame, wide} (tdnnf_supervision_info); wide: over 4 states per frame on average,
        the supervision holds its own numerator scratch and takes the numerator's wide form.  End-to-end kind: the totals over its
        graphs, max_states_per_frame the largest graph's state count, wide 0."""
        v = [C.c_int() for _ in range(4)]
        check(load().tdnnf_supervision_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("num_states", "num_arcs", "max_states_per_frame", "wide"), (x.value for x in v)))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_supervision_destroy(self.h)
            self.h = None


class AlignGraphs:
    """Device-resident set of pdf-labelled graphs for best-path alignment and forward-backward (tdnnf_align_graphs).  `graphs`: one graph or a list of graphs,
    each a dict {S, P, src, dst, pdf, logprob, init, final} with states numbered from 0 (synth.make_alignment_graph,
    synth.alignment_graph_from_den); they are stacked with the state numbering of tdnnf_align_graphs_create.  A graph dict may carry
    "label", one int per arc in [0, num_labels) -- all graphs or none: with labels the handle is tdnnf_align_graphs_create_labelled's and
    serves the label methods (labels, best_path_labels, label_posteriors_*) as well.  num_labels: default the largest label + 1."""

    def __init__(self, graphs, num_pdfs=None, num_labels=None):
        lib = load()
        graphs = [graphs] if isinstance(graphs, dict) else list(graphs)
        self.h = C.c_void_p()
        self.reserved = False
        self.P = int(num_pdfs if num_pdfs is not None else max(int(g["P"]) for g in graphs))
        self.labelled = self._stack(graphs)
        if self.labelled:
            lab = self._keep[8]
            self.L = int(num_labels if num_labels is not None else (int(lab[0].max()) + 1 if len(lab[0]) else 1))
            check(lib.tdnnf_align_graphs_create_labelled(self.G, self.P, *[k[1] for k in self._keep], self.L, C.byref(self.h)))
        else:
            if num_labels is not None:
                raise HipAbiError("AlignGraphs: num_labels without a \"label\" array in the graphs")
            self.L = 0
            check(lib.tdnnf_align_graphs_create(self.G, self.P, *[k[1] for k in self._keep], C.byref(self.h)))
        self.num_states = [int(g["S"]) for g in graphs]

    def _stack(self, graphs):
        """The graphs' arrays stacked with the state numbering of tdnnf_align_graphs_create into self._keep (the eight arrays, and the labels
        where every graph carries them); sets G and arc_begin.  Returns whether the graphs carry labels."""
        import numpy as np
        self.G = len(graphs)
        sb = np.concatenate([[0], np.cumsum([int(g["S"]) for g in graphs])])
        ab = np.concatenate([[0], np.cumsum([len(g["src"]) for g in graphs])])
        cat = lambda key, off=None: np.concatenate([np.asarray(g[key]) + (0 if off is None else off[i]) for i, g in enumerate(graphs)])
        self._keep = [iarr(sb), iarr(ab), iarr(cat("src", sb)), iarr(cat("dst", sb)), iarr(cat("pdf")), farr(cat("logprob")),
                      farr(cat("init")), farr(cat("final"))]
        with_label = ["label" in g for g in graphs]
        if any(with_label) != all(with_label):
            raise HipAbiError("AlignGraphs: every graph carries a \"label\" array, or none does")
        self.arc_begin = ab.astype(np.int64)
        if all(with_label):
            self._keep.append(iarr(cat("label")))
        return all(with_label)

    @classmethod
    def reserve(cls, max_graphs, num_pdfs, max_states, max_arcs, num_labels=None):
        """A reusable graph set (tdnnf_align_graphs_reserve): every allocation is made here for max_graphs graphs with max_states states and
        max_arcs arcs between them; num_labels: None or 0 an unlabelled handle, else one whose every batch carries "label" arrays.  It holds
        no graphs until assign, and every method refuses it until then."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.reserved = True
        self.P, self.L = int(num_pdfs), int(num_labels or 0)
        self.labelled = self.L > 0
        self.G, self.num_states, self.arc_begin, self._keep = 0, [], None, []
        check(load().tdnnf_align_graphs_reserve(int(max_graphs), self.P, self.L, int(max_states), int(max_arcs), C.byref(self.h)))
        return self

    def assign(self, graphs, stream=None):
        """tdnnf_align_graphs_assign: the handle's next batch, built on the device in stream order (stream: a raw stream, default the current
        one).  Nothing is allocated or synchronised; G, num_states, arc_begin follow the new batch, and every method works on it.  A refused
        batch (HipAbiError) leaves the handle and this object on the previous one."""
        import torch
        graphs = [graphs] if isinstance(graphs, dict) else list(graphs)
        before = (self.G, self.arc_begin, self._keep)
        on = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        try:
            labelled = self._stack(graphs)
            check(load().tdnnf_align_graphs_assign(self.h, self.G, *[k[1] for k in self._keep[:8]], self._keep[8][1] if labelled else None, on))
        except HipAbiError:
            self.G, self.arc_begin, self._keep = before
            raise
        self.num_states = [int(g["S"]) for g in graphs]

    def assign_transcripts(self, unit_set, transcripts, stream=None):
        """tdnnf_align_graphs_assign_transcripts: the handle's next batch compiled on the device from (units, optional) transcripts (UnitSet),
        in stream order as assign; on a labelled handle an arc's label is the slot it enters.  G, num_states and arc_begin follow the new
        batch.  A refused batch (HipAbiError) leaves the handle and this object on the previous one."""
        import numpy as np
        import torch
        begin, unit, opt = _slots(transcripts)
        on = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        check(load().tdnnf_align_graphs_assign_transcripts(self.h, unit_set.h, len(begin[0]) - 1, begin[1], unit[1], opt[1], on))
        states, arcs = unit_set.sizes(transcripts)
        self.G, self._keep = len(states), []
        self.num_states = [int(s) for s in states]
        self.arc_begin = np.concatenate([[0], np.cumsum(arcs)]).astype(np.int64)

    def assign_pronunciations(self, unit_set, transcripts, stream=None):
        """tdnnf_align_graphs_assign_pronunciations: the handle's next batch compiled on the device from transcripts with pronunciation
        alternatives -- each (positions, optional[, alt_logprob]), positions[p] a list of unit sequences (UnitSet) -- in stream order as
        assign; on a labelled handle an arc's label is the entry it enters, the entries numbered in flat order (position, alternative,
        unit).  G, num_states and arc_begin follow the new batch.  A refused batch (HipAbiError) leaves the handle and this object on the
        previous one."""
        import numpy as np
        import torch
        k = _pronunciations(transcripts)
        on = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        check(load().tdnnf_align_graphs_assign_pronunciations(self.h, unit_set.h, len(k[0][0]) - 1, *[x[1] for x in k], on))
        states, arcs = unit_set.pronunciation_sizes(transcripts)
        self.G, self._keep = len(states), []
        self.num_states = [int(s) for s in states]
        self.arc_begin = np.concatenate([[0], np.cumsum(arcs)]).astype(np.int64)

    def capacity(self):
        """{max_graphs, max_states, max_arcs, device_bytes, device_allocs, assigns} of a reserved handle (tdnnf_align_graphs_capacity)."""
        v = [C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_int(), C.c_int()]
        check(load().tdnnf_align_graphs_capacity(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("max_graphs", "max_states", "max_arcs", "device_bytes", "device_allocs", "assigns"), (int(x.value) for x in v)))

    def tables(self):
        """The device arrays of the handle as numpy int32 arrays (tdnnf_align_graphs_dump; waits for the last assign): {"by_dst" / "by_src" /
        "by_pdf" [/ "by_label"]: {"slots", "heavy", "arcs"} of shape [n, 4], "graphs" [G, 14], "label_ranges", "pdf_columns",
        "label_columns", "init", "final", "labels"}."""
        import numpy as np
        lib = load()

        def dump(table, which):
            n = C.c_longlong()
            check(lib.tdnnf_align_graphs_dump(self.h, table, which, None, 0, C.byref(n)))
            out = np.zeros(n.value, np.int32)
            check(lib.tdnnf_align_graphs_dump(self.h, table, which, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
            return out

        t = {}
        for i, name in enumerate(("by_dst", "by_src", "by_pdf", "by_label")[:4 if self.L > 0 else 3]):
            t[name] = {w: dump(i, j).reshape(-1, 4) for j, w in enumerate(("slots", "heavy", "arcs"))}
        for j, name in enumerate(("graphs", "label_ranges", "pdf_columns", "label_columns", "init", "final", "labels")):
            t[name] = dump(4, j)
        t["graphs"] = t["graphs"].reshape(-1, 14)
        return t

    @classmethod
    def from_den_graph(cls, g):
        """The graph of the free best path through a denominator graph: arcs log(prob), initial log(init) (-inf where init is 0),
        every state final at 0."""
        from . import synth
        return cls(synth.alignment_graph_from_den(g))

    def info(self, graph=0):
        """{num_states, num_arcs, max_in_degree} of one graph (tdnnf_align_graphs_info)."""
        v = [C.c_int() for _ in range(3)]
        check(load().tdnnf_align_graphs_info(self.h, int(graph), *[C.byref(x) for x in v]))
        return dict(zip(("num_states", "num_arcs", "max_in_degree"), (x.value for x in v)))

    def workspace_bytes(self, utt_graph, utt_frames, checkpoint=None):
        """tdnnf_align_workspace_bytes (0 for a call it refuses).  checkpoint (here and on best_path / best_path_labels): None reads option
        align_path_checkpoint as it stands; an int (0 off, C >= 1 an interval, -1 automatic) sets it around the workspace question and the
        call and restores it afterwards -- back-pointers of one segment of C frames at a time, the same path."""
        ug = iarr(utt_graph)[1] if utt_graph is not None else None
        with _path_checkpoint(checkpoint):
            return int(load().tdnnf_align_workspace_bytes(self.h, len(utt_frames), ug, iarr(utt_frames)[1]))

    def best_path(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, states=False, checkpoint=None):
        """tdnnf_align_best_path on the current stream.  Returns (pdf_out int32 [sum frames], state_out int32 [sum frames + utterances]
        or None, results float64 [utterances, 2]) as CUDA tensors; nothing is synchronised."""
        with _path_checkpoint(checkpoint):
            return self._best_path(nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, states, False)[:3]

    def best_path_labels(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, states=False,
                         checkpoint=None):
        """tdnnf_align_best_path_labels on the current stream.  Returns (pdf_out, state_out or None, results, label_out int32 [sum frames],
        arc_out int32 [sum frames]) as CUDA tensors: best_path's three, the label of the arc taken at every frame and that arc's index
        LOCAL to the utterance's graph dict (the C call's global index minus the graph's first arc); -1 both where ok is 0.  Nothing is
        synchronised."""
        with _path_checkpoint(checkpoint):
            return self._best_path(nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, states, True)

    def _best_path(self, nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, states, labels):
        import numpy as np
        import torch
        n = len(utt_frames)
        fr, frp = iarr(utt_frames)
        rb, rbp = iarr(utt_row_begin)
        ug = iarr(utt_graph) if utt_graph is not None else (None, None)
        nbytes = int(load().tdnnf_align_workspace_bytes(self.h, n, ug[1], frp))
        if nbytes == 0:
            raise HipAbiError(f"tdnnf_align_workspace_bytes: {load().tdnnf_last_error().decode()}")
        ws = workspace(nbytes)
        total = int(fr.sum())
        pdf_out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        state_out = torch.empty(total + n, dtype=torch.int32, device="cuda") if states else None
        results = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        if not labels:
            check(load().tdnnf_align_best_path(self.h, n, ug[1], frp, rbp, int(row_stride), pmat(nnet_output), float(acoustic_scale), ptr(pdf_out),
                                               ptr(state_out), ptr(results), ptr(ws), nbytes, stream()))
            return pdf_out[:total], state_out, results
        label_out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        arc_out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        check(load().tdnnf_align_best_path_labels(self.h, n, ug[1], frp, rbp, int(row_stride), pmat(nnet_output), float(acoustic_scale), ptr(pdf_out),
                                                  ptr(state_out), ptr(label_out), ptr(arc_out), ptr(results), ptr(ws), nbytes, stream()))
        # the arcs local to each utterance's graph dict: minus the graph's first arc, where there is an arc
        first = np.asarray([self.arc_begin[int(ug[0][u]) if ug[0] is not None else (0 if self.G == 1 else u)] for u in range(n)], dtype=np.int64)
        shift = torch.from_numpy(np.repeat(first, fr).astype(np.int32)).to("cuda")
        arc_out = arc_out[:total]
        arc_out = torch.where(arc_out >= 0, arc_out - shift, arc_out)
        return pdf_out[:total], state_out, results, label_out[:total], arc_out

    def posteriors_workspace_bytes(self, utt_graph, utt_frames, want_posteriors=True, checkpoint=None):
        """tdnnf_align_posteriors_workspace_bytes.  checkpoint (here and on every posterior call below): None reads option
        align_checkpoint as it stands; an int (0 off, C >= 1 an interval, -1 automatic) sets it around the workspace question and the call
        and restores it afterwards -- alpha of every C-th frame only, the same bits."""
        ug = iarr(utt_graph)[1] if utt_graph is not None else None
        with _checkpoint(checkpoint):
            return int(load().tdnnf_align_posteriors_workspace_bytes(self.h, len(utt_frames), ug, iarr(utt_frames)[1], 1 if want_posteriors else 0))

    def posteriors_sparse_workspace_bytes(self, utt_graph, utt_frames, max_per_frame=16, checkpoint=None):
        """tdnnf_align_posteriors_sparse_workspace_bytes (0 for a call it refuses)."""
        return self._sparse_workspace_bytes("tdnnf_align_posteriors_sparse", utt_graph, utt_frames, max_per_frame, checkpoint)

    def label_posteriors_sparse_workspace_bytes(self, utt_graph, utt_frames, max_per_frame=16, checkpoint=None):
        """tdnnf_align_label_posteriors_sparse_workspace_bytes (0 for a call it refuses)."""
        return self._sparse_workspace_bytes("tdnnf_align_label_posteriors_sparse", utt_graph, utt_frames, max_per_frame, checkpoint)

    def _sparse_workspace_bytes(self, entry, utt_graph, utt_frames, max_per_frame, checkpoint):
        ug = iarr(utt_graph)[1] if utt_graph is not None else None
        with _checkpoint(checkpoint):
            return int(getattr(load(), entry + "_workspace_bytes")(self.h, len(utt_frames), ug, iarr(utt_frames)[1], int(max_per_frame)))

    def _forward_backward(self, nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight, post, checkpoint=None):
        with _checkpoint(checkpoint):
            return self._forward_backward_call(nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight, post)

    def _forward_backward_call(self, nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight, post):
        import torch
        n = len(utt_frames)
        fr, frp = iarr(utt_frames)
        rb, rbp = iarr(utt_row_begin)
        ug = iarr(utt_graph) if utt_graph is not None else (None, None)
        nbytes = int(load().tdnnf_align_posteriors_workspace_bytes(self.h, n, ug[1], frp, 0 if post is None else 1))
        if nbytes == 0:
            raise HipAbiError(f"tdnnf_align_posteriors_workspace_bytes: {load().tdnnf_last_error().decode()}")
        ws = workspace(nbytes)
        results = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        check(load().tdnnf_align_posteriors(self.h, n, ug[1], frp, rbp, int(row_stride), pmat(nnet_output), float(acoustic_scale), float(weight),
                                            pmat(post), ptr(results), ptr(ws), nbytes, stream()))
        return results

    def posteriors(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, weight=1.0, out=None, checkpoint=None):
        """tdnnf_align_posteriors on the current stream.  Returns (post, results): post float32, addressed like nnet_output (row
        utt_row_begin[u] + t * row_stride) -- `out` if given, else a new zeroed [rows of nnet_output, num_pdfs] matrix; results float64
        [utterances, 2] (logprob, ok).  CUDA tensors; nothing is synchronised."""
        import torch
        post = out if out is not None else torch.zeros((nnet_output.shape[0], self.P), dtype=torch.float32, device="cuda")
        return post, self._forward_backward(nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight, post, checkpoint)

    def pdfs(self, graph=0):
        """The column list of one graph (tdnnf_align_graphs_pdfs): the distinct pdfs its arcs name, ascending, as a numpy int32 array."""
        import numpy as np
        n = C.c_int()
        check(load().tdnnf_align_graphs_pdfs(self.h, int(graph), C.byref(n), None))
        out = np.zeros(n.value, np.int32)
        check(load().tdnnf_align_graphs_pdfs(self.h, int(graph), None, out.ctypes.data_as(C.c_void_p)))
        return out

    def labels(self, graph=0):
        """The label column list of one graph (tdnnf_align_graphs_labels): the distinct labels its arcs carry, ascending, numpy int32."""
        import numpy as np
        n = C.c_int()
        check(load().tdnnf_align_graphs_labels(self.h, int(graph), C.byref(n), None))
        out = np.zeros(n.value, np.int32)
        check(load().tdnnf_align_graphs_labels(self.h, int(graph), None, out.ctypes.data_as(C.c_void_p)))
        return out

    def posteriors_compact_layout(self, utt_frames, utt_graph=None):
        """tdnnf_align_posteriors_compact_layout: utt_begin, numpy int64 [utterances + 1] -- utterance u owns floats
        [utt_begin[u], utt_begin[u + 1]) of the compact output, utt_frames[u] rows of len(pdfs(its graph)) floats."""
        return self._compact_layout("tdnnf_align_posteriors_compact_layout", utt_frames, utt_graph)

    def label_posteriors_compact_layout(self, utt_frames, utt_graph=None):
        """tdnnf_align_label_posteriors_compact_layout: as posteriors_compact_layout with rows of len(labels(its graph)) floats."""
        return self._compact_layout("tdnnf_align_label_posteriors_compact_layout", utt_frames, utt_graph)

    def _compact_layout(self, entry, utt_frames, utt_graph):
        import numpy as np
        n = len(utt_frames)
        ug = iarr(utt_graph) if utt_graph is not None else (None, None)
        begin = np.zeros(n + 1, np.int64)
        check(getattr(load(), entry)(self.h, n, ug[1], iarr(utt_frames)[1], None, begin.ctypes.data_as(C.c_void_p)))
        return begin

    def posteriors_compact(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, weight=1.0, checkpoint=None):
        """tdnnf_align_posteriors_compact on the current stream.  Returns (values, utt_begin, results): values float32 CUDA tensor of
        utt_begin[-1] floats, of which utterance u owns [utt_begin[u], utt_begin[u + 1]) -- utt_frames[u] rows of one float per pdf of
        pdfs(its graph), = weight x the posterior; utt_begin numpy int64; results float64 [utterances, 2] (logprob, ok) CUDA tensor.
        Nothing is synchronised."""
        with _checkpoint(checkpoint):
            return self._compact("tdnnf_align_posteriors_compact", nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight)

    def label_posteriors_compact(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, weight=1.0,
                                 checkpoint=None):
        """tdnnf_align_label_posteriors_compact on the current stream: posteriors_compact per label -- utterance u owns utt_frames[u] rows of
        one float per label of labels(its graph), = weight x the summed posterior of the arcs that carry the label.  Returns (values,
        utt_begin, results) as posteriors_compact does.  Nothing is synchronised."""
        with _checkpoint(checkpoint):
            return self._compact("tdnnf_align_label_posteriors_compact", nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale,
                                 weight)

    def _compact(self, entry, nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight):
        import torch
        n = len(utt_frames)
        fr, frp = iarr(utt_frames)
        rb, rbp = iarr(utt_row_begin)
        ug = iarr(utt_graph) if utt_graph is not None else (None, None)
        begin = self._compact_layout(entry + "_layout", fr, utt_graph)
        nbytes = int(load().tdnnf_align_posteriors_workspace_bytes(self.h, n, ug[1], frp, 1))
        if nbytes == 0:
            raise HipAbiError(f"tdnnf_align_posteriors_workspace_bytes: {load().tdnnf_last_error().decode()}")
        ws = workspace(nbytes)
        elems = int(begin[-1])
        values = torch.empty(elems, dtype=torch.float32, device="cuda")
        results = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        check(getattr(load(), entry)(self.h, n, ug[1], frp, rbp, int(row_stride), pmat(nnet_output), float(acoustic_scale), float(weight),
                                     ptr(values) if elems else None, elems, ptr(results), ptr(ws), nbytes, stream()))
        return values, begin, results

    def posteriors_sparse(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, weight=1.0, min_post=0.01,
                          max_per_frame=16, checkpoint=None):
        """tdnnf_align_posteriors_sparse on the current stream: per frame the at most K = max_per_frame (pdf, value) pairs with value >
        min_post, of the values posteriors_compact gives, in ascending pdf order.  Returns (pdf int32 [F, K], post float32 [F, K], count
        int32 [F], results float64 [utterances, 4]) as CUDA tensors, F = sum(utt_frames), utterance after utterance: the first count[f]
        slots of frame f hold its pairs, the others (-1, 0); results = (logprob, ok, frames with more than K candidates, the greatest
        number of candidates in a frame).  Nothing is synchronised."""
        with _checkpoint(checkpoint):
            return self._sparse("tdnnf_align_posteriors_sparse", nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight,
                                min_post, max_per_frame)

    def label_posteriors_sparse(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0, weight=1.0,
                                min_post=0.01, max_per_frame=16, checkpoint=None):
        """tdnnf_align_label_posteriors_sparse on the current stream: posteriors_sparse over label_posteriors_compact's values and the
        graphs' label lists.  Returns (label int32 [F, K], post float32 [F, K], count int32 [F], results float64 [utterances, 4]) as
        posteriors_sparse does.  Nothing is synchronised."""
        with _checkpoint(checkpoint):
            return self._sparse("tdnnf_align_label_posteriors_sparse", nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale,
                                weight, min_post, max_per_frame)

    def _sparse(self, entry, nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, weight, min_post, max_per_frame):
        import torch
        n = len(utt_frames)
        fr, frp = iarr(utt_frames)
        rb, rbp = iarr(utt_row_begin)
        ug = iarr(utt_graph) if utt_graph is not None else (None, None)
        K = int(max_per_frame)
        nbytes = int(getattr(load(), entry + "_workspace_bytes")(self.h, n, ug[1], frp, K))
        if nbytes == 0:
            raise HipAbiError(f"{entry}_workspace_bytes: {load().tdnnf_last_error().decode()}")
        ws = workspace(nbytes)
        F = int(fr.sum())
        pdf = torch.empty((F, K), dtype=torch.int32, device="cuda")
        post = torch.empty((F, K), dtype=torch.float32, device="cuda")
        count = torch.empty(F, dtype=torch.int32, device="cuda")
        results = torch.empty((n, 4), dtype=torch.float64, device="cuda")
        check(getattr(load(), entry)(self.h, n, ug[1], frp, rbp, int(row_stride), pmat(nnet_output), float(acoustic_scale), float(weight),
                                     float(min_post), K, ptr(pdf) if F else None, ptr(post) if F else None, ptr(count) if F else None, ptr(results),
                                     ptr(ws), nbytes, stream()))
        return pdf, post, count, results

    def logprob(self, nnet_output, utt_frames, utt_row_begin, row_stride=1, utt_graph=None, acoustic_scale=1.0):
        """The same call without a posterior matrix: the forward recursion alone.  Returns results float64 [utterances, 2] (logprob, ok)."""
        return self._forward_backward(nnet_output, utt_frames, utt_row_begin, row_stride, utt_graph, acoustic_scale, 1.0, None)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_align_graphs_destroy(self.h)
            self.h = None


def _sequence_chunks(seq_utt, chunk_begins):
    """(seq_utt, chunk_begin) of a minibatch of chunks as (array, pointer) pairs of iarr: one int a sequence each."""
    import numpy as np
    utt, first = np.asarray(seq_utt, dtype=np.int64).reshape(-1), np.asarray(chunk_begins, dtype=np.int64).reshape(-1)
    if len(utt) != len(first):
        raise HipAbiError(f"{len(utt)} seq_utt and {len(first)} chunk_begins")
    return iarr(utt), iarr(first)


class ChunkInput:
    """The net's input for minibatches of chunks, gathered on the device from whole utterances (tdnnf_chunk_input; include/tdnnf_hip.h,
    "CHUNK INPUTS"): one handle for up to max_sequences sequences, allocated once; every gather stages 16 bytes a sequence and enqueues a
    copy and one kernel on the current stream."""

    def __init__(self, max_sequences):
        self.h = C.c_void_p()
        self.max_sequences = int(max_sequences)
        check(load().tdnnf_chunk_input_create(self.max_sequences, C.byref(self.h)))

    @staticmethod
    def _shape(net_or_shape):
        """(first_t, num_t, frame_subsampling) of a ChainNet, or the triple itself"""
        if hasattr(net_or_shape, "num_t_in"):
            return int(net_or_shape.first_t), int(net_or_shape.num_t_in), int(net_or_shape.cfg.frame_subsampling)
        first_t, num_t, fsf = net_or_shape
        return int(first_t), int(num_t), int(fsf)

    @staticmethod
    def plan(frame_subsampling, frames_per_sequence, seq_utt, chunk_begins, frames, ivector_rows=None, ivector_period=10, frame_shift=0):
        """tdnnf_chunk_input_plan (host only, no device, no handle): the table of a minibatch, numpy int32 (sequences, 4) -- the first stacked
        feature row of the sequence's utterance, the utterance's frames, the window start begin * fsf - frame_shift, the stacked i-vector
        row (ivector_rows None with ivector_period > 0: no i-vectors, 0).  Refuses (HipAbiError) what gather refuses of these arguments."""
        import numpy as np
        utt, first = _sequence_chunks(seq_utt, chunk_begins)
        fr = iarr(frames)
        ivr = iarr(ivector_rows) if ivector_rows is not None else (None, None)
        table = np.zeros((max(len(utt[0]), 1), 4), np.int32)
        check(load().tdnnf_chunk_input_plan(int(frame_subsampling), int(frames_per_sequence), len(utt[0]), utt[1], first[1], int(frame_shift), len(fr[0]),
                                            fr[1], ivr[1], int(ivector_period), table.ctypes.data_as(C.c_void_p)))
        return table[:len(utt[0])]

    def gather(self, net_or_shape, frames_per_sequence, seq_utt, chunk_begins, frames, feats, ivector_rows, ivectors, ivector_period, frame_shift=0,
               out=None):
        """tdnnf_chunk_input_gather on the current stream.  net_or_shape: a ChainNet or (first_t, num_t, frame_subsampling); sequence b is the
        output frames [chunk_begins[b], chunk_begins[b] + frames_per_sequence) of utterance seq_utt[b]; frames: the input frames of every
        utterance; feats / ivectors: the utterances' rows stacked, CUDA tensors (ivectors None or of no columns: none; ivector_rows may be
        None for ivector_period <= 0).  out: (feats_out, ivectors_out) to write into, default new tensors.  Returns (feats_out
        [num_t * sequences, feat_dim] t-major, ivectors_out [sequences, ivector_dim] or None) as ChainNet.forward_backward takes them."""
        import torch
        first_t, num_t, fsf = self._shape(net_or_shape)
        utt, first = _sequence_chunks(seq_utt, chunk_begins)
        B = len(utt[0])
        fr = iarr(frames)
        use_iv = ivectors is not None and ivectors.shape[1] > 0
        ivr = iarr(ivector_rows) if ivector_rows is not None else (None, None)
        if out is None:
            out = (torch.empty(num_t * B, feats.shape[1], dtype=torch.float32, device=feats.device),
                   torch.empty(B, ivectors.shape[1], dtype=torch.float32, device=feats.device) if use_iv else None)
        feats_out, ivectors_out = out
        check(load().tdnnf_chunk_input_gather(self.h, first_t, num_t, fsf, int(frames_per_sequence), B, utt[1], first[1], int(frame_shift), len(fr[0]), fr[1],
                                              pmat(feats), ivr[1], pmat(ivectors) if use_iv else None, int(ivector_period), pmat(feats_out),
                                              pmat(ivectors_out) if use_iv else None, stream()))
        return feats_out, (ivectors_out if use_iv else None)

    def gather_stored(self, net_or_shape, frames_per_sequence, seq_utt, chunk_begins, store, ivector_rows, ivectors, ivector_period, frame_shift=0,
                      out=None):
        """tdnnf_chunk_input_gather_stored on the current stream: gather with the features decoded out of `store` (a FeatureStore; include/
        tdnnf_hip.h, "FEATURE STORES").  seq_utt indexes the store's utterances, whose frames are the store's; ivector_rows / ivectors:
        one entry / the rows of every utterance of the store, float, as gather takes them.  Counted in store.info(), not in info()."""
        import torch
        first_t, num_t, fsf = self._shape(net_or_shape)
        utt, first = _sequence_chunks(seq_utt, chunk_begins)
        B = len(utt[0])
        use_iv = ivectors is not None and ivectors.shape[1] > 0
        ivr = iarr(ivector_rows) if ivector_rows is not None else (None, None)
        if out is None:
            out = (torch.empty(num_t * B, store.feat_dim, dtype=torch.float32, device="cuda"),
                   torch.empty(B, ivectors.shape[1], dtype=torch.float32, device="cuda") if use_iv else None)
        feats_out, ivectors_out = out
        check(load().tdnnf_chunk_input_gather_stored(self.h, first_t, num_t, fsf, int(frames_per_sequence), B, utt[1], first[1], int(frame_shift), store.h,
                                                     ivr[1], pmat(ivectors) if use_iv else None, int(ivector_period), pmat(feats_out),
                                                     pmat(ivectors_out) if use_iv else None, stream()))
        return feats_out, (ivectors_out if use_iv else None)

    def info(self):
        """{max_sequences, allocations, gathers, last_form} (tdnnf_chunk_input_info): device and pinned allocations since create, successful
        gathers, the last one's form -- 4: 16-byte loads and stores, 1: a float at a time, 0: none yet."""
        a, b, c, d = C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int()
        check(load().tdnnf_chunk_input_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(max_sequences=a.value, allocations=b.value, gathers=c.value, last_form=d.value)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_chunk_input_destroy(self.h)
            self.h = None


class FeaturePayload(C.Structure):
    """tdnnf_feature_payload: one CompressedMatrix in Kaldi's order, as an archive holds it"""
    _fields_ = [("format", C.c_int), ("min_value", C.c_float), ("range", C.c_float), ("rows", C.c_int), ("cols", C.c_int), ("percentiles", C.c_void_p),
                ("codes", C.c_void_p)]


FEATURE_TOKENS = {1: "CM", 2: "CM2", 3: "CM3"}


def _payload(item, format=None):
    """(FeaturePayload, the arrays it points into) of an item dict {"min", "range", "rows", "cols", "codes"[, "percentiles"][, "format"]}:
    codes uint8 [cols, rows] (format 1, column-major as Kaldi holds them), uint16 [rows, cols] (2) or uint8 [rows, cols] (3); percentiles
    uint16 [cols, 4].  The format is the item's own where it names one, else `format`."""
    import numpy as np
    fmt = int(item.get("format", format if format is not None else 0))
    rows, cols = int(item["rows"]), int(item["cols"])
    codes = np.ascontiguousarray(item["codes"], dtype=np.uint16 if fmt == 2 else np.uint8)
    if codes.size != rows * cols:
        raise HipAbiError(f"an item of {rows} x {cols} with {codes.size} codes")
    pct = None
    if fmt == 1:
        pct = np.ascontiguousarray(item.get("percentiles"), dtype=np.uint16)
        if pct.size != 4 * cols:
            raise HipAbiError(f"an item of {cols} columns with {pct.size} percentiles")
    p = FeaturePayload(fmt, float(item["min"]), float(item["range"]), rows, cols, pct.ctypes.data if pct is not None else None, codes.ctypes.data)
    return p, (codes, pct)


class FeatureStore:
    """Utterances' features kept on the device as Kaldi's CompressedMatrix codes (tdnnf_feature_store; include/tdnnf_hip.h, "FEATURE
    STORES"): one format (1 "CM", 2 "CM2", 3 "CM3") and one feat_dim, capacities fixed and everything allocated at create.  Utterances are
    numbered in append order; ChunkInput.gather_stored and expand decode them on the device, bit for bit egs.Reader's values."""

    def __init__(self, format, feat_dim, max_utterances, max_frames):
        self.h = C.c_void_p()
        self.format, self.feat_dim = int(format), int(feat_dim)
        self.frames = []  # of every utterance, in append order: the library's (tdnnf_feature_store_frames), read back behind every append
        check(load().tdnnf_feature_store_create(self.format, self.feat_dim, int(max_utterances), int(max_frames), C.byref(self.h)))

    def _read_frames(self):
        import numpy as np
        n = self.info()["utterances"]
        frames = np.zeros(max(n, 1), np.int32)
        check(load().tdnnf_feature_store_frames(self.h, 0, n, frames.ctypes.data_as(C.c_void_p)))
        self.frames = [int(f) for f in frames[:n]]

    def append(self, items):
        """tdnnf_feature_store_append: item dicts {"min", "range", "rows", "cols", "codes"[, "percentiles"]} in Kaldi's order, as
        egs.read_feature_archive yields them.  Waits for its copies; a refusal (HipAbiError) leaves the store as it was."""
        payloads = [_payload(item, self.format) for item in items]
        arr = (FeaturePayload * max(len(payloads), 1))(*[p for p, _ in payloads])
        check(load().tdnnf_feature_store_append(self.h, len(payloads), arr))
        self._read_frames()

    def append_float(self, matrices):
        """tdnnf_feature_store_append_float: float matrices [frames, feat_dim] (numpy or torch) compressed on the host by the egs writer's
        rule into the store's format (2 or 3; format 1 is refused)."""
        import numpy as np
        ms = [np.ascontiguousarray(m.detach().cpu().numpy() if hasattr(m, "detach") else m, dtype=np.float32) for m in matrices]
        for i, m in enumerate(ms):
            if m.ndim != 2 or (m.shape[1] != self.feat_dim and m.shape[0] > 0):
                raise HipAbiError(f"feature_store_append_float: item {i} has shape {m.shape}, feat_dim is {self.feat_dim}")
        rows = iarr([m.shape[0] for m in ms])
        stacked = farr(np.concatenate([m.reshape(-1, self.feat_dim) for m in ms]) if ms else np.zeros((0, self.feat_dim), np.float32))
        check(load().tdnnf_feature_store_append_float(self.h, len(ms), rows[1], stacked[1]))
        self._read_frames()

    def expand(self, utts, out=None):
        """tdnnf_feature_store_expand on the current stream: the decoded rows of the listed utterances stacked in list order (any order,
        repeats allowed), a float32 CUDA tensor [sum of their frames, feat_dim] -- out, or a new one."""
        import torch
        u = iarr(utts)
        if out is None:
            rows = sum(self.frames[i] for i in u[0] if 0 <= i < len(self.frames))
            out = torch.empty(rows, self.feat_dim, dtype=torch.float32, device="cuda")
        check(load().tdnnf_feature_store_expand(self.h, len(u[0]), u[1], pmat(out), stream()))
        return out

    def utterances(self, utts, ivectors):
        """The [(feats, ivectors)] list AcousticModel.compute / align / posteriors* take, for the listed utterances: the features are views
        of ONE expand, ivectors[k] goes with utts[k]."""
        import torch
        utts = [int(u) for u in utts]
        if len(ivectors) != len(utts):
            raise HipAbiError(f"{len(utts)} utterances and {len(ivectors)} i-vector matrices")
        feats = torch.split(self.expand(utts), [self.frames[u] for u in utts]) if utts else []
        return list(zip(feats, ivectors))

    def info(self):
        """{format, feat_dim, utterances, frames, device_bytes, reserved_bytes, allocations, gathers, expands, last_form}
        (tdnnf_feature_store_info): device_bytes is the closed form of the header (layout), reserved_bytes the arena of the capacities,
        allocations those since create, last_form 4 (a lane decodes 4 columns: 16-byte stores), 1 (a code at a time) or 0 (none yet)."""
        v = [C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_int()]
        check(load().tdnnf_feature_store_info(self.h, *[C.byref(x) for x in v]))
        keys = ("format", "feat_dim", "utterances", "frames", "device_bytes", "reserved_bytes", "allocations", "gathers", "expands", "last_form")
        return {k: x.value for k, x in zip(keys, v)}

    @staticmethod
    def layout(format, feat_dim, frames):
        """tdnnf_feature_store_layout (host only): (code offsets numpy int64 [utterances + 1], device_bytes) of utterances of these frames."""
        import numpy as np
        fr = iarr(frames)
        offsets, total = np.zeros(len(fr[0]) + 1, np.int64), C.c_longlong()
        check(load().tdnnf_feature_store_layout(int(format), int(feat_dim), len(fr[0]), fr[1], offsets.ctypes.data_as(C.c_void_p), C.byref(total)))
        return offsets, total.value

    @staticmethod
    def pack(format, feat_dim, item):
        """Host only, what an append copies to the device.  item a dict: tdnnf_feature_store_pack -- {"min", "range", "header": float32
        [feat_dim, 4] p0..p3 a column (format 1) or None, "codes": row-major [rows, feat_dim] uint8 or uint16}.  item a float matrix:
        tdnnf_feature_store_compress in `format` -- the same dict with the matrix's (min, range) and codes."""
        import numpy as np
        if isinstance(item, dict):
            p, keep = _payload(item, format)
            if p.format != int(format):
                raise HipAbiError(f"feature_store_pack: item 0 is a payload of format {p.format}, not of format {int(format)}")
            header = np.zeros((int(feat_dim), 4), np.float32) if p.format == 1 else None
            codes = np.zeros((max(p.rows, 0), int(feat_dim)), np.uint16 if p.format == 2 else np.uint8)
            check(load().tdnnf_feature_store_pack(int(feat_dim), C.byref(p), header.ctypes.data_as(C.c_void_p) if header is not None else None,
                                                  codes.ctypes.data_as(C.c_void_p)))
            return dict(min=np.float32(p.min_value), range=np.float32(p.range), header=header, codes=codes)
        m = np.ascontiguousarray(item, dtype=np.float32)
        codes = np.zeros(m.shape, np.uint16 if int(format) == 2 else np.uint8)
        mn, rg = C.c_float(), C.c_float()
        check(load().tdnnf_feature_store_compress(int(format), m.shape[0], m.shape[1] if m.ndim == 2 else 0, m.ctypes.data_as(C.c_void_p), C.byref(mn), C.byref(rg),
                                                  codes.ctypes.data_as(C.c_void_p)))
        return dict(min=np.float32(mn.value), range=np.float32(rg.value), header=None, codes=codes)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.tdnnf_feature_store_destroy(self.h)
            self.h = None
