"""CPU: what the labelled alignment entries (include/tdnnf_hip.h: tdnnf_align_graphs_create_labelled, tdnnf_align_best_path_labels,
tdnnf_align_label_posteriors_*) refuse before anything touches a device, and the labels synth.make_alignment_graph gives.
(An unlabelled HANDLE needs a device to exist: tests/test_gpu_align_labels.py makes one and sees every label entry refuse it.  Here the
same check, align_need_labels, turns away the handle that is not there.)"""
import ctypes as C

import numpy as np

F = np.float32
NEW = ["tdnnf_align_graphs_create_labelled", "tdnnf_align_graphs_labels", "tdnnf_align_best_path_labels", "tdnnf_align_label_posteriors_compact_layout",
       "tdnnf_align_label_posteriors_compact", "tdnnf_align_label_posteriors_sparse_workspace_bytes", "tdnnf_align_label_posteriors_sparse"]


def test_symbols_are_declared_and_exported(pkg):
    assert set(NEW) <= set(pkg.hipabi.declared_symbols())
    lib = pkg.hipabi.load()
    assert all(hasattr(lib, s) for s in NEW)


def _create(pkg, label, num_labels):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    g = pkg.synth.make_alignment_graph([1, 2, 3], num_pdfs=5)
    A = len(g["src"])
    arrays = [abi.iarr([0, g["S"]]), abi.iarr([0, A]), abi.iarr(g["src"]), abi.iarr(g["dst"]), abi.iarr(g["pdf"]), abi.farr(g["logprob"]),
              abi.farr(g["init"]), abi.farr(g["final"])]
    lab = abi.iarr(label(A)) if label is not None else (None, None)
    h = C.c_void_p()
    rc = lib.tdnnf_align_graphs_create_labelled(1, 5, *[a[1] for a in arrays], lab[1], num_labels, C.byref(h))
    return rc, lib.tdnnf_last_error(), h


def test_a_label_outside_the_range_is_refused_by_arc(pkg):
    for bad, at in ((7, 4), (-1, 0), (8, 5)):
        def label(A, bad=bad, at=at):
            v = np.arange(A) % 7
            v[at] = bad
            return v
        rc, err, h = _create(pkg, label, 7)
        assert rc == 1 and not h.value and err.startswith(b"align_graphs_create_labelled: ")
        assert b"arc %d " % at in err and b"label %d " % bad in err and b"[0, 7)" in err, err
    rc, err, h = _create(pkg, None, 7)
    assert rc == 1 and err.startswith(b"align_graphs_create_labelled: ") and b"arc_label" in err
    rc, err, h = _create(pkg, lambda A: np.zeros(A), 0)
    assert rc == 1 and err.startswith(b"align_graphs_create_labelled: ") and b"num_labels" in err
    # the unlabelled entry's own refusals keep their name
    lib = pkg.hipabi.load()
    assert lib.tdnnf_align_graphs_create(0, 5, None, None, None, None, None, None, None, None, None) == 1
    assert lib.tdnnf_last_error().startswith(b"align_graphs_create: ")


def test_label_entries_refuse_a_handle_without_labels_by_name(pkg):
    lib = pkg.hipabi.load()
    frames = (C.c_int * 2)(3, 4)
    y = pkg.hipabi.Mat(None, 0, 0, 0)
    n = C.c_int()
    named = lambda who: lib.tdnnf_last_error().startswith(who + b": ")
    assert lib.tdnnf_align_graphs_labels(None, 0, C.byref(n), None) == 1 and named(b"align_graphs_labels")
    assert lib.tdnnf_align_label_posteriors_compact_layout(None, 2, None, frames, None, None) == 1 and named(b"align_label_posteriors_compact_layout")
    assert lib.tdnnf_align_label_posteriors_compact(None, 2, None, frames, frames, 1, C.byref(y), 1.0, 1.0, None, 0, None, None, 0, None) == 1
    assert named(b"align_label_posteriors_compact")
    assert lib.tdnnf_align_best_path_labels(None, 2, None, frames, frames, 1, C.byref(y), 1.0, None, None, None, None, None, None, 0, None) == 1
    assert named(b"align_best_path_labels")
    assert lib.tdnnf_align_label_posteriors_sparse_workspace_bytes(None, 2, None, frames, 16) == 0 and named(b"align_label_posteriors_sparse")
    assert lib.tdnnf_align_label_posteriors_sparse(None, 2, None, frames, frames, 1, C.byref(y), 1.0, 1.0, 0.01, 16, None, None, None, None, None, 0, None) == 1
    assert named(b"align_label_posteriors_sparse")


def test_max_per_frame_outside_1_to_64_is_refused(pkg):
    """(checked on the GPU with a labelled handle as well: tests/test_gpu_align_labels.py)"""
    lib = pkg.hipabi.load()
    frames = (C.c_int * 2)(3, 4)
    y = pkg.hipabi.Mat(None, 0, 0, 0)
    for K in (0, 65, -3):
        assert lib.tdnnf_align_label_posteriors_sparse_workspace_bytes(None, 2, None, frames, K) == 0
        assert lib.tdnnf_last_error().startswith(b"align_label_posteriors_sparse: ")
        assert lib.tdnnf_align_label_posteriors_sparse(None, 2, None, frames, frames, 1, C.byref(y), 1.0, 1.0, 0.01, K, None, None, None, None, None, 0, None) == 1
        assert lib.tdnnf_last_error().startswith(b"align_label_posteriors_sparse: ")


def test_wrapper_wants_labels_on_all_graphs_or_none(pkg):
    import pytest
    g = pkg.synth.make_alignment_graph([1, 2], num_pdfs=5)
    gl = pkg.synth.make_alignment_graph([1, 2], num_pdfs=5, labels="unit")
    with pytest.raises(pkg.hipabi.HipAbiError, match="label"):
        pkg.hipabi.AlignGraphs([g, gl])
    with pytest.raises(pkg.hipabi.HipAbiError, match="num_labels"):
        pkg.hipabi.AlignGraphs([g], num_labels=3)
    assert gl["label"].tolist()[:3] == [0, 0, 1]  # (arcs by (source, destination): start -> unit 0, its loop, unit 0 -> unit 1)
    with pytest.raises(pkg.hipabi.HipAbiError, match=r"align_graphs_create_labelled: arc 2 carries label 1 outside \[0, 1\)"):
        pkg.hipabi.AlignGraphs([gl], num_labels=1)


def test_synth_labels(pkg):
    kw = dict(optional=[1], alternatives={2: [7, 8]}, num_pdfs=12, seed=3)
    seq = [4, 5, 6, 9]
    plain = pkg.synth.make_alignment_graph(seq, **kw)
    unit = pkg.synth.make_alignment_graph(seq, labels="unit", **kw)
    arc = pkg.synth.make_alignment_graph(seq, labels="arc", **kw)
    assert "label" not in plain and "L" not in plain
    for g in (unit, arc):  # the graph itself is what it is without labels
        assert all(np.array_equal(g[k], plain[k], equal_nan=True) for k in plain)
    A = len(plain["src"])
    assert arc["label"].tolist() == list(range(A)) and arc["L"] == A and arc["label"].dtype == np.int32
    # a unit's label: shared by the arcs that enter it and its loop, and it names one pdf
    assert unit["L"] == 6 and unit["label"].dtype == np.int32 and np.array_equal(unit["label"], unit["dst"] - 1)
    assert sorted(set(unit["label"].tolist())) == list(range(6))
    units_pdf = [4, 5, 6, 9, 7, 8]
    assert all(units_pdf[l] == p for l, p in zip(unit["label"], unit["pdf"]))
    loops = unit["src"] == unit["dst"]
    assert loops.sum() == 6 and all((unit["label"] == l).sum() >= 2 for l in range(6))
