"""CPU: what the sparse posteriors need no device for.
 * tests/posteriors_sparse_ref.py, the reference the GPU test holds the library to, on hand-written rows whose answers are written out here;
 * infer.write_posterior_archive takes (key, pdf, post, count) items: where no frame was truncated the bytes are those of the dense matrix
   through the old (key, matrix) form -- pure numpy on both sides;
 * the two new C entries refuse a null handle with TDNNF_EINVAL and a message that names the call (the refusals that need a handle are in
   tests/test_gpu_posteriors_sparse.py)."""
import ctypes as C

import numpy as np
import pytest

from tests.posteriors_sparse_ref import sparsify

F = np.float32
PDFS = np.asarray([2, 3, 7, 11, 40, 41], np.int32)


def _one(row, min_post, K):
    pdf, post, count, n = sparsify(np.asarray([row], F), PDFS, min_post, K)
    assert pdf.dtype == np.int32 and post.dtype == F and count.dtype == np.int32 and pdf.shape == post.shape == (1, K)
    return pdf[0].tolist(), post[0].tolist(), int(count[0]), int(n[0])


def test_fewer_candidates_than_slots():
    assert _one([0.5, 0, 0, 0.25, 0, 0], 0.0, 3) == ([2, 11, -1], [0.5, 0.25, 0.0], 2, 2)


def test_as_many_candidates_as_slots():
    assert _one([0.5, 0, 0.125, 0.25, 0, 0], 0.0, 3) == ([2, 7, 11], [0.5, 0.125, 0.25], 3, 3)


def test_one_candidate_more_than_slots_drops_the_least():
    assert _one([0.5, 0, 0.125, 0.25, 0, 0.0625], 0.0, 3) == ([2, 7, 11], [0.5, 0.125, 0.25], 3, 4)
    assert _one([0.0625, 0, 0.125, 0.25, 0, 0.5], 0.0, 3) == ([7, 11, 41], [0.125, 0.25, 0.5], 3, 4)


def test_a_tie_across_the_cutoff_keeps_the_lower_pdfs():
    # 0.5 is in; of the three 0.25s two fit: pdfs 3 and 11, not 40 -- and the pairs come out in pdf order, not value order
    assert _one([0, 0.25, 0.5, 0.25, 0.25, 0.125], 0.0, 3) == ([3, 7, 11], [0.25, 0.5, 0.25], 3, 5)
    assert _one([0.25, 0.25, 0.25, 0.25, 0.25, 0.25], 0.0, 2) == ([2, 3], [0.25, 0.25], 2, 6)


def test_zeros_a_nan_and_a_value_equal_to_the_floor_are_no_candidates():
    assert _one([0.0, np.nan, 0.25, 0.5, -0.5, 0.75], 0.25, 4) == ([11, 41, -1, -1], [0.5, 0.75, 0.0, 0.0], 2, 2)
    assert _one([0.0, np.nan, -0.0, 0.0, -1.0, 0.0], 0.0, 2) == ([-1, -1], [0.0, 0.0], 0, 0)
    assert _one([0.0, np.nan, 0.25, np.inf, 0.5, 0.0], 0.0, 2) == ([11, 40], [np.inf, 0.5], 2, 3)  # (a NaN is not the greatest value either)


def test_one_slot():
    assert _one([0.125, 0.5, 0, 0.5, 0.25, 0], 0.0, 1) == ([3], [0.5], 1, 4)
    assert _one([0, 0, 0, 0, 0.25, 0], 0.0, 1) == ([40], [0.25], 1, 1)
    assert _one([0, 0, 0, 0, 0.25, 0], 0.25, 1) == ([-1], [0.0], 0, 0)


def test_several_frames_and_an_empty_block():
    block = np.asarray([[0.5, 0, 0, 0.5, 0, 0], [0, 0, 0, 0, 0, 0], [0.1, 0.2, 0.3, 0.2, 0.1, 0.1]], F)
    pdf, post, count, n = sparsify(block, PDFS, 0.0, 2)
    assert pdf.tolist() == [[2, 11], [-1, -1], [3, 7]] and count.tolist() == [2, 0, 2] and n.tolist() == [2, 0, 6]
    assert np.array_equal(post, np.asarray([[0.5, 0.5], [0, 0], [0.2, 0.3]], F))
    pdf, post, count, n = sparsify(np.zeros((0, 6), F), PDFS, 0.0, 4)
    assert pdf.shape == post.shape == (0, 4) and count.shape == n.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------------- the archive
def _items(K):
    """[(key, column list, compact block)] with entries at, below and above the floors tried, a frame of zeros, a zero-frame utterance, one
    column, the first and the last pdf; no frame has more than K entries above 0"""
    rng = np.random.default_rng(3)
    items = []
    for key, ids, T in (("a", [0, 3, 4, 17, 49], 6), ("b", [7], 3), ("none", [2, 9], 0), ("c", list(range(10, 40)), 4)):
        post = rng.random((T, len(ids))).astype(F)
        post[post < 0.6] = 0.0
        if T > 1:
            post[1] = 0.0
        if T > 2:
            post[2, 0] = F(0.25)  # an entry equal to the positive floor: dropped
        assert (post > 0).sum(1).max(initial=0) <= K
        items.append((key, np.asarray(ids, np.int32), post))
    return items


@pytest.mark.parametrize("call_floor,min_post", [(0.0, 0.0), (0.0, 0.25), (0.25, 0.25), (0.25, 0.7)])
def test_archive_bytes_equal_the_dense_form(pkg, tmp_path, call_floor, min_post):
    """the writer's floor is at least the call's and no frame is truncated: byte-equal to the dense matrix's file"""
    P, K = 50, 32
    items = _items(K)
    dense, sparse = [], []
    for key, ids, block in items:
        m = np.zeros((len(block), P), F)
        m[:, ids] = block
        dense.append((key, m))
        pdf, post, count, n = sparsify(block, ids, call_floor, K)
        assert (n <= K).all()
        sparse.append((key, pdf, post, count))
    old, new = tmp_path / "dense.ark", tmp_path / "sparse.ark"
    pkg.infer.write_posterior_archive(old, dense, min_post=min_post)
    pkg.infer.write_posterior_archive(new, sparse, min_post=min_post)
    assert old.read_bytes() == new.read_bytes() and len(old.read_bytes()) > 100
    back = pkg.infer.read_posterior_archive(new)
    assert list(back) == ["a", "b", "none", "c"] and back["none"] == [] and back["a"][1] == [] and len(back["a"]) == 6
    # the forms mixed in one archive
    mixed = tmp_path / "mixed.ark"
    pkg.infer.write_posterior_archive(mixed, [sparse[0], dense[1], items[2], sparse[3]], min_post=min_post)
    assert mixed.read_bytes() == old.read_bytes()


def test_archive_writes_only_the_counted_slots(pkg, tmp_path):
    """slots at and behind count[t] are not read, whatever they hold; a truncated frame writes its K pairs"""
    pdf = np.asarray([[3, 9, 5], [4, -1, -1]], np.int32)
    post = np.asarray([[0.5, 0.25, 0.75], [0.125, 0.0, 0.0]], F)
    path = tmp_path / "x.ark"
    pkg.infer.write_posterior_archive(path, [("k", pdf, post, np.asarray([2, 1], np.int32))], min_post=0.0)
    assert pkg.infer.read_posterior_archive(path) == {"k": [[(3, 0.5), (9, 0.25)], [(4, 0.125)]]}
    pkg.infer.write_posterior_archive(path, [("k", pdf, post, np.asarray([3, 0], np.int32))], min_post=0.25)
    assert pkg.infer.read_posterior_archive(path) == {"k": [[(3, 0.5), (5, 0.75)], []]}


def test_entries_refuse_null_arguments_by_name(pkg):
    lib = pkg.hipabi.load()
    assert {"tdnnf_align_posteriors_sparse", "tdnnf_align_posteriors_sparse_workspace_bytes"} <= set(pkg.hipabi.declared_symbols())
    frames = (C.c_int * 2)(3, 4)
    assert lib.tdnnf_align_posteriors_sparse_workspace_bytes(None, 2, None, frames, 16) == 0
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_sparse: ")
    assert lib.tdnnf_align_posteriors_sparse_workspace_bytes(None, 2, None, frames, 65) == 0
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_sparse: ") and b"max_per_frame" in lib.tdnnf_last_error()
    y = pkg.hipabi.Mat(None, 0, 0, 0)
    assert lib.tdnnf_align_posteriors_sparse(None, 2, None, frames, frames, 1, C.byref(y), 1.0, 1.0, 0.01, 16, None, None, None, None, None, 0, None) == 1
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_sparse: ")
