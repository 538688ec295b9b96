"""CPU: what the compact posteriors need no device for.
 * infer.write_posterior_archive takes (key, pdf_ids, post) items: the bytes are those of the equivalent dense matrix through the old
   (key, matrix) form -- pure numpy on both sides.
 * the three new C entries refuse bad arguments with TDNNF_EINVAL and a message that names the call (as tests/test_abi_load.py checks the
   boundary: the library loads without a GPU; a handle cannot be created without one, so these are the null-handle cases -- the refusals
   that need a handle are in tests/test_gpu_posteriors_compact.py)."""
import ctypes as C

import numpy as np
import pytest

F = np.float32


def _items(P=50):
    """[(key, pdf_ids, post)]: entries at, below and above the thresholds tried, a frame of zeros, a zero-frame utterance, one column,
    the first and the last pdf"""
    rng = np.random.default_rng(3)
    items = []
    for key, ids, T in (("a", [0, 3, 4, 17, 49], 6), ("b", [7], 3), ("none", [2, 9], 0), ("c", list(range(10, 40)), 4)):
        post = rng.random((T, len(ids))).astype(F)
        post[post < 0.3] = 0.0  # exact zeros, as the pdfs of an unreachable arc get
        if T > 1:
            post[1] = 0.0  # a frame without a surviving entry at any threshold
        if T > 2:
            post[2, 0] = F(0.25)  # an entry equal to the positive threshold: dropped (post <= min_post)
        items.append((key, np.asarray(ids, np.int32), post))
    return items


def _dense(ids, post, P):
    m = np.zeros((post.shape[0], P), F)
    m[:, ids] = post
    return m


@pytest.mark.parametrize("min_post", [0.0, 0.25])
def test_archive_bytes_equal_the_dense_form(pkg, tmp_path, min_post):
    P = 50
    items = _items(P)
    old, new = tmp_path / "dense.ark", tmp_path / "compact.ark"
    pkg.infer.write_posterior_archive(old, [(k, _dense(ids, post, P)) for k, ids, post in items], min_post=min_post)
    pkg.infer.write_posterior_archive(new, items, min_post=min_post)
    assert old.read_bytes() == new.read_bytes() and len(old.read_bytes()) > 100
    back = pkg.infer.read_posterior_archive(new)
    assert list(back) == ["a", "b", "none", "c"] and back["none"] == [] and back["a"][1] == [] and len(back["a"]) == 6
    for k, ids, post in items:
        for t, pairs in enumerate(back[k]):
            keep = post[t] > min_post
            assert [q for q, _ in pairs] == ids[keep].tolist() and np.array_equal(np.asarray([v for _, v in pairs], F), post[t][keep])
    # the two forms mixed in one archive, and ids given as a list
    mixed = tmp_path / "mixed.ark"
    pkg.infer.write_posterior_archive(mixed, [items[0], (items[1][0], _dense(items[1][1], items[1][2], P)), (items[2][0], items[2][1].tolist(), items[2][2]),
                                              items[3]], min_post=min_post)
    assert mixed.read_bytes() == old.read_bytes()


def test_archive_refuses_a_column_list_that_does_not_fit(pkg, tmp_path):
    post = np.ones((2, 3), F)
    for ids in ([1, 2], [1, 3, 2], [4, 4, 5]):  # too short, not ascending, not distinct
        with pytest.raises(AssertionError):
            pkg.infer.write_posterior_archive(tmp_path / "x.ark", [("k", ids, post)])


def test_entries_refuse_null_arguments_by_name(pkg):
    lib = pkg.hipabi.load()
    n, elems = C.c_int(-7), C.c_longlong(-7)
    frames = (C.c_int * 2)(3, 4)
    assert lib.tdnnf_align_graphs_pdfs(None, 0, C.byref(n), None) == 1
    assert lib.tdnnf_last_error().startswith(b"align_graphs_pdfs: ")
    assert lib.tdnnf_align_posteriors_compact_layout(None, 2, None, frames, C.byref(elems), None) == 1
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_compact_layout: ")
    y = pkg.hipabi.Mat(None, 0, 0, 0)
    assert lib.tdnnf_align_posteriors_compact(None, 2, None, frames, frames, 1, C.byref(y), 1.0, 1.0, None, 0, None, None, 0, None) == 1
    assert lib.tdnnf_last_error().startswith(b"align_posteriors_compact: ")
    assert n.value == -7 and elems.value == -7  # nothing was written
