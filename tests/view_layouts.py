"""Sub-matrix views for the -m gpu tests: a 2-D array placed inside a larger, guarded parent allocation the way a Kaldi
CuSubMatrix sits in its parent (include/tdnnf_hip.h: a tdnnf_mat is any device pointer with any stride >= cols).

Every cell of the parent outside the view is a guard cell.  Operands a call only reads get NaN guards (a pass that folds a pad
column into a reduction shows up in the result); operands a call writes get one fixed bit pattern, compared bitwise afterwards.
There are at least GUARD_COLS guard cells in front of and behind every row and `guard_rows` whole rows above and below, so that
a 16-byte access that overruns a row lands in a guard cell, never outside the allocation.

The arithmetic (view_geometry, vector_geometry) is free of torch and has a CPU test (tests/test_view_layouts.py)."""
from collections import namedtuple

import numpy as np

GUARD_COLS = 4
LAYOUTS = ("dense", "pitched", "odd-stride", "off1", "off2", "off1-odd")
# name -> (base offset from 16-byte alignment in floats, stride class).  "dense" has stride == cols: row guards only.
_CLASSES = {"dense": (0, "dense"), "pitched": (0, "mult4"), "odd-stride": (0, "odd"), "off1": (1, "mult4"), "off2": (2, "mult4"),
            "off1-odd": (1, "odd")}
READ_GUARD_BITS = 0x7FC00000       # quiet NaN
WRITE_GUARD_BITS = 0x4B3C614E      # 12345678.0f
_SLACK = 8                          # guard floats behind the last guard row

Geometry = namedtuple("Geometry", "stride offset size left right base_mod")
VecGeometry = namedtuple("VecGeometry", "offset size base_mod")


def view_geometry(rows, cols, layout, guard_rows=2):
    """Where a rows x cols view lies in a flat parent of `size` floats whose first float is 16-byte aligned: element (r, c) is
    parent[offset + r * stride + c].  left / right: guard cells in front of / behind each row inside the stride; base_mod: the
    offset of the view's first element from 16-byte alignment, in floats.  layout: one of LAYOUTS, or ("range", parent_cols,
    first_col): the column range a dim-range-node cuts out of a parent_cols-wide matrix (stride and base as they come)."""
    assert rows >= 1 and cols >= 1 and guard_rows >= 1
    if isinstance(layout, tuple):
        kind, parent_cols, first_col = layout
        assert kind == "range" and first_col >= 0 and first_col + cols <= parent_cols
        stride, left = parent_cols, first_col
        lead = 0
    else:
        base_mod, cls = _CLASSES[layout]
        if cls == "dense":
            stride, left = cols, 0
        else:
            left = GUARD_COLS
            stride = (cols + 3) // 4 * 4 + 2 * GUARD_COLS  # a multiple of 4 with >= GUARD_COLS cells behind the row
            if cls == "odd":
                stride += 1
        lead = (base_mod - (guard_rows * stride + left)) % 4  # floats in front of the first guard row: they set the base's alignment class
    offset = lead + guard_rows * stride + left
    size = lead + (rows + 2 * guard_rows) * stride + _SLACK
    return Geometry(stride, offset, size, left, stride - left - cols, offset % 4)


def vector_geometry(n, shift=0):
    """A vector of n floats `shift` floats behind a 16-byte-aligned address (shift 0: aligned; 1: only 4-byte aligned; K: the
    bias behind K architecture logits), GUARD_COLS or more guard floats on both sides."""
    assert n >= 1 and shift >= 0
    offset = 2 * GUARD_COLS + shift
    return VecGeometry(offset, offset + n + 2 * GUARD_COLS, offset % 4)


def _guarded(flat_values, index, size, writes):
    """(parent, check_guards) for a flat float32 CUDA parent of `size` floats holding flat_values at the int64 positions `index`."""
    import torch
    bits = WRITE_GUARD_BITS if writes else READ_GUARD_BITS
    parent = torch.full((size,), bits, dtype=torch.int32, device="cuda").view(torch.float32)
    assert parent.data_ptr() % 16 == 0
    idx = torch.from_numpy(index).cuda()
    parent[idx] = torch.from_numpy(np.ascontiguousarray(flat_values, dtype=np.float32)).cuda()
    guard = torch.ones(size, dtype=torch.bool, device="cuda")
    guard[idx] = False

    def check_guards():
        torch.cuda.synchronize()
        bad = (parent.view(torch.int32) != bits) & guard
        assert not bool(bad.any()), "guard cells overwritten at parent offsets %s" % bad.nonzero().flatten()[:8].tolist()

    return parent, check_guards


def laid_out(array, layout, guard_rows=2, writes=False):
    """Device copy of a 2-D float32 array as a view in the given layout: (view, parent, check_guards).  writes: the call under
    test writes this operand (its guards hold the fixed pattern instead of NaN)."""
    import torch
    a = np.ascontiguousarray(array, dtype=np.float32)
    assert a.ndim == 2
    rows, cols = a.shape
    g = view_geometry(rows, cols, layout, guard_rows)
    index = (g.offset + np.arange(rows, dtype=np.int64)[:, None] * g.stride + np.arange(cols, dtype=np.int64)[None, :]).reshape(-1)
    parent, check = _guarded(a.reshape(-1), index, g.size, writes)
    view = torch.as_strided(parent, (rows, cols), (g.stride, 1), g.offset)
    # the view really has the alignment class its name claims: a test cannot silently land on the aligned path
    assert view.stride(0) == g.stride and view.data_ptr() == parent.data_ptr() + 4 * g.offset
    if not isinstance(layout, tuple):
        base_mod, cls = _CLASSES[layout]
        assert view.data_ptr() % 16 == 4 * base_mod, (layout, view.data_ptr() % 16)
        assert {"dense": g.stride == cols, "mult4": g.stride % 4 == 0 and g.stride > cols, "odd": g.stride % 2 == 1 and g.stride > cols}[cls], (layout, g)
    return view, parent, check


def laid_out_vec(array, shift=0, writes=False):
    """The same for a raw float vector (bias, memo, scale / offset, coefficients): (view, parent, check_guards); the view starts
    `shift` floats behind a 16-byte-aligned address.  A 2-D array is laid out as its dense rows (a 5 x D memo, a mask)."""
    import torch
    a = np.ascontiguousarray(array, dtype=np.float32).reshape(-1)
    g = vector_geometry(a.size, shift)
    parent, check = _guarded(a, g.offset + np.arange(a.size, dtype=np.int64), g.size, writes)
    view = parent[g.offset:g.offset + a.size]
    assert view.data_ptr() % 16 == 4 * (shift % 4), (shift, view.data_ptr() % 16)
    return view, parent, check
