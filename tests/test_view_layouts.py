"""The layout arithmetic of tests/view_layouts.py (no GPU, no torch): every layout has the property its name claims, the guards
are at least GUARD_COLS wide on both sides of a row and guard_rows rows deep, and the view stays inside its parent."""
import numpy as np
import pytest

from tests.view_layouts import GUARD_COLS, LAYOUTS, vector_geometry, view_geometry

SHAPES = [(1, 1), (1, 8), (5, 3), (261, 260), (261, 262), (261, 261), (17, 6034), (5, 8196), (270, 25), (9, 2)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("guard_rows", [1, 2, 3])
def test_every_layout_has_its_property(layout, guard_rows):
    for rows, cols in SHAPES:
        g = view_geometry(rows, cols, layout, guard_rows)
        assert g.stride >= cols and g.left + cols + g.right == g.stride
        assert g.base_mod == g.offset % 4 == {"dense": 0, "pitched": 0, "odd-stride": 0, "off1": 1, "off2": 2, "off1-odd": 1}[layout]
        if layout == "dense":
            assert g.stride == cols and g.left == g.right == 0
        else:
            assert g.stride > cols and g.left >= GUARD_COLS and g.right >= GUARD_COLS
            assert (g.stride % 2 == 1) if layout in ("odd-stride", "off1-odd") else (g.stride % 4 == 0)
        # guard_rows whole rows above and below, and a float4 that starts at the last element of the last row stays inside
        first, last = g.offset, g.offset + (rows - 1) * g.stride + cols - 1
        assert first - g.left >= guard_rows * g.stride and first >= 0
        assert last + g.right + guard_rows * g.stride < g.size and last + 4 <= g.size
        # view cells and guard cells partition the parent
        cells = np.zeros(g.size, np.int32)
        idx = g.offset + np.arange(rows)[:, None] * g.stride + np.arange(cols)[None, :]
        np.add.at(cells, idx.reshape(-1), 1)
        assert cells.max() == 1 and cells.sum() == rows * cols
        if layout != "dense":  # the run of guard cells between two rows takes a 16-byte overrun from either side
            gaps = np.diff(np.flatnonzero(cells)) - 1
            assert (gaps[gaps > 0] >= 2 * GUARD_COLS).all()


def test_column_ranges_of_a_parent_matrix():
    for parent_cols, first, cols in [(240, 25, 25), (240, 50, 30), (8, 0, 1), (8, 7, 1)]:
        g = view_geometry(261, cols, ("range", parent_cols, first))
        assert g.stride == parent_cols and g.left == first and g.right == parent_cols - first - cols
        assert g.base_mod == first % 4  # two guard rows of an even number of columns in front: the base is parent + first_col
        assert g.offset + 260 * g.stride + cols + 4 <= g.size


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 7])
def test_vectors(shift):
    for n in (1, 3, 132, 5 * 261):
        g = vector_geometry(n, shift)
        assert g.base_mod == shift % 4 == g.offset % 4
        assert g.offset >= GUARD_COLS and g.size - (g.offset + n) >= GUARD_COLS
