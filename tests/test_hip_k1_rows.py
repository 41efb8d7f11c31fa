"""K1's row build (csrc/grid.hip: k_row_count, k_cell_scan, k_row_place, k_row_settle) against the counting build and the
radix build: the cell-sorted order, the layer table and every list of a self search are the same bit for bit, whichever of the
three ordered the grid.

`SF_K1_ROWS=1` takes the row build wherever there is a point to order, `SF_K1_ROWS=0` never, `SF_K1_RADIX=1` forces the sort;
all are read at every build.  The row build keeps the counting build's four timer names (bench.py and the recorded launch
tables know them), so the launch names tell the sort from the other two, not the other two apart: what separates those here is
the switch itself."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import config1_cloud, family, synth_cloud

pytestmark = pytest.mark.gpu

SWITCHES = ("SF_K1_ROWS", "SF_K1_RADIX")


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


@contextmanager
def switches(**env):
    """The two build switches set to `env` (a missing one unset) for the duration, then put back."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def launches(eng, fn):
    eng.sync()
    eng.profile_reset()
    eng.profile(True)
    try:
        out = fn()
        eng.sync()
    finally:
        eng.profile(False)
    return out, {k for k, v in eng.profile_report().items() if v[0]}


def grid_and_lists(eng, p, r, block):
    """(launch names, [order, layer table, list offsets, list entries]) of one build + self search of p at radius r."""
    cloud = eng.cloud(p)
    try:
        lo, hi = (0, cloud.n) if block is None else block

        def go():
            if block is None:
                cloud.build_grid(r)
            else:
                cloud.build_grid(r, block=block, reach=1)
            return cloud.radius_search_self(r, lo, hi) if hi > lo else None

        nb, names = launches(eng, go)
        out = [cloud.perm()[lo:hi], cloud.layer_table()]
        if nb is not None:
            out += list(nb.export())
            nb.free()
        return names, out
    finally:
        cloud.free()


def three_ways(eng, p, r, block=None):
    """Row build, whatever the older rules take, and the radix build: equal results, and the launches of the build asked for."""
    with switches(SF_K1_ROWS="1"):
        n_rows, rows = grid_and_lists(eng, p, r, block)
    with switches(SF_K1_ROWS="0"):
        n_old, old = grid_and_lists(eng, p, r, block)
    with switches(SF_K1_RADIX="1"):
        n_radix, radix = grid_and_lists(eng, p, r, block)
    populated = block is None or block[1] > block[0]
    if populated:
        assert "k1_cell_settle" in n_rows and "k1_radix_sort" not in n_rows, n_rows
        assert ("k1_cell_settle" in n_old) != ("k1_radix_sort" in n_old), n_old
        assert "k1_radix_sort" in n_radix and "k1_cell_settle" not in n_radix, n_radix
    else:  # (nothing to order: only the cell table is written)
        for names in (n_rows, n_old, n_radix):
            assert "k1_cell_settle" not in names and "k1_radix_sort" not in names, names
    assert len(rows) == len(old) == len(radix)
    for x, y, z in zip(rows, old, radix):
        assert x.shape == z.shape and np.array_equal(x, z)
        assert np.array_equal(y, z)
    return rows


def clustered(n, seed=4):
    return family("clustered", n, np.random.default_rng(seed))[0]


# ---- (a) the common path, whole and block --------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [None, (12000, 31000)])
def test_uniform_cloud_whole_and_block(eng, block):
    """400 rows of ~100 points: every row sorted in LDS, tiles of one or two z-layers inside the LDS window."""
    p, _, _ = synth_cloud(40000, 5)
    order = three_ways(eng, p, 0.05, block)[0]
    assert order.size == (40000 if block is None else 19000)


# ---- (b) mostly empty rows and cells ----------------------------------------------------------------------------------------
def test_surface_cloud(eng):
    """A noisy sphere: most rows hold nothing or a few points at the two places where they cross the surface (the empty-row fill
    of the cell table, runs of empty cells inside a row filled by whole waves)."""
    p, _ = config1_cloud(40000, 5)
    three_ways(eng, p, 0.04)


# ---- (c) many entries per cell ------------------------------------------------------------------------------------------------
def test_duplicated_points_keep_index_order_inside_a_cell(eng):
    """Every position occurs eight times: eight equal cells per key group, ordered by the internal index alone."""
    q, _, _ = synth_cloud(5000, 5)
    p = np.concatenate([q] * 8)[np.random.default_rng(1).permutation(40000)]
    three_ways(eng, p, 0.06)


# ---- (d) one row longer than the LDS holds --------------------------------------------------------------------------------
def test_one_long_row(eng):
    """40 000 points on a line along x: one row of 40 000 keys (ten times what is sorted in LDS: the same network over global
    memory) and 8 000 fine cells in it."""
    x = np.random.default_rng(2).random(40000, dtype=np.float32).astype(np.float64)
    p = np.column_stack([x, np.full(40000, 0.25), np.full(40000, 0.75)])
    three_ways(eng, p, 0.002)


@pytest.mark.parametrize("n", [1500, 3000])
def test_one_row_sorted_by_the_network_in_lds(eng, n):
    """The same line with fewer points: 8 000 cells are more than the counting form of the settle holds counters for (1 500
    keys), and 3 000 keys more than it holds keys; both fit the network's 4 096 keys in LDS."""
    x = np.random.default_rng(2).random(n, dtype=np.float32).astype(np.float64)
    p = np.column_stack([x, np.full(n, 0.25), np.full(n, 0.75)])
    three_ways(eng, p, 0.002)


# ---- (e) rows outside the LDS window --------------------------------------------------------------------------------------
def test_tall_sparse_box_leaves_the_window(eng):
    """3 000 points in a box 250 cells tall and 13 x 13 cells wide: the one tile of count and place spans every layer, 3 250
    rows against a window of 1 024, so two thirds of the points take the global atomic of their own."""
    p = np.random.default_rng(3).random((3000, 3), dtype=np.float32).astype(np.float64) * np.array([0.05, 0.05, 1.0])
    three_ways(eng, p, 0.004)


# ---- (f) coordinates on cell edges and on the upper faces ---------------------------------------------------------------------
def test_points_on_cell_edges_and_upper_faces(eng):
    """Coordinates k * edge for the grid's own edge (r * (1 + 2^-20)), their two floating-point neighbours, and the bounding
    box's upper faces (k = 8, where sf_cell_coord's clamp holds the last cell): the row build forms (cx, row) as the other
    two form the cell id."""
    r = 0.125
    g = np.arange(9) * (r * (1.0 + 2.0 ** -20))
    vals = np.concatenate([g, np.nextafter(g, np.inf)[:-1], np.nextafter(g, -np.inf)[1:]])
    corners = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(6)
    p = np.concatenate([corners, vals[rng.integers(0, vals.size, (6000, 3))]])
    three_ways(eng, p[rng.permutation(p.shape[0])], r)


# ---- (g) degenerate sizes -------------------------------------------------------------------------------------------------------
def test_one_point(eng):
    order, _, off, idx = three_ways(eng, np.array([[0.25, 0.5, 0.75]]), 0.1)
    assert order.tolist() == [0] and off.tolist() == [0, 1] and idx.tolist() == [0]


def test_two_identical_points(eng):
    order, _, off, idx = three_ways(eng, np.array([[0.25, 0.5, 0.75]] * 2), 0.1)
    assert order.tolist() == [0, 1] and off.tolist() == [0, 2, 4] and idx.tolist() == [0, 1, 0, 1]


def test_empty_block(eng):
    p, _, _ = synth_cloud(500, 9)
    out = three_ways(eng, p, 0.2, (100, 100))
    assert out[0].size == 0


# ---- (h) the host's rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [None, (12000, 31000)])
def test_unset_switch_takes_the_row_build_for_well_filled_rows(eng, block):
    """Case (a) with no switch set: 400 rows of ~100 points pass the rule (a mean of 32 .. 1 024 points per row), and the
    result is the forced row build's."""
    p, _, _ = synth_cloud(40000, 5)
    with switches():
        names, got = grid_and_lists(eng, p, 0.05, block)
    assert "k1_cell_settle" in names and "k1_radix_sort" not in names, names
    with switches(SF_K1_ROWS="1"):
        _, want = grid_and_lists(eng, p, 0.05, block)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_unset_switch_leaves_a_sparse_grid_on_the_radix_sort(eng):
    """Six blobs in a sparse background at r = 0.02: 2 500 rows of 16 points on average, below the rule's 32, and 8·10⁶ cells
    for 40 000 points: the radix sort, as before."""
    with switches():
        names, _ = grid_and_lists(eng, clustered(40000), 0.02, None)
    assert "k1_radix_sort" in names and "k1_cell_settle" not in names, names
