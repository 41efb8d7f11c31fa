"""K2's shared sweep: a wave whose four queries have the same stencil rows sweeps the UNION of their windows once and tests every
candidate against all four (search.hip, `k_radius<2, false, true>`); a wave whose queries differ in their stencil bounds, or with
fewer than four queries, sweeps query by query as before.

Every case searches one cloud twice, each time on a fresh upload: with the shared sweep and with SF_K2_SHARED=0 (the per-query sweep
everywhere).  `count`, `offset` and the stored lists (cell-sorted positions, in the order the sweep wrote them) must be equal word for
word (the offsets of refilled lists: relative to their area's start, see check()), and both must equal a brute-force list of the same unfused float64 expression, `(dx*dx + dy*dy) + dz*dz <= r*r`, in ascending
position.  Query sets are 16 384 .. 20 000 points: the single sweep into slots serves sets of at least 16 384.
"""
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


def search_raw(eng, p, r, before=None):
    """Self search of all points at radius r on a fresh upload -> (count, offset, idx, perm).  `before`: (begin, end) of a self
    search made first on the same cloud (its list statistics become the capacity hint of the second)."""
    cloud = eng.cloud(p)
    try:
        if before is not None:
            cloud.radius_search_self(r, *before).free()
        nb = cloud.radius_search_self(r)
        try:
            cnt, off, idx = nb.export_raw()
        finally:
            nb.free()
        return cnt, off, idx, cloud.perm()
    finally:
        cloud.free()


def brute_force(ps, r, queries):
    """Lists of the given queries (positions into the cell-sorted points ps), ascending position."""
    r2 = r * r
    out = []
    for q in queries:
        d = ps - ps[q]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out.append(np.flatnonzero(d2 <= r2).astype(np.int32))
    return out


def check(eng, monkeypatch, p, r, before=None, every=11):
    """Shared sweep == per-query sweep, word for word; both == brute force for every `every`-th query, the first and last 40
    and the queries with the shortest and the longest lists.  Returns (count, offset, lists' start in idx, perm)."""
    monkeypatch.delenv("SF_K2_SHARED", raising=False)
    cnt, off, idx, perm = search_raw(eng, p, r, before)
    monkeypatch.setenv("SF_K2_SHARED", "0")
    cnt0, off0, idx0, perm0 = search_raw(eng, p, r, before)
    monkeypatch.delenv("SF_K2_SHARED")
    m = p.shape[0]
    assert cnt.shape == (m + 1,) and off.shape == (m + 1,)
    assert np.array_equal(perm, perm0)
    assert cnt.tobytes() == cnt0.tobytes()
    # offset: q * cap for a list in its slot, byte-equal.  A list that outgrew its slot is refilled in an area of its own, and its
    # offset is measured from the slots' base address: it depends on where the allocator put that area, not on the sweep --
    # those offsets are held to each other relative to the area's start, and to the running sum of the refilled lists' counts.
    cap = off[m] // m
    moved = off[:m] != np.arange(m) * cap
    assert np.array_equal(moved, off0[:m] != np.arange(m) * cap) and off[m] == off0[m]
    assert off[:m][~moved].tobytes() == off0[:m][~moved].tobytes()
    if moved.any():
        rel = np.concatenate([[0], np.cumsum(cnt[:m][moved], dtype=np.int64)[:-1]])
        assert np.array_equal(off[:m][moved] - off[:m][moved][0], rel)
        assert np.array_equal(off0[:m][moved] - off0[:m][moved][0], rel)
    else:
        assert off.tobytes() == off0.tobytes()
    assert idx.tobytes() == idx0.tobytes()
    ps = p[perm]
    start = np.concatenate([[0], np.cumsum(cnt[:m], dtype=np.int64)])
    order = np.argsort(cnt[:m], kind="stable")
    pick = np.unique(np.concatenate([np.arange(0, m, every), np.arange(40), np.arange(m - 40, m), order[:20], order[-20:]]))
    for q, want in zip(pick, brute_force(ps, r, pick)):
        got = idx[start[q]:start[q + 1]]
        assert np.array_equal(got, want), (q, cnt[q], want.size)
    return cnt[:m], off, start, perm


def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [18000, 18001, 18002, 18003])
def test_uniform_cube_and_query_counts_that_leave_a_short_last_wave(eng, monkeypatch, n):
    """About 40 neighbours per ball; m = 4k, 4k + 1, 4k + 2 and 4k + 3 (the last wave has 1 .. 3 queries and sweeps them one by one)."""
    cnt, off, _, _ = check(eng, monkeypatch, cube(n, 5), 0.081)
    assert 30 < cnt.mean() < 50
    cap = off[1] - off[0]
    assert np.array_equal(off, np.arange(n + 1) * cap)  # no list outgrew its slot


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [(1, 1), (1, 2), (2, 2), (3, 3)])
def test_clouds_a_few_cells_thick_in_y_and_z(eng, monkeypatch, cells):
    """Clipped stencils: the grid has 1, 2 or 3 cells along y and along z, so the stencils have 1 .. 3 rows per axis."""
    r = 0.02
    p = cube(18000, 7) * np.array([8.0, (cells[0] - 0.2) * r, (cells[1] - 0.2) * r])
    cnt, _, _, _ = check(eng, monkeypatch, p, r)
    assert cnt.min() >= 1 and cnt.max() > 40


@pytest.mark.gpu
def test_eight_points_per_position(eng, monkeypatch):
    p = np.repeat(cube(2250, 9), 8, axis=0)
    cnt, _, _, _ = check(eng, monkeypatch, p, 0.081)  # (about five positions per ball, fewer next to the faces)
    assert (cnt % 8 == 0).all() and cnt.min() >= 8 and 24 < cnt.mean() < 64


def lattice(side):
    g = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1.0e6])
def test_lattice_with_neighbours_exactly_on_the_radius(eng, monkeypatch, shift):
    """26^3 points, spacing 2^-5, r = 3 spacings: (3, 0, 0) and (2, 2, 1) are at squared distance exactly r * r (every term is an
    exact multiple of 2^-10) and belong to the list; 123 lattice points lie within r of an interior point.  The same cloud at
    coordinates near 10^6 (still exact: 20 + 5 bits) exercises the grid-relative window bounds."""
    h = 2.0 ** -5
    p = lattice(26) * h + shift
    r = 3 * h
    cnt, _, start, perm = check(eng, monkeypatch, p, r)
    assert cnt.max() == 123
    ps = p[perm]
    q = int(np.flatnonzero((np.rint((ps - shift) / h) == 12).all(axis=1))[0])  # an interior point
    assert cnt[q] == 123
    ring = ps[brute_force(ps, r, [q])[0]] - ps[q]
    on_radius = np.flatnonzero((ring * ring).sum(axis=1) == r * r)
    found = {tuple(np.abs(np.rint(v / h)).astype(int)) for v in ring[on_radius]}
    assert (3, 0, 0) in found and (2, 2, 1) in found and on_radius.size == 30


def ring_lattice():
    """A 26^3 integer lattice with two points removed and one position holding 7 extra copies, another 1: at r^2 = 5 an interior
    point has 57 neighbours, at r^2 = 16 it has 257 -- the removals and the copies make lists of 63, 64, 65 (r^2 = 5) and of 255, 256,
    257 (r^2 = 16) entries, each side of the ring's flush (64) and wrap (256) points."""
    p = lattice(26)
    gone = (p == [12.0, 12.0, 12.0]).all(axis=1) | (p == [13.0, 12.0, 12.0]).all(axis=1)
    extra = np.vstack([np.tile([[5.0, 5.0, 5.0]], (6, 1)), np.tile([[7.0, 6.0, 5.0]], (1, 1)), np.tile([[6.0, 7.0, 5.0]], (1, 1))])
    return np.vstack([p[~gone], extra])


@pytest.mark.gpu
@pytest.mark.parametrize("r2,lengths", [(5, (63, 64, 65)), (16, (255, 256, 257))])
def test_lists_around_the_flush_and_wrap_points_of_the_ring(eng, monkeypatch, r2, lengths):
    p = ring_lattice()
    cnt, _, _, _ = check(eng, monkeypatch, p, float(np.sqrt(r2)) if r2 != 16 else 4.0)
    for n in lengths:
        assert (cnt == n).any(), (n, np.unique(cnt))


@pytest.mark.gpu
def test_lists_that_outgrow_a_slot_sized_from_a_stale_hint(eng, monkeypatch):
    """A tight cluster of 1 000 points (high z) in a sparse cloud.  A self search of the first 4 096 sorted positions -- low z, sparse --
    leaves its list statistics as the capacity hint; the search of the whole cloud then takes slots of about a hundred entries, the
    cluster's lists (hundreds of points) overflow them, are counted past the slot and refilled in an area of their own."""
    rng = np.random.default_rng(13)
    p = np.vstack([rng.random((17000, 3)), np.array([0.5, 0.5, 0.9]) + 0.02 * rng.standard_normal((1000, 3))])
    p = p.astype(np.float32).astype(np.float64)
    cnt, off, _, _ = check(eng, monkeypatch, p, 0.06, before=(0, 4096))
    m = p.shape[0]
    cap = off[1] - off[0]
    moved = off[:m] != np.arange(m) * cap
    assert cap < 200 and 500 < moved.sum() < m // 2
    assert np.array_equal(moved, cnt > cap)


@pytest.mark.gpu
def test_which_sweep_ran(eng, monkeypatch):
    """SF_K2_SHARED=2 launches the instantiation that counts its waves by path.  The stencil bounds of a query are those of its
    row of cells (cy - 1 .. cy + 1, clipped), so a wave takes the per-query sweeps exactly when its four queries straddle two rows
    -- or are fewer than four: the last wave of m = 4k + 1.  Uniform cube, 13 x 13 rows: at most 168 + 1 of the 4 501 waves.  Cloud
    three cells thick in y and z: nine rows with bounds that differ from row to row, at most 8 + 1 waves.  One or two cells
    thick: every stencil clips to the same bounds whatever the row, so every full wave shares -- with clipped stencils -- and only
    the short last wave sweeps its query alone."""
    def paths(p, r):
        monkeypatch.setenv("SF_K2_SHARED", "2")
        eng.k2_debug_paths()
        dbg = search_raw(eng, p, r)
        got = eng.k2_debug_paths()
        monkeypatch.delenv("SF_K2_SHARED")
        ref = search_raw(eng, p, r)
        assert eng.k2_debug_paths() == (0, 0)  # (the sweep that ships counts nothing)
        for a, b in zip(dbg, ref):
            assert a.tobytes() == b.tobytes()
        assert sum(got) == (p.shape[0] + 3) // 4
        return got

    shared, single = paths(cube(18001, 5), 0.081)
    assert shared >= 4501 - 169 and 1 + 40 <= single <= 169
    r = 0.02
    shared, single = paths(cube(18001, 7) * np.array([8.0, 2.8 * r, 2.8 * r]), r)
    assert 1 + 1 <= single <= 9
    shared, single = paths(cube(18001, 7) * np.array([8.0, 0.8 * r, 1.8 * r]), r)
    assert (shared, single) == (4500, 1)


def test_the_shared_sweep_keeps_the_registers_of_the_per_query_sweep():
    """From the compiler's resource remarks of the build: the shared instantiation spills nothing, uses no scratch, and runs at
    no fewer waves per SIMD than the per-query instantiation of the same launch."""
    files = glob.glob(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "search.remarks"))
    if not files:
        pytest.skip("no build/search.remarks (the library was not built by its Makefile here)")
    res, cur = {}, None
    for ln in open(files[0], errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    # k_radius<MODE = 2, SEL = false, SHARE, DBG>
    old = [v for k, v in res.items() if "k_radiusILi2ELb0ELb0ELb0EE" in k]
    new = [v for k, v in res.items() if "k_radiusILi2ELb0ELb1ELb0EE" in k]
    assert len(old) == 1 and len(new) == 1, sorted(k for k in res if "k_radiusI" in k)
    old, new = old[0], new[0]
    assert new["VGPRs Spill"] == 0 and new["SGPRs Spill"] == 0 and new["ScratchSize"] == 0, new
    assert new["Occupancy"] >= old["Occupancy"], (new, old)
    assert new["VGPRs"] <= 64, new  # eight waves per SIMD
