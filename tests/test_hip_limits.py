"""GPU tests at the size limits (all through the C ABI): the 64-bit offset arithmetic of K2 and of every kernel that reads its
lists, executed with values a 32-bit register cannot hold, and the limits the library states for itself.

  * case 1  slots of the single sweep past 2^32 elements (SF_K2_CAP), SHOT rows past 4 GiB, short lists;
  * case 2  more than 2^31 (and, at radius 0.11, 2^32) real pairs in one search, the single sweep and count -> scan -> fill;
  * case 3  the 16-bit SPFH table one row below and exactly at K7's 4 GiB buffer-addressing limit;
  * case 4  the host-side refusals whose check is the first statement of the entry point.

Every expected value comes from outside the engine: neighbour lists from a NumPy float64 brute force over the whole cloud with
the inclusion rule of include/shotfpfh.h, normals / frames / SHOT / FPFH rows from the CPU oracle at the tolerances of
tests/test_hip_round2.py::test_config_c3_fpfh_and_shot_rows_vs_oracle_at_full_size.  No sampled row is ever dropped.
The sizes each case reached on the MI355X and its wall time: profiles/limits_tests.md (printed with -s as `LIMITS ...`).
"""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import synth_cloud

pytestmark = pytest.mark.gpu

TOL = 1e-5
GIB = 1 << 30


def close(a, b, tol=TOL):
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def reserve(eng, nbytes):
    """The case's peak need in ONE allocation, freed at once: the only reason a case may skip is a device without that room."""
    import shot_fpfh_amd as s

    try:
        a = eng.empty((nbytes,), np.uint8)
    except s.ShotFpfhError as exc:
        if "out of memory" in str(exc).lower():
            pytest.skip(f"SF_ERR_NOMEM: the device cannot hold the {nbytes} bytes this case needs at once")
        raise
    a.free()


def brute_list(p, q, r):
    """KDTree.query_radius of one query by brute force: ((dx*dx + dy*dy) + dz*dz) <= r*r in float64, indices ascending."""
    d = p - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = np.flatnonzero(d2 <= r * r)
    return idx, np.sqrt(d2[idx])


def rows_at(dev, positions):
    return np.stack([dev.rows_to_host(int(i), 1)[0] for i in positions])


def check_lists(nb, p, orig, positions, r):
    """Exported lists (original numbering, ascending, with distances) of single-query slice views against brute force.
    Returns {position: neighbour indices}.  The distance is sqrt of the very float64 sum the brute force forms: 1e-15 is some
    70 ulp of a distance below 0.1, room for a square root that is not correctly rounded and for nothing else."""
    lists = {}
    for pos in positions:
        v = nb.slice(int(pos), 1)
        off, idx, dist = v.export(return_distance=True)
        v.free()
        want_idx, want_dist = brute_list(p, p[orig[pos]], r)
        assert off.tolist() == [0, want_idx.size], (pos, off.tolist(), want_idx.size)
        assert np.array_equal(idx, want_idx), (pos, idx[:8], want_idx[:8])
        assert np.abs(dist - want_dist).max() <= 1e-15, (pos, np.abs(dist - want_dist).max())
        lists[int(pos)] = want_idx
    return lists


def searched(eng, cloud, r):
    """First self search of the whole cloud with the launch timers on: (lists, names of the K2 kernels that ran)."""
    eng.profile_reset()
    eng.profile(True)
    try:
        nb = cloud.radius_search_self(r)
    finally:
        eng.profile(False)
    ran = {k for k in eng.profile_report() if k.startswith("k2_radius")}
    eng.profile_reset()
    return nb, ran


# ---- case 1 ------------------------------------------------------------------------------------------------------------------
def test_slots_past_2_to_32_elements_and_output_rows_past_4_gib(eng, O, monkeypatch):
    """n = 1.6M uniform points, radius 0.025 (~105 neighbours), SF_K2_CAP = 3968: the single sweep's slots hold 6.35e9 int32
    (25.4e9 bytes), a third of the queries have a slot offset >= 2^32, 74 798 SHOT rows start at a byte offset >= 2^32.
    Normals, frames, SHOT, FPFH (5 bins) and exported lists of 256 cell-sorted positions -- 128 at SHOT byte offsets >= 2^32
    (all within the last 5 % of the positions), 64 with slot offsets in [2^31, 2^32), 64 from the start -- against the references."""
    t0 = time.time()
    n, r, cap = 1_600_000, 0.025, 3968
    slot_bytes = cap * n * 4
    # the single sweep is taken only with these (search.hip, run_search); otherwise count -> scan -> fill runs silently
    assert slot_bytes <= 24 * GIB and cap <= ((24 * GIB // (4 * n)) // 32) * 32 and cap % 32 == 0
    pos = np.arange(n, dtype=np.int64)
    assert (pos * cap >= 2**32).mean() >= 0.25 and ((pos * cap >= 2**31) & (pos * cap < 2**32)).any()
    first_far_row = -(-2**32 // (352 * 8))  # first SHOT row whose byte offset is >= 2^32
    assert n - first_far_row >= 50_000 and first_far_row >= n - n // 20
    reserve(eng, slot_bytes + n * (352 + 125 + 9 + 3) * 8 + (2 << 30))
    p, nr, _ = synth_cloud(n, 101)
    rng = np.random.default_rng(1001)
    lo31, lo32 = -(-2**31 // cap), -(-2**32 // cap)  # first positions with slot offsets >= 2^31, >= 2^32
    pick = np.sort(np.concatenate([
        np.arange(n - 16, n), rng.choice(np.arange(first_far_row, n - 16), 112, replace=False),
        rng.choice(np.arange(lo31, lo32), 64, replace=False), np.arange(4), rng.choice(np.arange(4, lo31), 60, replace=False)]))
    assert pick.size == 256 and np.unique(pick).size == 256
    assert (pick * 352 * 8 >= 2**32).sum() == 128 and (pick * cap >= 2**32).sum() == 128
    assert ((pick * cap >= 2**31) & (pick * cap < 2**32)).sum() == 64 and (pick * cap < 2**31).sum() == 64

    monkeypatch.setenv("SF_K2_CAP", str(cap))
    cloud = eng.cloud(p, nr)
    held = []
    try:
        nb, ran = searched(eng, cloud, r)
        held.append(nb)
        monkeypatch.delenv("SF_K2_CAP")
        # the lists are the planned main forms in slots nobody outgrew: the sweep ran, nothing was re-done
        assert ran == {"k2_radius_slots"}, ran
        assert nb.m == n and nb.max_count < cap and 95 < nb.total / n < 115, (nb.max_count, nb.total / n)
        print(f"LIMITS case1 n={n} cap={cap} slot_elements={cap * n} slot_bytes={slot_bytes} total={nb.total} "
              f"max_count={nb.max_count} n_overflow=0 kernels={sorted(ran)}")
        orig = cloud.perm().astype(np.int64)
        nrm_d, lrf_d = eng.empty((n, 3)), eng.empty((n, 9))
        shot_d, fpfh_d = eng.empty((n, 352)), eng.empty((n, 125))
        held += [nrm_d, lrf_d, shot_d, fpfh_d]
        nb.normals(out=nrm_d)
        nb.shot_single_scale(True, 10, out=shot_d, lrf_out=lrf_d)
        sp = eng.spfh(cloud, 5, nb.max_count)
        held.append(sp)
        sp.compute(nb).fpfh(nb, out=fpfh_d)
        eng.sync()
        t_dev = time.time() - t0
        kp = orig[pick]
        check_lists(nb, p, orig, pick, r)
        got = rows_at(nrm_d, pick)
        want = O.compute_normals(p[kp], p, radius=r)
        assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        got = rows_at(lrf_d, pick)
        want = O.shot_lrf(p, p[kp], r).reshape(-1, 9)
        assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        got = rows_at(shot_d, pick)
        want = O.shot_single_scale(p, nr, p[kp], r, True, 10)
        assert want.any(axis=1).all()
        assert close(got, want).all() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        got = rows_at(fpfh_d, pick)
        want = O.compute_fpfh_descriptor_sample(kp, p, nr, r, 5)
        assert close(got, want).all() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        print(f"LIMITS case1 wall_s={time.time() - t0:.1f} (until the device work was done: {t_dev:.1f})")
    finally:
        for h in reversed(held):
            h.free()
        cloud.free()


# ---- case 2 ------------------------------------------------------------------------------------------------------------------
_case2 = {}  # the cloud, and per radius the oracle's rows: the schemes of one radius share them


@pytest.mark.parametrize("scheme,r", [("sweep", 0.09), ("exact", 0.09), ("exact", 0.11)])
def test_more_than_2_to_31_pairs_in_one_search(eng, O, monkeypatch, scheme, r):
    """n = 1M uniform points, radius 0.09: n^2 (4/3 pi r^3 - 3/2 pi r^4 + 8/5 r^5 - r^6/6) ~ 2.75e9 pairs > 2^31 in lists of
    ~2 750 points.  `sweep`: the default single sweep into slots sized from a sample of the lists; `exact`: SF_K2_EXACT=1,
    rocPRIM's scan of int64 offsets with a total past 2^31.  Exported lists of 64 positions (the last 16 among them) against
    brute force, with the symmetry of the sampled lists; normals of 256 positions, SHOT and FPFH (5 bins) rows of 32 against
    the oracle.
    Radius 0.11 (the descriptors of radius 0.09 take 0.2 s on the device): 4.9e9 pairs > 2^32 in lists of ~5 000 points, 20 GB
    of indices, so the scanned offsets of `exact` pass 2^32 too; the oracle's cost grows with the square of the list length
    (32 FPFH keypoints at 0.09 are 88 000 SPFH rows of 2 750 pairs each: 19 s), so this radius compares 16 keypoints."""
    t0 = time.time()
    n = 1_000_000
    if "p" not in _case2:
        _case2["p"], _case2["nr"], _ = synth_cloud(n, 102)
    p, nr, ref = _case2["p"], _case2["nr"], _case2.setdefault(r, {})
    expect = n * n * (4 / 3 * np.pi * r**3 - 1.5 * np.pi * r**4 + 1.6 * r**5 - r**6 / 6)
    assert expect > (2**31 if r < 0.1 else 2**32)
    reserve(eng, 24 * GIB + n * (352 + 125 + 3) * 8 + (4 << 30))
    if scheme == "exact":
        monkeypatch.setenv("SF_K2_EXACT", "1")
    cloud = eng.cloud(p, nr)
    held = []
    try:
        nb, ran = searched(eng, cloud, r)
        held.append(nb)
        monkeypatch.delenv("SF_K2_EXACT", raising=False)
        assert nb.total > (2**31 if r < 0.1 else 2**32), nb.total  # the precondition of this case
        assert abs(nb.total / expect - 1) < 0.01, (nb.total, expect)
        assert ("k2_radius_slots" in ran) == (scheme == "sweep") and ("k2_radius_fill" in ran) == (scheme == "exact"), ran
        print(f"LIMITS case2[{scheme}-{r}] n={n} total={nb.total} max_count={nb.max_count} kernels={sorted(ran)}")
        orig = cloud.perm().astype(np.int64)
        rng = np.random.default_rng(1002)
        top = n - n // 10
        list_pos = np.sort(np.concatenate([np.arange(n - 16, n), rng.choice(np.arange(top, n - 16), 24, replace=False),
                                           rng.choice(top, 24, replace=False)]))
        nrm_pos = np.sort(np.concatenate([np.arange(n - 16, n), rng.choice(np.arange(top, n - 16), 112, replace=False),
                                          rng.choice(top, 128, replace=False)]))
        n_kp = 32 if r < 0.1 else 16
        kp_pos = np.sort(np.concatenate([np.arange(n - 4, n), rng.choice(np.arange(top, n - 4), n_kp // 2 - 4, replace=False),
                                         rng.choice(np.arange(n // 2, top), n_kp // 4, replace=False),
                                         rng.choice(n // 2, n_kp // 4, replace=False)]))
        assert list_pos.size == 64 and nrm_pos.size == 256 and kp_pos.size == n_kp
        nrm_d, shot_d, fpfh_d = eng.empty((n, 3)), eng.empty((n, 352)), eng.empty((n, 125))
        held += [nrm_d, shot_d, fpfh_d]
        td = time.time()
        nb.normals(out=nrm_d)
        nb.shot_single_scale(True, 10, out=shot_d)
        sp = eng.spfh(cloud, 5, nb.max_count)
        held.append(sp)
        sp.compute(nb).fpfh(nb, out=fpfh_d)
        eng.sync()
        t_desc = time.time() - td
        lists = check_lists(nb, p, orig, list_pos, r)
        inv = np.empty(n, np.int64)
        inv[orig] = np.arange(n)
        pairs = 0
        for a, la in lists.items():  # j in list(i) <=> i in list(j), on the sampled lists (the last 16 positions are neighbours)
            for b in inv[la]:
                if int(b) in lists and b != a:
                    pairs += 1
                    assert orig[a] in lists[int(b)], (a, int(b))
        assert pairs > 0
        got = rows_at(nrm_d, nrm_pos)
        want = O.compute_normals(p[orig[nrm_pos]], p, radius=r)
        assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        kp = orig[kp_pos]
        to = time.time()
        key = tuple(kp.tolist())
        if ref.get("key") != key:  # (both schemes sort the cloud alike: the same keypoints, one oracle run)
            ref["key"] = key
            ref["shot"] = O.shot_single_scale(p, nr, p[kp], r, True, 10)
            ref["fpfh"] = O.compute_fpfh_descriptor_sample(kp, p, nr, r, 5)
            ref["oracle_s"] = time.time() - to
        got = rows_at(shot_d, kp_pos)
        want = ref["shot"]
        assert want.any(axis=1).all()
        assert close(got, want).all() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        got = rows_at(fpfh_d, kp_pos)
        want = ref["fpfh"]
        assert close(got, want).all() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        print(f"LIMITS case2[{scheme}-{r}] wall_s={time.time() - t0:.1f} descriptors_s={t_desc:.2f} symmetric_pairs={pairs} "
              f"oracle_shot_fpfh_s={ref['oracle_s']:.1f}")
    finally:
        for h in reversed(held):
            h.free()
        cloud.free()


# ---- case 3 ------------------------------------------------------------------------------------------------------------------
def _table_case(eng, n, seed):
    r = 0.012  # ~30 neighbours per point at 4.19M points in the unit cube
    p, nr, _ = synth_cloud(n, seed)
    cloud = eng.cloud(p, nr)
    nb = cloud.radius_search_self(r)
    sp = eng.spfh(cloud, 8, nb.max_count)
    return r, p, nr, cloud, nb, sp


def test_spfh_table_one_row_below_4_gib(eng, O):
    """8 bins without a radius window: 16-bit counts in rows of 1 024 bytes.  n = 4 194 303 rows are 2^32 - 1024 bytes: K6 and K7
    run, and the FPFH rows of 128 keypoints among the last 1 024 cell-sorted positions (the last one included: neighbours in a
    cell-sorted cloud sit at nearby positions, so the top of the table is read) and of 128 from the first half equal the oracle's."""
    t0 = time.time()
    n = 4_194_303
    reserve(eng, 6 * GIB)
    r, p, nr, cloud, nb, sp = _table_case(eng, n, 103)
    try:
        assert sp.elem_bytes == 2 and n * 512 * sp.elem_bytes == 2**32 - 1024
        assert 25 < nb.total / n < 35, nb.total / n
        sp.compute(nb)
        orig = cloud.perm().astype(np.int64)
        rng = np.random.default_rng(1003)
        pos = np.sort(np.concatenate([[n - 1], n - 1024 + rng.choice(1023, 127, replace=False), rng.choice(n // 2, 128, replace=False)]))
        assert pos.size == 256
        kp = orig[pos]
        got = sp.fpfh(nb, keypoints_indices=kp)
        want = O.compute_fpfh_descriptor_sample(kp, p, nr, r, 8)
        assert want.any(axis=1).all()
        assert close(got, want).all() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()
        print(f"LIMITS case3[below] n={n} table_bytes={n * 512 * sp.elem_bytes} total={nb.total} max_count={nb.max_count} "
              f"wall_s={time.time() - t0:.1f}")
    finally:
        sp.free()
        nb.free()
        cloud.free()


def test_spfh_table_of_4_gib_is_refused_by_k7_and_the_context_lives_on(eng, O):
    """n = 4 194 304 rows of 1 024 bytes are exactly 2^32 bytes: K6 (64-bit row pointers) fills the table, sf_fpfh returns
    SF_ERR_UNSUPPORTED before its launch, and the context serves the next FPFH call."""
    import shot_fpfh_amd as s
    from shot_fpfh_amd import _ffi

    t0 = time.time()
    n = 4_194_304
    reserve(eng, 6 * GIB)
    r, p, nr, cloud, nb, sp = _table_case(eng, n, 104)
    try:
        assert sp.elem_bytes == 2 and n * 512 * sp.elem_bytes == 2**32
        sp.compute(nb)
        eng.sync()
        kp = np.array([0, 1, n - 2, n - 1], dtype=np.int64)
        out = np.zeros((kp.size, 512))
        rc = eng.lib.sf_fpfh(eng.h, cloud.h, nb.h, sp.h, kp.ctypes.data_as(C.c_void_p), kp.size, out.ctypes.data_as(C.c_void_p),
                             _ffi.SF_HOST)
        assert rc == -6, (rc, _ffi.last_error())  # SF_ERR_UNSUPPORTED
        assert "SPFH table of 4294967296 bytes exceeds the 4 GiB buffer-addressing limit of the K7 kernel" in _ffi.last_error()
        assert not out.any()
        print(f"LIMITS case3[at] n={n} table_bytes={n * 512 * sp.elem_bytes} total={nb.total} max_count={nb.max_count} "
              f"wall_s={time.time() - t0:.1f}")
    finally:
        sp.free()
        nb.free()
        cloud.free()
    q, qn, _ = synth_cloud(20000, 105)
    kp = np.arange(0, 20000, 100)
    got = s.compute_fpfh_descriptor(kp, q, qn, 0.06, 8, verbose=False)
    want = O.compute_fpfh_descriptor(kp, q, qn, 0.06, 8)
    assert want.any() and np.abs(got - want).max() < 1e-9, np.abs(got - want).max()


# ---- case 4 ------------------------------------------------------------------------------------------------------------------
def test_first_refused_sizes_never_reach_a_kernel(eng):
    """2 147 483 001 queries / points with a valid small buffer: each of these entry points compares the size in its FIRST
    statement -- before any allocation, copy or launch -- so the buffer is never read past its end.  The code (NULL plus
    sf_last_error for the handle-returning ones), and an ordinary call on the same context right after each refusal.
    Left out, because their checks sit behind allocations, copies or launches that a refused size would already have reached,
    or need a real cloud of that size: sf_fpfh's keypoint count (fpfh.hip, generic kernel), sf_knn_search's candidate total,
    the work-group and pair counts of the matching pre-filters, the draw count of sf_ransac_score (Limits)."""
    from shot_fpfh_amd import _ffi

    lib = eng.lib
    big = 2_147_483_001
    p, _, _ = synth_cloud(3000, 106)
    cloud = eng.cloud(p)
    q = np.ascontiguousarray(p[:4])
    qp, out = q.ctypes.data_as(C.c_void_p), np.zeros((4, 3))
    want = [brute_list(p, q[i], 0.1)[0] for i in range(4)]

    def ordinary():
        nb = cloud.radius_search(q, 0.1)
        off, idx = nb.export()
        nb.free()
        assert all(np.array_equal(idx[off[i]:off[i + 1]], want[i]) for i in range(4))

    try:
        ordinary()
        assert not lib.sf_radius_search(eng.h, cloud.h, qp, big, 0.1, _ffi.SF_HOST)
        assert _ffi.last_error() == "sf_radius_search: bad arguments (m=2147483001)"
        ordinary()
        assert not lib.sf_knn_search(eng.h, cloud.h, qp, big, 1, _ffi.SF_HOST)
        assert _ffi.last_error() == "sf_knn_search: bad arguments (m=2147483001)"
        ordinary()
        rc = lib.sf_normals_radius(eng.h, cloud.h, qp, big, 0, 0, 0.1, None, out.ctypes.data_as(C.c_void_p), _ffi.SF_HOST)
        assert rc == -1 and _ffi.last_error() == "sf_normals_radius: bad query count 2147483001"  # SF_ERR_ARG
        assert not out.any()
        ordinary()
        offsets, idx = np.zeros(5, np.int64), np.zeros(4, np.int64)
        assert not lib.sf_nbrs_import(eng.h, cloud.h, qp, big, offsets.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 0.1,
                                      _ffi.SF_HOST)
        assert _ffi.last_error() == "sf_nbrs_import: bad arguments (m=2147483001)"
        ordinary()
        assert not lib.sf_voxels_build(eng.h, qp, big, 0.1, _ffi.SF_HOST)
        assert _ffi.last_error() == "sf_voxels_build: bad argument"
        ordinary()
        assert not lib.sf_cloud_upload(eng.h, qp, None, big, _ffi.SF_HOST)
        assert _ffi.last_error() == "sf_cloud_upload: bad arguments (n=2147483001)"
        ordinary()
        # the largest accepted size is not what these calls object to: the same calls with 4 pass
        small = _ffi.check_handle(lib.sf_cloud_upload(eng.h, qp, None, 4, _ffi.SF_HOST), "sf_cloud_upload")
        lib.sf_cloud_free(eng.h, small)
    finally:
        cloud.free()
