"""Spin images on the MI355X (K24) against their NumPy statement (tests/spin_numpy.py).

The statement is fed the lists the device itself exported (or the ones it was given) and the library's own scale.  A row is then
a matter of integer weights, one correctly rounded conversion and an exact scaling or one division: rows are compared by EXACT
equality of their bit patterns."""

from fractions import Fraction

import numpy as np
import pytest

import spin_numpy as S
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd import ShotFpfhError, _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(engine, pts, nrm, kp, axes, R, W=8, lists=None, **opts):
    """(device rows, device counts, lists in the caller's numbering) of one layered call: the search (or the import of `lists`),
    the rows.  nrm may be None: a cloud of positions alone."""
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(kp, R) if lists is None else cloud.import_neighbors(kp, lists, R)
        try:
            rows, counts = nb.spin_images(axes, W, return_counts=True, **opts)
            rows = np.array(rows)
            off, idx = nb.export()
        finally:
            nb.free()
    finally:
        cloud.free()
    return rows, counts, [idx[off[i]:off[i + 1]] for i in range(kp.shape[0])]


def check_exact(engine, pts, nrm, kp, axes, R, W=8, lists=None, **opts):
    """The device's rows and counts equal the statement's on the device's own lists; imported lists keep their order and their
    repetitions in the statement (the export sorts a list, which changes no bit: the order test says so)."""
    rows, counts, got_lists = run(engine, pts, nrm, kp, axes, R, W, lists, **opts)
    fed = got_lists if lists is None else lists
    want, want_c = S.rows(pts, nrm, kp, axes, fed, R, W, opts.get("signed_beta", True), opts.get("min_cos"),
                          opts.get("normalize", False), opts.get("min_neighborhood_size", 0), return_counts=True)
    assert rows.shape == want.shape == (kp.shape[0], S.shape(W, opts.get("signed_beta", True))[1])
    wrong = np.flatnonzero((bits(rows) != bits(want)).any(axis=1))
    assert wrong.size == 0, (wrong[:5], [len(fed[i]) for i in wrong[:5]])
    assert counts.dtype == np.int32 and np.array_equal(counts, want_c)
    return rows, counts, got_lists


def _pick(n, m, seed=3):
    return np.sort(np.random.default_rng(seed).choice(n, min(m, n), replace=False))


def _lattice():
    pts = family("lattice", 4096, np.random.default_rng(1))[0]
    return pts, np.tile(np.array([1.0, 2.0, 2.0]) / 3.0, (pts.shape[0], 1))  # one tilted common normal


# ---- the families -------------------------------------------------------------------------------------------------------------
FAMILY = {
    # name: (points and normals, radius)
    "uniform": (lambda: family("uniform", 5000, np.random.default_rng(1))[:2], 0.14),
    "noisy_sphere": (lambda: config1_cloud(5000, 2), 0.12),
    "clustered": (lambda: family("clustered", 5000, np.random.default_rng(1))[:2], 0.03),
    "lattice_tilted_normal": (_lattice, 0.125),
    "duplicates": (lambda: family("duplicates", 5000, np.random.default_rng(1))[:2], 0.14),
    "far_origin": (lambda: family("far_origin", 5000, np.random.default_rng(1))[:2], 0.14),
    "three_points": (lambda: synth_cloud(3, 7)[:2], 2.0),
}


@pytest.mark.parametrize("signed_beta", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("name", list(FAMILY))
def test_rows_equal_the_statement_bit_for_bit(engine, name, signed_beta):
    make, R = FAMILY[name]
    pts, nrm = make()
    idx = _pick(pts.shape[0], 200)
    rows, counts, lists = check_exact(engine, pts, nrm, pts[idx], nrm[idx], R, signed_beta=signed_beta)
    sizes = np.array([len(a) for a in lists])
    print(name, "list lengths: min %d, median %d, max %d; contributing: median %d" % (sizes.min(), np.median(sizes), sizes.max(), np.median(counts)))
    assert rows.any() and np.isfinite(rows).all() and (rows >= 0).all()
    assert np.array_equal(rows.sum(axis=1), counts.astype(np.float64))  # (mass is conserved to the bit)
    assert (counts < sizes).all()  # (the keypoint itself is in its list and takes no part)
    if name == "clustered":
        assert (sizes > 128).sum() >= 10 and (sizes <= 64).sum() >= 5  # several steps of 128, and less than one
    elif name != "three_points":
        assert 30 <= np.median(sizes) <= 100
    if name == "duplicates":  # d2 == 0 beyond the keypoint itself: its exact duplicates
        zero = [int((((pts[a] - pts[i]) ** 2).sum(axis=1) == 0).sum()) for i, a in zip(idx[:40], lists[:40])]
        assert sum(1 for z in zero if z >= 2) >= 10
    if name == "three_points":
        assert sizes.tolist() == [3, 3, 3] and rows.any(axis=1).all()


# ---- list lengths around the lanes of a wave and the step of 128 ----------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000]


@pytest.mark.parametrize("signed_beta", [True, False], ids=["signed", "unsigned"])
def test_imported_lists_of_every_length_around_a_wave_and_a_step(engine, signed_beta):
    pts, nrm, _ = synth_cloud(1200, 9)
    rng = np.random.default_rng(10)
    kp = pts[: len(LENGTHS)] + 1e-3
    axes = nrm[: len(LENGTHS)]
    lists = [rng.permutation(1200)[:n] for n in LENGTHS]
    rows, counts, got = check_exact(engine, pts, nrm, kp, axes, 0.6, lists=lists, signed_beta=signed_beta)
    assert [len(a) for a in got] == LENGTHS
    assert not rows[0].any() and counts[0] == 0 and (counts[3:] > 0).all() and rows[3:].any(axis=1).all()
    assert np.array_equal(rows.sum(axis=1), counts.astype(np.float64))


def test_a_repeated_entry_contributes_again(engine):
    pts, nrm, _ = synth_cloud(300, 11)
    lists = [np.r_[np.arange(150), np.arange(100)], np.arange(150), np.arange(100), np.full(70, 5), np.r_[np.arange(200), np.arange(200)],
             np.arange(200)]
    rows, counts, _ = check_exact(engine, pts, nrm, np.tile(pts[7] + 1e-3, (6, 1)), np.tile(nrm[7], (6, 1)), 0.9, lists=lists)
    assert counts[0] == counts[1] + counts[2] and counts[3] in (0, 70) and counts[4] == 2 * counts[5] and counts[5] > 0
    assert np.array_equal(bits(rows[0]), bits(rows[1] + rows[2])) and np.array_equal(bits(rows[4]), bits(2.0 * rows[5]))


def test_a_list_of_two_to_the_24_entries_is_refused(engine):
    """Through an imported list of repeated indices: the kernel does not walk it (it raises the error word)."""
    pts, nrm, _ = synth_cloud(300, 12)
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.import_neighbors(pts[:2], [np.arange(40), np.arange(S.MAX_LIST, dtype=np.int32) % 300], 0.5)
        try:
            with pytest.raises(ShotFpfhError, match=r"\(-1\).*sf_spin_images:.*entries"):
                nb.spin_images(nrm[:2])
        finally:
            nb.free()
    finally:
        cloud.free()


# ---- order ----------------------------------------------------------------------------------------------------------------------
def test_permuting_a_list_or_the_cloud_changes_no_bit(engine):
    pts, nrm = family("clustered", 5000, np.random.default_rng(1))[:2]
    idx = _pick(5000, 200)
    kp, axes = pts[idx], nrm[idx]
    first, c1, lists = run(engine, pts, nrm, kp, axes, 0.03, min_cos=0.2)
    again, c2, _ = run(engine, pts, nrm, kp, axes, 0.03, min_cos=0.2)
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(c1, c2) and first.any()
    rng = np.random.default_rng(8)
    mixed, c3, _ = run(engine, pts, nrm, kp, axes, 0.03, lists=[rng.permutation(a) for a in lists], min_cos=0.2)
    assert np.array_equal(bits(first), bits(mixed)) and np.array_equal(c1, c3)
    order = rng.permutation(5000)
    shuffled, c4, _ = run(engine, pts[order], nrm[order], kp, axes, 0.03, min_cos=0.2)
    assert np.array_equal(bits(first), bits(shuffled)) and np.array_equal(c1, c4)


# ---- signs ----------------------------------------------------------------------------------------------------------------------
def test_unsigned_rows_do_not_see_the_sign_of_any_normal(engine):
    pts, nrm = config1_cloud(5000, 2)
    idx = _pick(5000, 200)
    flip = np.where(np.random.default_rng(4).random(5000) < 0.5, -1.0, 1.0)[:, None]
    assert 50 < (flip[idx] < 0).sum() < 150
    turned = nrm * flip
    for min_cos in (None, 0.99):
        a, ca, _ = check_exact(engine, pts, nrm, pts[idx], nrm[idx], 0.12, signed_beta=False, min_cos=min_cos)
        b, cb, _ = check_exact(engine, pts, turned, pts[idx], turned[idx], 0.12, signed_beta=False, min_cos=min_cos)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(ca, cb) and a.any()
    full = run(engine, pts, nrm, pts[idx], nrm[idx], 0.12, signed_beta=False)[1]
    assert (ca <= full).all() and (ca < full).any()  # (the support angle at 0.99 did reject neighbours)
    c, _, _ = run(engine, pts, turned, pts[idx], turned[idx], 0.12, signed_beta=True)
    d, _, _ = run(engine, pts, nrm, pts[idx], nrm[idx], 0.12, signed_beta=True)
    assert not np.array_equal(bits(c), bits(d))  # (the signed image does see them)


# ---- edges: entries exactly on nodes, on quantisation steps, on the image's border ----------------------------------------------
EDGE_W, EDGE_K = 8, 3  # inv_bin = 2^3: a bin is 1 / 8 wide, the image reaches alpha = 1 and |beta| = 1


def _edge_offsets():
    """(x, z) of single neighbours of a keypoint at the origin with axis (0, 0, 1): alpha = |x| exactly when z = 0 (the root of a
    rounded square is the number itself), beta = z exactly, and a2 = 0 exactly when x = 0."""
    W, ib = EDGE_W, 2.0 ** EDGE_K
    up, down = (lambda a: np.nextafter(a, np.inf)), (lambda a: np.nextafter(a, -np.inf))
    u_vals = []
    for i in range(W + 1):  # image nodes and one ulp either side; u = W exactly (kept) and one ulp above (skipped)
        u_vals += [i / ib, up(i / ib)] + ([down(i / ib)] if i else [])
    for q in (0, 1, 32768, 65535):  # fractions of exactly q / 65536 and one ulp either side
        x = (3 + q / 65536.0) / ib
        u_vals += [x, up(x), down(x)]
    offs = [(x, 0.0) for x in u_vals] + [(x, -0.0) for x in u_vals[:4]]  # beta = +0 and -0; (0, 0): d2 = 0
    t_vals = []
    for i in range(-W, W + 1):
        t_vals += [i / ib, up(i / ib), down(i / ib)]  # |t| = W exactly and one ulp beyond, on both sides
    for q in (1, 32768, 65535):
        z = (2 + q / 65536.0) / ib
        t_vals += [z, up(z), down(z), -z, up(-z), down(-z)]
    t_vals += [2.0 ** -40, -(2.0 ** -40)]
    offs += [(0.0, z) for z in t_vals]  # the axis-parallel offsets: a2 = 0
    offs += [(0.375, z) for z in t_vals[:12]] + [(x, 0.25) for x in u_vals[:12]]  # and both coordinates at work
    return np.array(offs)


def _closed_form(x, z, signed_beta):
    """node -> weight of one entry (x, 0, z) by exact rational arithmetic, for x = 0 or z = 0; None: skipped."""
    W, ib = EDGE_W, 2 ** EDGE_K
    d2 = (x * x + 0.0) + z * z
    u = Fraction(abs(x)) * ib
    t = Fraction(z if signed_beta else abs(z)) * ib
    if not (d2 > 0 and u <= W and abs(t) <= W):
        return None
    v = Fraction(float(t) + float(W)) if signed_beta else t  # (v = t + W is one float64 add: the statement's rounding)
    NV = 2 * W + 1 if signed_beta else W + 1
    iu, iv = int(u // 1), int(v // 1)
    qu, qv = int(((u - iu) * 65536) // 1), int(((v - iv) * 65536) // 1)
    w = {(iu, iv): (65536 - qu) * (65536 - qv), (iu + 1, iv): qu * (65536 - qv), (iu, iv + 1): (65536 - qu) * qv, (iu + 1, iv + 1): qu * qv}
    return {a * NV + b: val for (a, b), val in w.items() if val}


@pytest.mark.parametrize("signed_beta", [True, False], ids=["signed", "unsigned"])
def test_entries_exactly_on_nodes_steps_and_borders(engine, signed_beta):
    W = EDGE_W
    R = (W * np.sqrt(2.0)) / 2 ** EDGE_K
    assert S.scale(R, W) == 2.0 ** EDGE_K
    offs = _edge_offsets()
    m = offs.shape[0]
    pts = np.vstack([np.zeros((1, 3)), np.column_stack([offs[:, 0], np.zeros(m), offs[:, 1]])])
    kp = np.zeros((m, 3))
    axes = np.tile(np.array([0.0, 0.0, 1.0]), (m, 1))
    lists = [np.array([i + 1]) for i in range(m)]
    rows, counts, _ = check_exact(engine, pts, None, kp, axes, R, W, lists=lists, signed_beta=signed_beta)
    kept = skipped = 0
    for i, (x, z) in enumerate(offs):
        if x != 0.0 and z != 0.0:
            continue  # (only the statement speaks)
        want = _closed_form(x, z, signed_beta)
        if want is None:
            skipped += 1
            assert counts[i] == 0 and not rows[i].any(), (i, x, z)
        else:
            kept += 1
            assert counts[i] == 1 and sum(want.values()) == 1 << 32
            got = {int(b): int(rows[i, b] * S.TWO32) for b in np.flatnonzero(rows[i])}
            assert got == want, (i, x, z, got, want)
    assert kept >= 100 and skipped >= 6
    # u = W exactly: the whole weight on the last node of its column, and nothing one ulp above
    NV = S.shape(W, signed_beta)[0]
    at_w = int(np.flatnonzero((offs[:, 0] == 1.0) & (offs[:, 1] == 0.0) & ~np.signbit(offs[:, 1]))[0])
    assert rows[at_w, W * NV + (W if signed_beta else 0)] == 1.0 and counts[at_w + 1] == 0 and offs[at_w + 1, 0] > 1.0
    # and all of them in one list, about a tilted keypoint axis too: only the statement speaks
    both = [np.arange(1, m + 1), np.arange(1, m + 1)[::-1]]
    tilt = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8]])
    check_exact(engine, pts, None, np.zeros((2, 3)), tilt, R, W, lists=both, signed_beta=signed_beta)


# ---- the support angle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed_beta", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("min_cos", [-1.0, 0.0, 0.5, 1.0])
def test_support_angle_with_neighbours_exactly_on_it(engine, min_cos, signed_beta):
    cz = [-1.0, -0.5, -0.0, 0.0, 0.5, 1.0]
    cz += [np.nextafter(c, -np.inf) for c in cz] + [np.nextafter(c, np.inf) for c in cz]  # c = m_z exactly: the axis is (0, 0, 1)
    k = len(cz)
    nrm = np.vstack([[0.0, 0.0, 1.0], np.column_stack([np.full(k, 0.25), np.full(k, -0.5), cz])])
    pts = np.vstack([np.zeros((1, 3)), np.column_stack([0.0625 * (1 + np.arange(k)) / k, np.full(k, 0.03125), np.full(k, 0.015625)])])
    lists = [np.arange(1, k + 1)] + [np.array([j + 1]) for j in range(k)]
    kp = np.zeros((k + 1, 3))
    axes = np.tile(np.array([0.0, 0.0, 1.0]), (k + 1, 1))
    rows, counts, _ = check_exact(engine, pts, nrm, kp, axes, 0.25, lists=lists, signed_beta=signed_beta, min_cos=min_cos)
    passes = np.array([(c if signed_beta else abs(c)) >= min_cos for c in cz])
    assert np.array_equal(counts[1:], passes.astype(np.int32)) and counts[0] == passes.sum()
    on_it = [j for j, c in enumerate(cz) if (c if signed_beta else abs(c)) == min_cos]
    assert (on_it or (not signed_beta and min_cos < 0)) and all(counts[1 + j] == 1 for j in on_it)  # (exactly on the angle: kept)
    assert 0 < passes.sum() and (min_cos < 0.5 or passes.sum() < k)


# ---- widths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed_beta", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("W", [1, 2, 8, 16, 44])
def test_widths(engine, W, signed_beta):
    pts, nrm = config1_cloud(4000, 4)
    idx = _pick(4000, 150)
    rows, counts, _ = check_exact(engine, pts, nrm, pts[idx], nrm[idx], 0.15, W, signed_beta=signed_beta)
    assert rows.shape[1] == (W + 1) * (2 * W + 1 if signed_beta else W + 1) and rows.any(axis=1).all()


# ---- the gate, the normalisation, the counts --------------------------------------------------------------------------------------
def test_gate_normalisation_and_counts(engine):
    pts, nrm = config1_cloud(5000, 2)
    idx = _pick(5000, 200)
    kp, axes, R = pts[idx], nrm[idx], 0.12
    rows, counts, _ = check_exact(engine, pts, nrm, kp, axes, R)
    assert np.array_equal(rows.sum(axis=1), counts.astype(np.float64)) and counts.min() > 3
    chosen = int(np.argsort(counts)[100])
    c = int(counts[chosen])
    for min_nb, alive in ((c - 1, True), (c, False), (c + 1, False)):
        gated, gc, _ = check_exact(engine, pts, nrm, kp, axes, R, min_neighborhood_size=min_nb)
        assert bool(gated[chosen].any()) == alive and np.array_equal(gc, counts)
        assert np.array_equal(gated.any(axis=1), counts > min_nb)
    for signed_beta in (True, False):
        norm, nc, _ = check_exact(engine, pts, nrm, kp, axes, R, signed_beta=signed_beta, normalize=True)
        assert np.abs(norm.sum(axis=1) - 1.0).max() < 1e-13
    both, _, _ = check_exact(engine, pts, nrm, kp, axes, R, normalize=True, min_neighborhood_size=c, min_cos=0.5)
    assert both.any(axis=1).any() and not both.any(axis=1).all()
    # without return_counts: the rows alone, the same bits
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(kp, R)
        try:
            alone = np.array(nb.spin_images(axes))
        finally:
            nb.free()
    finally:
        cloud.free()
    assert np.array_equal(bits(alone), bits(rows))


# ---- interfaces -----------------------------------------------------------------------------------------------------------------
def test_keypoints_outside_the_cloud_get_rows_of_zeros(engine):
    pts, nrm, _ = synth_cloud(2000, 5)
    kp = np.vstack([pts[:5], pts[:20] + 10.0])
    axes = np.vstack([nrm[:5], nrm[:20]])
    rows, counts, lists = check_exact(engine, pts, nrm, kp, axes, 0.2)
    assert all(len(a) == 0 for a in lists[5:]) and not rows[5:].any() and rows[:5].any(axis=1).all() and not counts[5:].any()


def test_device_axes_and_output_equal_the_host_route(engine):
    pts, nrm = config1_cloud(3000, 6)
    idx = _pick(3000, 100)
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(pts[idx], 0.15)
        try:
            host, hc = nb.spin_images(nrm[idx], min_cos=0.3, return_counts=True)
            host = np.array(host)
            dev, dax = engine.empty((100, 153)), engine.empty((100, 3))
            try:
                dax.from_host(nrm[idx])
                got, dc = nb.spin_images(dax, min_cos=0.3, out=dev, return_counts=True)
                assert got is dev and np.array_equal(bits(dev.to_host()), bits(host)) and np.array_equal(dc, hc) and host.any()
                assert np.array_equal(bits(np.array(nb.spin_images(dax, min_cos=0.3))), bits(host))  # device axes, host rows
                assert nb.spin_images(nrm[idx], min_cos=0.3, out=dev) is dev  # host axes, device rows
                assert np.array_equal(bits(dev.to_host()), bits(host))
                with pytest.raises(ValueError):
                    nb.spin_images(nrm[idx], 16, out=dev)
            finally:
                dev.free()
                dax.free()
        finally:
            nb.free()
    finally:
        cloud.free()


def test_refused_arguments_fail_through_the_raw_call(engine):
    pts, nrm, _ = synth_cloud(500, 1)
    axes = np.ascontiguousarray(nrm[:10])
    out = np.zeros(10 * 4005)
    lib = engine.lib

    def raw(cloud, nb, ax, W, use_cos=0, min_cos=0.0, o=out):
        return lib.sf_spin_images(engine.h, cloud.h, nb.h, None if ax is None else ax.ctypes.data, W, 1, use_cos, min_cos, 0, 0,
                                  None if o is None else o.ctypes.data, None, 0)

    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(pts[:10], 0.2)
        try:
            bad_axes = axes.copy()
            bad_axes[4, 2] = np.inf
            nan_axes = axes.copy()
            nan_axes[0, 0] = np.nan
            for args in [(axes, 0), (axes, 45), (axes, -3), (None, 8), (bad_axes, 8), (nan_axes, 8), (axes, 8, 1, 1.5), (axes, 8, 1, -1.25),
                         (axes, 8, 1, float("nan"))]:
                assert raw(cloud, nb, *args) == -1 and _ffi.last_error().startswith("sf_spin_images:"), (args[1:], _ffi.last_error())
            assert raw(cloud, nb, axes, 8, o=None) == -1 and _ffi.last_error().startswith("sf_spin_images:")
            assert lib.sf_spin_images(engine.h, cloud.h, None, axes.ctypes.data, 8, 1, 0, 0.0, 0, 0, out.ctypes.data, None, 0) == -1
            assert _ffi.last_error().startswith("sf_spin_images:")
            assert raw(cloud, nb, axes, 8, 0, 7.0) == 0  # (min_cos is not looked at unless use_min_cos is set)
            for W in (0, 45):
                with pytest.raises(ValueError):
                    nb.spin_images(axes, W)
            with pytest.raises(ValueError):
                nb.spin_images(axes, min_cos=2.0)
            with pytest.raises(ValueError):
                nb.spin_images(axes[:9])
            with pytest.raises(ValueError):
                nb.spin_images(nan_axes)
            assert nb.spin_images(axes).shape == (10, 153) and nb.spin_images(axes, 44).shape == (10, 4005)
            with_normals = np.array(nb.spin_images(axes))
        finally:
            nb.free()
    finally:
        cloud.free()
    bare = engine.cloud(pts)  # positions alone suffice -- until the support angle asks for the normals
    try:
        nb = bare.radius_search(pts[:10], 0.2)
        try:
            assert np.array_equal(bits(np.array(nb.spin_images(axes))), bits(with_normals))
            assert raw(bare, nb, axes, 8, 1, 0.5) == -5 and _ffi.last_error().startswith("sf_spin_images:")
            with pytest.raises(ShotFpfhError, match=r"\(-5\).*normals"):
                nb.spin_images(axes, min_cos=0.5)
        finally:
            nb.free()
    finally:
        bare.free()


def test_public_function_pipeline_and_layered_calls_return_the_same_bits(engine):
    from shot_fpfh_amd.descriptors import compute_spin_image_descriptor
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    pts, nrm = config1_cloud(5000, 2)
    idx = _pick(5000, 200)
    R = 0.12
    rows, _, _ = run(engine, pts, nrm, pts[idx], nrm[idx], R)
    assert np.array_equal(bits(compute_spin_image_descriptor(idx, pts, nrm, R)), bits(rows))
    mask = np.zeros(5000, dtype=bool)
    mask[idx] = True
    assert np.array_equal(bits(compute_spin_image_descriptor(mask, pts, nrm, R, 8, engine=engine)), bits(rows))
    assert np.array_equal(bits(compute_spin_image_descriptor(idx - 5000, pts, nrm, radius=R, image_width=8)), bits(rows))  # negative indices
    opts = dict(signed_beta=False, min_cos=0.4, normalize=True, min_neighborhood_size=20)
    rows4, _, _ = run(engine, pts, nrm, pts[idx[:50]], nrm[idx[:50]], R, 4, **opts)
    assert np.array_equal(bits(compute_spin_image_descriptor(idx[:50], pts, nrm, R, 4, **opts)), bits(rows4)) and rows4.any()

    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(6)
    pipe = RegistrationPipeline(scan=pts @ rot.T, scan_normals=nrm @ rot.T, ref=pts, ref_normals=nrm)
    pipe.scan_keypoints = np.sort(rng.choice(5000, 300, replace=False))
    pipe.ref_keypoints = np.sort(rng.choice(5000, 300, replace=False))
    pipe.compute_descriptors(R, descriptor_choice="spin")  # (the pipeline's default: unsigned, W = 8)
    sd, rd = pipe.scan_descriptors, pipe.ref_descriptors
    assert sd.shape == rd.shape == (300, 81) and sd.any(axis=1).all() and rd.any(axis=1).all()
    assert np.array_equal(bits(rd), bits(compute_spin_image_descriptor(pipe.ref_keypoints, pts, nrm, R, signed_beta=False)))
    pipe.find_descriptors_matches("simple", reject_threshold=0.8, threshold_multiplier=10)
    assert np.array_equal(pipe.matches[0], np.arange(300)) and pipe.matches[1].shape == (300,)
    pipe.compute_descriptors(R, descriptor_choice="spin", spin_width=4, spin_signed=True, force_recompute=True)
    assert pipe.ref_descriptors.shape == (300, 45)
    assert np.array_equal(bits(pipe.ref_descriptors), bits(compute_spin_image_descriptor(pipe.ref_keypoints, pts, nrm, R, 4)))
    pipe.compute_spin_image_descriptor(R, 8, True, force_recompute=True)
    assert np.array_equal(bits(pipe.ref_descriptors), bits(compute_spin_image_descriptor(pipe.ref_keypoints, pts, nrm, R)))
