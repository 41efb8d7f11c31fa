"""Point-to-point and point-to-plane ICP without a GPU: the NumPy statement of one pass (tests/icp_numpy.py) against formulations
it does not use itself, its layout against what shot_fpfh_amd.icp reads, every condition tests/test_hip_icp_sums.py places on
its inputs (same generators, same seeds -- so that file cannot fail because of an input), and the row validation of
`_Registration.pairs`."""
import numpy as np
import pytest

import gicp_numpy as G
import icp_numpy as I
import test_hip_icp_sums as T
from test_hip_gicp import assert_unambiguous, one_pass_set

U = 2.0**-53


def pairs_at_the_true_motion(k_rows=400):
    s = one_pass_set()
    label, R, t = s["states"][1]
    a = s["scan"][:k_rows]
    p, idx, d, d2 = I.kept_pairs(a, s["ref"], R, t, T.D_MAX, s["tree"])
    assert 200 < p.shape[0] < k_rows  # a few hundred pairs, and the filter drops some
    return s, a, R, t, p, s["ref"][idx], s["nref"][idx]


def within(got, want, k, mags, c):
    return np.all(np.abs(np.asarray(got) - np.asarray(want)) <= c * k * U * np.asarray(mags))


# ---- the statement against independent formulations ----------------------------------------------------------------------------------
def test_plane_terms_are_the_normal_equations():
    """G = hstack([cross(p, n), n]), G^T G, G^T h with h = (q - p) . n: core/solvers.py:38-46, restated here."""
    s, a, R, t, p, q, n = pairs_at_the_true_motion()
    want = I.sums(a, s["ref"], s["nref"], R, t, T.D_MAX, I.PLANE, tree=s["tree"])
    k, c = want["count"], T.C_ROUNDINGS[I.PLANE]
    assert k == p.shape[0]
    count, sp, sq, gtg, gth, abs_h = I.unpack(want["vec"], I.PLANE)
    _c, _sp, _sq, gtg_mag, gth_mag, abs_mag = I.unpack(want["abs"], I.PLANE)
    Gm = np.hstack([np.cross(p, n), n])
    h = np.einsum("ij,ij->i", q - p, n)
    assert count == k and within(sp, p.sum(axis=0), k, np.abs(p).sum(axis=0), c) and within(sq, q.sum(axis=0), k, np.abs(q).sum(axis=0), c)
    assert within(gtg, Gm.T @ Gm, k, gtg_mag, c) and np.array_equal(gtg, gtg.T)
    assert within(gth, Gm.T @ h, k, gth_mag, c)
    assert within(abs_h, np.abs(h).sum(), k, abs_mag, c)
    assert not want["vec"][I.UNUSED[I.PLANE]].any() and not want["abs"][I.UNUSED[I.PLANE]].any()


def test_point_terms_are_the_centred_cross_covariance():
    s, a, R, t, p, q, n = pairs_at_the_true_motion()
    want = I.sums(a, s["ref"], None, R, t, T.D_MAX, I.POINT, tree=s["tree"])
    k, c = want["count"], T.C_ROUNDINGS[I.POINT]
    count, sp, sq, cov, sq_dist = I.unpack(want["vec"], I.POINT)
    _c, _sp, _sq, cov_mag, d2_mag = I.unpack(want["abs"], I.POINT)
    assert count == k == p.shape[0]
    assert within(cov, (p - p.mean(0)).T @ (q - q.mean(0)), k, cov_mag, c)
    assert within(sq_dist, ((q - p) ** 2).sum(), k, d2_mag, c)
    assert not want["vec"][I.UNUSED[I.POINT]].any() and not want["abs"][I.UNUSED[I.POINT]].any()


def test_inexact_centroids_enter_the_centred_form_to_second_order():
    """sum (p - pm)(q - qm)^T = sum (p - pbar)(q - qbar)^T + k (pbar - pm)(qbar - qm)^T, on a cloud 1000 from the origin on every
    axis and with centroids that are off by ~1e-5 (rounded to float32).  The first-order terms vanish because the exactly centred
    factors sum to zero -- which is why the device's two-pass form, centred with its own rounded centroids (off by ~k 2^-53 1000),
    may be held to a bound made of the centred magnitudes at any offset."""
    f = T.far_set()
    label, which, R, t = f["states"][1]
    a = f[which][:400]
    p, idx, d, d2 = I.kept_pairs(a, f["ref"], R, t, T.D_MAX, f["tree"])
    q = f["ref"][idx]
    k, c = p.shape[0], T.C_ROUNDINGS[I.POINT]
    assert k > 200 and p.min() > 990
    exact = I.centroids(p, q)
    rough = exact.astype(np.float32).astype(np.float64)
    assert 1e-7 < np.abs(rough - exact).max() < 1e-4
    def cov(means):
        tm, mg = I.terms(a, f["ref"], None, R, t, T.D_MAX, I.POINT, means, f["tree"])
        return G.fsum_cols(tm)[8:17].reshape(3, 3), mg.sum(axis=0)[8:17].reshape(3, 3)
    c_rough, m_rough = cov(rough)
    c_exact, m_exact = cov(exact)
    second = k * np.outer(exact[:3] - rough[:3], exact[3:] - rough[3:])
    # each side: terms rounded once (a subtraction and a product, 2 roundings relative to |term|), the sums exact; the centroid
    # `exact` itself is pbar rounded once, which moves the right side by another k 2^-53 1000 * |sum of centred q| -- second order again
    assert np.all(np.abs(c_rough - (c_exact + second)) <= c * k * U * (m_rough + m_exact))
    # and with the centroids as far off as a float64 accumulation can leave them, the second-order term is below one rounding
    delta = c * k * U * np.abs(np.hstack([p, q])).max()
    assert k * delta * delta <= U * m_exact.min()


def test_layout_is_what_pair_sums_reads():
    from shot_fpfh_amd.icp import _PLANE, _POINT, _PairSums

    assert (_POINT, _PLANE) == (I.POINT, I.PLANE)
    s, a, R, t, p, q, n = pairs_at_the_true_motion()
    k = p.shape[0]
    point = _PairSums(I.sums(a, s["ref"], None, R, t, T.D_MAX, I.POINT, tree=s["tree"])["vec"], _POINT)
    assert point.count == k and np.allclose(point.sum_p, p.sum(0), rtol=1e-12) and np.allclose(point.sum_q, q.sum(0), rtol=1e-12)
    want = (p - p.mean(0)).T @ (q - q.mean(0))
    assert not np.allclose(want, want.T, rtol=1e-3)  # (a transposed layout would show)
    assert np.allclose(point.cross_cov, want, rtol=0, atol=1e-12 * np.abs(want).max())
    assert np.isclose(point.sq_dist, ((q - p) ** 2).sum(), rtol=1e-12)
    plane = _PairSums(I.sums(a, s["ref"], s["nref"], R, t, T.D_MAX, I.PLANE, tree=s["tree"])["vec"], _PLANE)
    Gm = np.hstack([np.cross(p, n), n])
    h = np.einsum("ij,ij->i", q - p, n)
    assert plane.count == k and np.array_equal(plane.gtg, plane.gtg.T)
    assert np.allclose(plane.gtg, Gm.T @ Gm, rtol=0, atol=1e-12 * np.abs(Gm.T @ Gm).max())
    assert np.allclose(plane.gth, Gm.T @ h, rtol=0, atol=1e-12 * np.abs(Gm.T @ h).max())
    assert np.isclose(plane.abs_h, np.abs(h).sum(), rtol=1e-12)
    with pytest.raises(np.linalg.LinAlgError):
        _PairSums(np.zeros(40), _POINT).require_pairs()


def test_statement_loop_composes_like_the_product():
    """`refine` composes and fits as shot_fpfh_amd.icp does: RigidTransform.__matmul__, kabsch_from_covariance, _plane_fit."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.core.geometry import kabsch_from_covariance
    from shot_fpfh_amd.icp import _PLANE, _PairSums, _plane_fit

    rng = np.random.default_rng(3)
    R, t = G.true_motion()
    dR, dt = G.rodrigues(np.array([0.01, -0.02, 0.03])), np.array([0.1, 0.2, -0.3])
    want = RigidTransform(dR, dt) @ RigidTransform(R, t)
    got = I.compose(dR, dt, R, t)
    assert np.array_equal(got[0], want.rotation) and np.array_equal(got[1], want.translation)
    for flip in (1.0, -1.0):  # the second covariance is a reflection's: the rule of the last singular direction
        cov = (rng.standard_normal((3, 3)) + 3 * np.eye(3)) @ np.diag([1.0, 1.0, flip])
        pb, qb = rng.random(3), rng.random(3)
        want = kabsch_from_covariance(cov, pb, qb)
        got = I.kabsch(cov, pb, qb)
        assert np.array_equal(got[0], want.rotation) and np.array_equal(got[1], want.translation) and np.linalg.det(got[0]) > 0
    s, a, Rm, tm, p, q, n = pairs_at_the_true_motion()
    vec = I.sums(a, s["ref"], s["nref"], Rm, tm, T.D_MAX, I.PLANE, tree=s["tree"])["vec"]
    count, sp, sq, gtg, gth, abs_h = I.unpack(vec, I.PLANE)
    from scipy.spatial.transform import Rotation

    sol = np.linalg.solve(gtg, gth)
    want = _plane_fit(_PairSums(vec, _PLANE))
    assert np.array_equal(want.rotation, Rotation.from_euler("xyz", sol[:3]).as_matrix()) and np.array_equal(want.translation, sol[3:6])


# ---- the conditions the GPU tests place on their inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("m", T.M_SIZES)
def test_one_pass_inputs_are_unambiguous(m):
    s = one_pass_set()
    a = s["scan"][:m]
    for label, R, t in s["states"]:
        assert_unambiguous(s, a, R, t, T.D_MAX, (m, label))
    if m == 1:  # the single pair IS kept at the true motion (the bound is not vacuous there)
        label, R, t = s["states"][1]
        assert I.kept_pairs(a, s["ref"], R, t, T.D_MAX, s["tree"])[0].shape[0] == 1
    if m == max(T.M_SIZES):  # every state keeps pairs, and none keeps all of them
        for label, R, t in s["states"]:
            assert 1000 < I.kept_pairs(a, s["ref"], R, t, T.D_MAX, s["tree"])[0].shape[0] < m, label


def test_selection_far_and_edge_inputs():
    s = one_pass_set()
    a, ids = s["scan"][:5000], T.selection_ids()
    assert ids.shape == (777,) and np.unique(ids).size < 777 and ids.min() >= 0 and ids.max() < 5000
    label, R, t = s["states"][1]
    for pts in (a[ids], a):
        for R2, t2 in ((R, t), (None, None)):
            # (repeated ids are the same point twice: the nearest / second-nearest condition is per row and still holds)
            assert_unambiguous(s, pts, R2, t2, T.D_MAX, "selection")
    assert_unambiguous(s, a, R, t, np.inf, "inf")
    assert I.kept_pairs(a, s["ref"], R, t, T.D_MAX, s["tree"])[0].shape[0] > 2500
    assert I.kept_pairs(a, s["ref"], R, t, T.NO_PAIR_RADIUS, s["tree"])[0].shape[0] == 0  # the "no pair" radius
    assert I.kept_pairs(a, s["ref"], R, t, np.inf, s["tree"])[0].shape[0] == 5000
    for d_max in (float("nan"), -1.0):
        w = I.sums(a, s["ref"], s["nref"], R, t, d_max, I.PLANE, tree=s["tree"])
        assert w["count"] == 0 and not w["vec"].any()
    f = T.far_set()
    for label, which, R2, t2 in f["states"]:
        assert G.move(R2, t2, f[which]).min() > 990
        assert_unambiguous(f, f[which], R2, t2, T.D_MAX, ("far", label))
        assert I.kept_pairs(f[which], f["ref"], R2, t2, T.D_MAX, f["tree"])[0].shape[0] > 2500


def test_lattice_distances_are_exact():
    L = T.lattice_set()
    assert L["ref"].shape == (512, 3) and T.LATTICE_R == 0.0390625
    for name, on in (("off", 0), ("mixed", L["on_lattice"])):
        for R, t in ((None, None), (np.eye(3), np.zeros(3))):
            p = G.move(R, t, L[name])
            assert np.array_equal(p, L[name])  # the identity as an explicit transform is exact
            d = L["tree"].query(p, k=2)[0]
            assert np.all(d[:, 1] - d[:, 0] > 0.01)  # the nearest lattice point is not a matter of rounding
            idx, d2 = G.nearest(p, L["ref"], L["tree"])
            assert np.array_equal(idx, np.arange(512))
            assert set(np.unique(d2)) == ({25 * 2.0**-14} if on == 0 else {0.0, 25 * 2.0**-14})
            assert set(np.unique(np.sqrt(d2))) <= {0.0, T.LATTICE_R} and T.LATTICE_R * T.LATTICE_R == 25 * 2.0**-14
            below = float(np.nextafter(T.LATTICE_R, 0.0))
            assert below < T.LATTICE_R
            for d_max, want in ((T.LATTICE_R, 512), (below, on), (0.0, on)):
                assert I.kept_pairs(L[name], L["ref"], R, t, d_max, L["tree"])[0].shape[0] == want
    assert L["on_lattice"] == 103


def test_square_root_cases_drop_exactly_one_pair():
    s = one_pass_set()
    a, R, t, radii = T.sqrt_cases()
    assert radii.shape == (16,) and np.all(np.diff(radii) > 0) and radii[0] < 0.01 < 0.04 < radii[-1]
    for r in radii:
        assert float(r) * float(r) != G.nearest(G.move(R, t, a), s["ref"], s["tree"])[1].min()  # (not the trivial pair)
        at = I.kept_pairs(a, s["ref"], R, t, float(r), s["tree"])[0].shape[0]
        below = I.kept_pairs(a, s["ref"], R, t, float(np.nextafter(r, 0.0)), s["tree"])[0].shape[0]
        assert at - below == 1 and below >= 9
    d2 = G.nearest(G.move(R, t, a), s["ref"], s["tree"])[1]
    roots = np.sqrt(d2)
    assert np.count_nonzero(roots * roots != d2) > 2000  # these are not perfect squares: the rounding of sqrt decides


def test_changed_normals_and_surface_inputs():
    new = T.changed_normals()
    length = np.linalg.norm(new, axis=1)
    assert np.count_nonzero(length == 0) == len(range(0, 2000, 9)) and length.max() > 2 and 0 < length[length > 0].min() < 0.5
    assert np.count_nonzero(np.abs(length - 1) < 1e-12) > 1500
    f = T.surface_set()
    assert f["scan"].shape == (T.SURFACE_ROWS, 3) and T.SURFACE_ROWS >= 2 * 2048  # 2 * SF_K2_SAMPLE (csrc/search_util.h)
    d = f["tree"].query(f["scan"], k=1)[0]
    assert np.count_nonzero(d > 2 * f["diag"]) == T.SURFACE_FAR and np.count_nonzero(d < 0.05) == T.SURFACE_ROWS - T.SURFACE_FAR
    assert_unambiguous(f, f["scan"], None, None, np.inf, "surface")
    # the far rows are spread over the scan, not a block at its end
    assert np.flatnonzero(d > 1).min() < 200 and np.flatnonzero(d > 1).max() > T.SURFACE_ROWS - 200


@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_whole_run_stop_is_not_a_matter_of_rounding(mode):
    scan, ref, nref, r0, t0 = T.corner_run_set()
    n_it = T.RUN_ITERATIONS[mode]
    run = I.refine(scan, ref, nref, mode, T.RUN_D_MAX, max_iter=n_it, rms_threshold=0.0)
    trace = np.array(run["rms_trace"])
    assert run["iterations"] == n_it and not run["converged"] and min(run["counts"]) > 1000
    # no residual is a hundredth of the one before: no threshold has the last rms 10 x below and the one before 10 x above
    assert np.all(trace[1:] * 100 > trace[:-1])
    # the rms stop that IS run: between two residuals at least 5 % apart
    thr, k = T.stop_threshold(trace, mode), T.STOP_AFTER[mode]
    assert trace[k - 1] * 1.05 < trace[k - 2] and trace[k - 1] * 1.02 < thr < trace[k - 2] / 1.02
    stopped = I.refine(scan, ref, nref, mode, T.RUN_D_MAX, max_iter=n_it, rms_threshold=thr)
    assert stopped["converged"] and stopped["iterations"] == k
    assert G.rotation_error(run["R"], r0) < (2e-2 if mode == I.POINT else 2e-3)


# ---- the row validation of _Registration.pairs ---------------------------------------------------------------------------------------
def test_row_selection_is_validated_on_the_host():
    from shot_fpfh_amd.icp import _checked_rows

    ok = _checked_rows([4, 0, 4, 9], 10)
    assert ok.dtype == np.int64 and ok.flags.c_contiguous and ok.tolist() == [4, 0, 4, 9]
    assert _checked_rows(np.arange(10, dtype=np.int32)[::2], 10).tolist() == [0, 2, 4, 6, 8]
    for empty in ([], np.zeros(0, dtype=np.int64), np.zeros(0)):
        got = _checked_rows(empty, 10)
        assert got.shape == (0,) and got.dtype == np.int64
    assert _checked_rows([], 0).shape == (0,)
    for bad, value, n in (([0, 10], 10, 10), ([3, -1, 2], -1, 10), (np.array([2**40]), 2**40, 10),
                          (np.array([2**63], dtype=np.uint64), 2**63, 10), ([0], 0, 0)):
        with pytest.raises(IndexError, match=rf"= {value} "):
            _checked_rows(bad, n)
    with pytest.raises(ValueError):
        _checked_rows(np.zeros((2, 2), dtype=np.int64), 10)
    with pytest.raises(TypeError):
        _checked_rows(np.array([1.0, 2.0]), 10)
    with pytest.raises(TypeError):
        _checked_rows(np.array([True, False]), 10)


def test_pairs_checks_rows_before_any_device_call():
    """`pairs(rows=...)` with an id out of range raises before it touches the engine (the registration here has none)."""
    from shot_fpfh_amd.icp import _POINT, _Registration

    reg = object.__new__(_Registration)
    reg.n, reg.rows, reg.engine = 10, None, None
    for bad in ([10], [-1], [0, 3, 11]):
        with pytest.raises(IndexError):
            reg.pairs(_POINT, 0.1, rows=bad)


# ---- a CPU transcription of k_icp_sums: the bound passes the kernel as written and fails it when it is subtly wrong ----------------
def transcribed_call(a, ref, nref, R, t, d_max, mode, tree, wrong=None):
    """sf_icp_accumulate as csrc/icp.hip performs it, in NumPy: the terms of k_icp_sums per pair (every weight 1.0), then ITS order of additions --
    thread i + 65 536 j serially, the xor butterfly over the 64 lanes of a wave, ((w0 + w1) + w2) + w3 per block, the 256 block
    partials one after the other, the centroids of k_icp_means in between.  `wrong` breaks one thing the way a slip in the kernel
    would: "sign" (px nz - pz nx for g[1]), "uncentred" (products of uncentred factors, k pbar qbar^T taken off at the end),
    "strict" (`<` for `<=` in the distance test)."""
    p = G.move(R, t, np.asarray(a, dtype=np.float64))
    idx, d2 = G.nearest(p, ref, tree)
    with np.errstate(invalid="ignore"):
        keep = np.sqrt(d2) < d_max if wrong == "strict" else np.sqrt(d2) <= d_max
    m = p.shape[0]

    def fold(cols):  # (m, nv) terms, zero where the pair is dropped -> nv sums in the device's order
        x = np.where(keep[:, None], cols, 0.0)
        acc = np.zeros((65536, x.shape[1]))
        for first in range(0, m, 65536):
            part = x[first:first + 65536]
            acc[:part.shape[0]] += part
        lanes = acc.reshape(256, 4, 64, -1)
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, :, np.arange(64) ^ off]
        waves = lanes[:, :, 0]
        blocks = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
        out = np.zeros(x.shape[1])
        for b in range(256):
            out = out + blocks[b]
        return out

    q = ref[idx]
    raw = np.zeros(40)
    raw[:7] = fold(np.hstack([np.ones((m, 1)), p, q]))
    d = q - p
    if mode == I.POINT:
        mean = raw[1:7] / raw[0] if raw[0] > 0 else np.zeros(6)
        if wrong == "uncentred":
            cov = fold(np.stack([p[:, i] * q[:, j] for i in range(3) for j in range(3)], axis=1))
            raw[8:17] = cov - raw[0] * np.outer(mean[:3], mean[3:]).reshape(9)
        else:
            av, bv = p - mean[:3], q - mean[3:]
            raw[8:17] = fold(np.stack([av[:, i] * bv[:, j] for i in range(3) for j in range(3)], axis=1))
        raw[17] = fold(d2[:, None])[0]
        return raw
    n = nref[idx]
    px, py, pz, nx, ny, nz = p[:, 0], p[:, 1], p[:, 2], n[:, 0], n[:, 1], n[:, 2]
    g = [py * nz - pz * ny, (px * nz - pz * nx) if wrong == "sign" else (pz * nx - px * nz), px * ny - py * nx, nx, ny, nz]
    h = (d[:, 0] * nx + d[:, 1] * ny) + d[:, 2] * nz
    raw[8:36] = fold(np.stack([g[i] * g[j] for i, j in I.TRIU] + [g[i] * h for i in range(6)] + [np.abs(h)], axis=1))
    return raw


def test_the_bound_passes_the_kernel_as_written_and_fails_a_subtly_wrong_one():
    s = one_pass_set()
    for m in (65, 65537):
        a = s["scan"][:m]
        for label, R, t in s["states"][:2]:
            for mode in (I.POINT, I.PLANE):
                got = transcribed_call(a, s["ref"], s["nref"], R, t, T.D_MAX, mode, s["tree"])
                T.check_sums(got, a, s["ref"], s["nref"], R, t, T.D_MAX, mode, f"transcription mode {mode} m={m} {label}", s["tree"])
    label, R, t = s["states"][1]
    a = s["scan"][:257]
    with pytest.raises(AssertionError):  # one sign in g: G^T G's second row and column, G^T h's second entry
        T.check_sums(transcribed_call(a, s["ref"], s["nref"], R, t, T.D_MAX, I.PLANE, s["tree"], "sign"), a, s["ref"], s["nref"], R, t,
                     T.D_MAX, I.PLANE, "wrong sign", s["tree"])
    f = T.far_set()
    label, which, R, t = f["states"][1]
    good = transcribed_call(f[which], f["ref"], None, R, t, T.D_MAX, I.POINT, f["tree"])
    T.check_sums(good, f[which], f["ref"], None, R, t, T.D_MAX, I.POINT, "transcription +1000", f["tree"])
    with pytest.raises(AssertionError):  # no centring: the cancellation of 1e6-sized products shows against the centred magnitudes
        T.check_sums(transcribed_call(f[which], f["ref"], None, R, t, T.D_MAX, I.POINT, f["tree"], "uncentred"), f[which], f["ref"], None,
                     R, t, T.D_MAX, I.POINT, "uncentred", f["tree"])
    L = T.lattice_set()
    assert transcribed_call(L["off"], L["ref"], L["nref"], None, None, T.LATTICE_R, I.POINT, L["tree"])[0] == 512
    assert transcribed_call(L["off"], L["ref"], L["nref"], None, None, T.LATTICE_R, I.POINT, L["tree"], "strict")[0] == 0  # `<` for `<=`
