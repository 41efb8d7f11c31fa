"""sf_eigh3 -- csrc/eigh3.h's eigh3_lower called from a kernel exactly as K3, K4 and the ISS saliency call it -- against the
oracle's orc_eigh3, bit for bit, on every family of tests/eigh3_families.py in ONE launch; batch shapes around the wave and the
block; the call sites against the hook; argument errors.

The host build of the same header equals the oracle bit for bit (tests/test_eigh3_host.py), so a difference here is not the
logic: it is an operation the device rounds differently (float64 sqrt and division are correctly rounded on gfx950 and
contraction is off).

"Bit for bit" on a NaN means a NaN in the same place: its sign and payload are not values (IEEE 754 leaves them to the
implementation; the default NaN of an x86 division is the negative one, the GPU's the positive one).  Every other output --
zeros' signs and infinities included -- has to have the same bit pattern.
"""
import ctypes as C

import numpy as np
import pytest

import eigh3_families as F
from conftest import synth_cloud

pytestmark = pytest.mark.gpu

SHAPES = (1, 63, 64, 65, 255, 256, 257)


def same_bits(x, y):
    """Elementwise: the same bit pattern, or a NaN in both."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def rows_equal(w1, v1, w2, v2):
    return same_bits(w1, w2).all(axis=1) & same_bits(v1, v2).all(axis=(1, 2))


def has_nonfinite(w, v):
    return (~np.isfinite(w)).any(axis=1) | (~np.isfinite(v)).any(axis=(1, 2))


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


@pytest.fixture(scope="module")
def everything(eng):
    """All families end to end, the oracle on them, and the device on them in one call."""
    from oracle import oracle as O

    a, slices = F.all_matrices()
    return a, slices, O.eigh3_batch(a), eng.eigh3(a)


def mixed_batch(m):
    """m matrices in which neighbouring lanes take different paths: generic covariances (QL beside QR, by which end of the
    diagonal is larger), zero patterns (a31 = 0: no reflector; a split into 1 + 2: the 2 x 2 exit beside full steps), blocks
    scaled down (1e-140: the ssfmin branch) and up (1e200: ssfmax) beside unscaled ones, diagonal ones (no iteration at all)."""
    f = F.families()
    src = [f["cov"], f["realzero"], f["scaled"][2 * 800:3 * 800], f["range"][2000:], f["outside"][4 * 800:], f["diag"]]
    return np.ascontiguousarray(np.stack([src[i % 6][(i // 6) % src[i % 6].shape[0]] for i in range(m)]))


@pytest.fixture(scope="module")
def alone(eng):
    """Every matrix of the mixed batch solved alone: a launch of one lane each."""
    a = mixed_batch(max(SHAPES))
    w, v = zip(*(eng.eigh3(a[i:i + 1]) for i in range(a.shape[0])))
    return a, np.concatenate(w), np.concatenate(v)


def device_call(eng, a):
    """sf_eigh3 with device pointers in and out."""
    from shot_fpfh_amd import _ffi

    lower = F.lower(a)
    m = lower.shape[0]
    d_in, d_w, d_v = eng.empty((m, 6)).from_host(lower), eng.empty((m, 3)), eng.empty((m, 3, 3))
    try:
        _ffi.check(eng.lib.sf_eigh3(eng.h, d_in.ptr, m, d_w.ptr, d_v.ptr, _ffi.SF_IN_DEVICE | _ffi.SF_OUT_DEVICE), "sf_eigh3")
        return d_w.to_host(), d_v.to_host()
    finally:
        for d in (d_in, d_w, d_v):
            d.free()


def test_device_equals_the_oracle_bit_for_bit_on_every_family(everything):
    a, slices, (wo, vo), (w, v) = everything
    assert 35_000 <= a.shape[0] <= 45_000
    counts, strict = {}, {}
    for name, sl in slices.items():
        if name == "nonfinite":  # fmax and an `if` treat NaN differently: only "both return, something is non-finite"
            counts[name] = (int((has_nonfinite(w[sl], v[sl]) & has_nonfinite(wo[sl], vo[sl])).sum()), sl.stop - sl.start)
            continue
        counts[name] = (int(rows_equal(w[sl], v[sl], wo[sl], vo[sl]).sum()), sl.stop - sl.start)
        strict[name] = int(((w[sl].view(np.uint64) == wo[sl].view(np.uint64)).all(axis=1)
                            & (v[sl].view(np.uint64) == vo[sl].view(np.uint64)).all(axis=(1, 2))).sum())
    print("device == oracle, bit for bit (nonfinite: both have a non-finite output):", counts)
    print("... counting a NaN's sign and payload too:", strict)
    assert all(got == m for got, m in counts.values()), counts


@pytest.mark.parametrize("m", SHAPES)
def test_every_row_of_a_batch_equals_the_matrix_solved_alone(eng, alone, m):
    a, w1, v1 = alone
    for w, v in (eng.eigh3(a[:m]), device_call(eng, a[:m])):
        assert w.shape == (m, 3) and v.shape == (m, 3, 3)
        assert rows_equal(w, v, w1[:m], v1[:m]).all()


def test_the_mixed_batch_mixes_and_equals_the_oracle(alone):
    from oracle import oracle as O

    a, w1, v1 = alone
    wo, vo = O.eigh3_batch(a)
    assert rows_equal(w1, v1, wo, vo).all()
    big = np.abs(a).max(axis=(1, 2))
    assert (big[:64] < 1e-130).any() and (big[:64] > 1e190).any() and (a[:64, 2, 0] == 0.0).any() and (a[:64, 2, 0] != 0.0).any()


def test_seventy_thousand_lanes(eng, everything):
    a, slices, _, (w_all, v_all) = everything
    cov = a[slices["cov"]]
    reps = -(-70_000 // cov.shape[0])
    big = np.ascontiguousarray(np.tile(cov, (reps, 1, 1))[:70_000])
    w_ref = np.tile(w_all[slices["cov"]], (reps, 1))[:70_000]
    v_ref = np.tile(v_all[slices["cov"]], (reps, 1, 1))[:70_000]
    for w, v in (eng.eigh3(big), device_call(eng, big)):
        assert rows_equal(w, v, w_ref, v_ref).all()


def test_a_nonfinite_matrix_leaves_its_neighbours_alone(eng, alone):
    a, w1, v1 = alone
    a = a[:257].copy()
    bad = [0, 63, 64]
    a[bad] = F.families()["nonfinite"][:3]
    w, v = eng.eigh3(a)
    keep = np.ones(257, bool)
    keep[bad] = False
    assert has_nonfinite(w[bad], v[bad]).all()
    assert rows_equal(w[keep], v[keep], w1[:257][keep], v1[:257][keep]).all()


def test_the_call_sites_agree_with_the_hook(eng):
    """K3's decomposition of every neighbourhood of a small cloud against sf_eigh3 on the covariance rebuilt on the host from the
    exported lists: guards the argument order (a11, a21, a31, a22, a32, a33) at the call sites.  Not a bit-level check: the
    host's covariance sums in another order."""
    from shot_fpfh_amd.descriptors import compute_local_pca_with_moments

    p, _, _ = synth_cloud(2000, 77)
    radius = 0.168  # 4/3 pi r^3 x 2000 = 40 neighbours in the unit cube
    w, v, _, sizes = compute_local_pca_with_moments(p, p, radius=radius)
    cloud = eng.cloud(p)
    nb = cloud.radius_search(p, radius)
    off, idx = nb.export()
    nb.free()
    cloud.free()
    assert np.array_equal(np.diff(off), sizes) and 15 < np.mean(sizes) < 45  # (fewer than 40 near the cube's faces)
    cov = np.empty((p.shape[0], 3, 3))
    for i in range(p.shape[0]):
        c = p[idx[off[i]:off[i + 1]]]
        c = c - c.mean(axis=0)
        cov[i] = c.T @ c / c.shape[0]
    w2, v2 = eng.eigh3(cov)
    big = np.abs(w2).max(axis=1)
    assert np.all(np.abs(w - w2).max(axis=1) <= 1e-12 * big)
    gap = np.minimum(w2[:, 1] - w2[:, 0], w2[:, 2] - w2[:, 1]) / big
    simple = gap > 1e-6
    assert simple.sum() > 1900
    assert np.all((np.abs(v - v2).max(axis=(1, 2)) * gap)[simple] <= 1e-9)


def test_argument_errors_name_the_argument_and_the_context_lives_on(eng):
    from shot_fpfh_amd import ShotFpfhError, _ffi

    lower, w, v = np.zeros((2, 6)), np.zeros((2, 3)), np.zeros((2, 3, 3))
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args, word in (((None, 2, p(w), p(v)), "null lower"), ((p(lower), 2, None, p(v)), "null w"), ((p(lower), 2, p(w), None), "null v"),
                       ((p(lower), -1, p(w), p(v)), "m < 0")):
        with pytest.raises(ShotFpfhError, match="sf_eigh3: " + word):
            _ffi.check(eng.lib.sf_eigh3(eng.h, *args, _ffi.SF_HOST), "sf_eigh3")
    with pytest.raises(ShotFpfhError, match="sf_eigh3: null ctx"):
        _ffi.check(eng.lib.sf_eigh3(None, p(lower), 2, p(w), p(v), _ffi.SF_HOST), "sf_eigh3")
    with pytest.raises(ValueError):
        eng.eigh3(np.zeros((3, 3)))
    w0, v0 = eng.eigh3(np.zeros((0, 3, 3)))
    assert w0.shape == (0, 3) and v0.shape == (0, 3, 3)
    w1, v1 = eng.eigh3(np.diag([3.0, 1.0, 2.0])[None])
    w_np, v_np = np.linalg.eigh(np.diag([3.0, 1.0, 2.0]))
    assert np.array_equal(w1[0], w_np) and np.array_equal(v1[0], v_np)
