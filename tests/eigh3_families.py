"""Seeded families of symmetric 3 x 3 matrices for the direct tests of the eigensolver (csrc/eigh3.h, orc_eigh3).

A plain module, like icp_numpy.py: `families()` returns {name: (m, 3, 3) float64}, the same arrays on every call; about
40 000 matrices in all.  Only the LOWER triangle of a matrix is read by any solver under test (numpy's UPLO='L'), and every
matrix here is exactly symmetric.

What LAPACK's dsyevd is for n = 3 holds for max|a| inside DOMAIN (rmin = sqrt(safmin / eps), rmax = sqrt(eps / safmin) with
LAPACK's eps = 2^-52): outside it dsyevd rescales the whole matrix first and neither restatement does.  INSIDE lists the
families that stay within it; `outside` is outside it on purpose and `nonfinite` has no LAPACK answer at all.
"""
import itertools

import numpy as np

DOMAIN = (1.0010415475915505e-146, 9.989595361011175e+145)
INSIDE = ("cov", "psd", "neardeg", "lowrank", "diag", "intsym", "negzero", "realzero", "range", "scaled")
# Families on which LAPACK's column signs are not a function of the matrix alone, so eigenvectors are compared up to sign
# (tests/test_eigh3_host.py).  Exactly structured entries: an exact zero in one build of LAPACK is a last-bit residue in another.
# `range`: the Householder step cancels a graded matrix's large entries and leaves tridiagonal entries with a relative error of
# eps / gap, so the rotation sequence hangs on the BLAS's last bits.  Measured, not supposed: the oracle's own source compiled
# with fused multiply-adds differs from itself in a column sign on 0.6 % of graded, 0.8 % of integer and 0.4 % of zero-pattern
# matrices with a simple spectrum, and on none of 6 000 `cov`, 4 000 `psd`, 1 145 `lowrank`, 360 `neardeg`.
UP_TO_SIGN = ("intsym", "negzero", "realzero", "range")
SCALES_INSIDE = (1e-121, 1e-123, 1e-140, 1e-145, 1e100, 1e145)
SCALES_OUTSIDE = (1e-200, 2.0 ** -1040, 1e153, 3e153, 1e200)
N_SCALED_PSD, N_SCALED_INT = 500, 300  # per scale: the leading `psd` rows, then the leading `intsym` rows

ZERO_PATTERNS = list(itertools.product((False, True), repeat=3))  # which of (a21, a31, a32) are exactly zero


def lower(a):
    """(m, 3, 3) -> (m, 6): a11 a21 a31 a22 a32 a33, the order of sf_eigh3 and of the device call sites."""
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(np.stack([a[:, 0, 0], a[:, 1, 0], a[:, 2, 0], a[:, 1, 1], a[:, 2, 1], a[:, 2, 2]], axis=1))


def _sym(a):
    """Exactly symmetric, from the lower triangle."""
    lo = np.tril(a)
    return lo + np.swapaxes(np.tril(a, -1), -1, -2)


def _rotations(rng, m):
    q, r = np.linalg.qr(rng.standard_normal((m, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _from_spectrum(rng, w):
    q = _rotations(rng, w.shape[0])
    return _sym(np.einsum("mik,mk,mjk->mij", q, w, q))


def _apply_zero_patterns(a):
    """Row i gets pattern i mod 8."""
    a = a.copy()
    for i, (z21, z31, z32) in enumerate(ZERO_PATTERNS):
        for (r, c), z in (((1, 0), z21), ((2, 0), z31), ((2, 1), z32)):
            if z:
                a[i::8, r, c] = 0.0
                a[i::8, c, r] = 0.0
    return a


def _cov(rng, m):
    out = np.empty((m, 3, 3))
    for i in range(m):
        k = int(rng.integers(4, 81))
        p = rng.standard_normal((k, 3)) * (rng.random(3) + 0.01) * 0.05 + rng.standard_normal(3)
        c = p - p.mean(axis=0)
        out[i] = c.T @ c / k
    return _sym(out)


def _neardeg(rng):
    out = []
    for g in 10.0 ** -np.arange(3, 16):
        w = np.tile(np.array([[1.0, 1.0 + g, 2.0], [1.0, 2.0, 2.0 + g]]), (60, 1))
        out.append(_from_spectrum(rng, w))
    return np.concatenate(out)


def _lowrank(rng, m):
    out = np.empty((m, 3, 3))
    for i in range(m):
        k = int(rng.integers(2, 6))
        p = rng.standard_normal((k, 3))
        if i % 4 == 1:  # rank 1: points on a line through a random offset
            p = rng.standard_normal((k, 1)) * rng.standard_normal((1, 3)) + rng.standard_normal(3)
        elif i % 4 == 2:  # a zeroed axis: the covariance has an exact zero row and column
            p[:, int(rng.integers(0, 3))] = 0.0
        elif i % 4 == 3:  # rank 2 (or less): points in a plane
            p = rng.standard_normal((k, 2)) @ rng.standard_normal((2, 3))
        c = p - p.mean(axis=0)
        out[i] = c.T @ c / k
    return _sym(out)


def _diag():
    vals = (0.0, 1.0, 2.0, 3.0, -1.0)
    return np.array([np.diag(d) for d in itertools.product(vals, repeat=3)])


def _intsym(rng, m):
    return _apply_zero_patterns(_sym(rng.integers(-3, 4, (m, 3, 3)).astype(np.float64)))


def _negzero(rng, intsym):
    a = intsym.copy()
    flip = (a == 0.0) & (rng.random(a.shape) < 0.5)
    flip = np.tril(flip) | np.swapaxes(np.tril(flip, -1), -1, -2)
    a[flip] = -0.0
    return a


def _range(rng, m):
    a = _from_spectrum(rng, 10.0 ** rng.uniform(-140.0, 0.0, (m, 3)))
    # block-diagonal matrices with a 2 x 2 sub-block around 1e-130 beside entries of order 1: dsteqr splits them, and the small
    # block's norm is below ssfmin although the matrix is well inside the domain -- the inner down-scaling fires
    nb = m // 2
    blocks = np.zeros((nb, 3, 3))
    s = rng.standard_normal((nb, 2, 2)) * 10.0 ** rng.uniform(-133.0, -127.0, (nb, 1, 1))
    s = np.tril(s) + np.swapaxes(np.tril(s, -1), -1, -2)
    big = rng.standard_normal(nb) + 2.0
    lowpos = np.arange(nb) % 2 == 0  # the small block in rows (2, 3) with a11 of order 1, or in rows (1, 2) with a33 of order 1
    blocks[lowpos, 0, 0] = big[lowpos]
    blocks[lowpos, 1:, 1:] = s[lowpos]
    blocks[~lowpos, 2, 2] = big[~lowpos]
    blocks[~lowpos, :2, :2] = s[~lowpos]
    return np.concatenate([a, blocks])


def _nonfinite(rng, m):
    a = _sym(rng.standard_normal((m, 3, 3)))
    bad = (np.nan, np.inf, -np.inf)
    pos = [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)]
    for i in range(m):
        for _ in range(1 + i % 2):
            r, c = pos[int(rng.integers(0, 6))]
            a[i, r, c] = a[i, c, r] = bad[int(rng.integers(0, 3))]
    return a


_CACHE = None


def families():
    """{name: (m, 3, 3)} in a fixed order; built once per process and returned read-only."""
    global _CACHE
    if _CACHE is not None:
        return _CACHE
    rng = np.random.default_rng(20260)
    f = {}
    f["cov"] = _cov(rng, 6000)
    # (largest eigenvalue in [0.5, 1): max|a| = the largest diagonal entry is in [1/6, 1), so every scale of `scaled` stays inside)
    f["psd"] = _from_spectrum(rng, rng.random((4000, 3)) * np.array([0.25, 0.5, 0.5]) + np.array([0.0, 0.0, 0.5]))
    f["neardeg"] = _neardeg(rng)
    f["lowrank"] = _lowrank(rng, 2000)
    f["diag"] = _diag()
    f["intsym"] = _intsym(rng, 4000)
    f["negzero"] = _negzero(rng, f["intsym"][:2000])
    f["realzero"] = _apply_zero_patterns(_sym(rng.standard_normal((4000, 3, 3))))
    f["range"] = _range(rng, 2000)
    base = np.concatenate([f["psd"][:N_SCALED_PSD], f["intsym"][:N_SCALED_INT]])
    f["scaled"] = np.concatenate([base * s for s in SCALES_INSIDE])
    f["outside"] = np.concatenate([base * s for s in SCALES_OUTSIDE])
    f["nonfinite"] = _nonfinite(rng, 3000)
    for name, a in f.items():
        assert a.ndim == 3 and a.shape[1:] == (3, 3) and a.dtype == np.float64, name
        if name != "nonfinite":
            assert np.array_equal(a, np.swapaxes(a, 1, 2)), name
        a.setflags(write=False)
    for name in INSIDE:
        big = np.abs(f[name]).max(axis=(1, 2))
        assert np.all((big == 0.0) | ((big >= DOMAIN[0]) & (big <= DOMAIN[1]))), name
    big = np.abs(f["outside"]).max(axis=(1, 2))
    assert np.all((big == 0.0) | (big < DOMAIN[0]) | (big > DOMAIN[1]))
    _CACHE = f
    return f


def scaled_is_structured():
    """Mask over `scaled` (and `outside`): True where the row comes from `intsym`."""
    one = np.r_[np.zeros(N_SCALED_PSD, bool), np.ones(N_SCALED_INT, bool)]
    return np.tile(one, len(SCALES_INSIDE))


def all_matrices(names=None):
    """(concatenated (M, 3, 3), {name: slice})."""
    f = families()
    names = list(f) if names is None else list(names)
    slices, at = {}, 0
    for n in names:
        slices[n] = slice(at, at + f[n].shape[0])
        at += f[n].shape[0]
    return np.concatenate([f[n] for n in names]), slices
