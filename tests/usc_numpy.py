"""The NumPy statement of Unique Shape Context (K21): what tests/test_usc_host.py checks against closed forms and
tests/test_hip_usc.py holds the device to, bit for bit.  Modelled on pcl::UniqueShapeContext, decided here so that no bin
decision depends on a transcendental function: the tables are computed once (by the library, sf_usc_tables -- `tables`; their
NumPy formulas are `tables_numpy`) and a neighbour is binned by comparisons against them.

Parameters: radius R; min_radius r0 (default R / 10, 0 < r0 < R); density_radius (default R / 5); azimuth_bins L (even, >= 2,
default 14); elevation_bins K (>= 1, 14); radius_bins J (>= 1, 10); D = L K J <= 4096; bin (l, k, j) at (l K + k) J + j.

Tables:  e[j] = exp(log r0 + (j / J) log(R / r0)), e[0] = r0 and e[J] = R exactly, e2 = e e
         ca[i], sa[i] = cos, sin(2 pi i / L), i < L / 2
         ct[i] = cos(pi i / K), ct[0] = 1, ct[K] = -1, ct[K / 2] = 0 (K even) exactly, q = ct |ct|
         vol[b] = 1 / cbrt((2 pi / L) (ct[k] - ct[k + 1]) (e[j + 1]^3 - e[j]^3) / 3)
Neighbour t of keypoint i, frame F (3 x 3, columns x y z as sf_shot_lrf lays them out), unfused float64 in this order:
         d = p_t - q_i;  r2 = (dx dx + dy dy) + dz dz, skipped when r2 == 0
         lx = (dx F[0, 0] + dy F[1, 0]) + dz F[2, 0], ly and lz with columns 1 and 2
         j = #{1 <= i < J : r2 >= e2[i]}
         h = ly < 0 or (ly == 0 and lx < 0);  (u, v) = (-lx, -ly) if h else (lx, ly)
         l = #{1 <= i < L / 2 : ca[i] v - sa[i] u >= 0} + h L / 2
         k = #{1 <= i < K : lz |lz| <= q[i] r2}
         w = 1.0 / c_t, c_t = number of cloud points within density_radius of p_t, itself included (the project's ball rule)
Row:     row[b] = fsum(w over the bin) vol[b]; zeros for a keypoint with at most min_neighborhood_size neighbours at non-zero
         distance; normalize: divided by its L2 norm (a zero row stays zero).
"""
import ctypes as C
import math

import numpy as np

MAX_BINS = 4096


def check_shape(radius, min_radius, L, K, J):
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError("radius > 0")
    if not 0 < min_radius < radius:
        raise ValueError("0 < min_radius < radius")
    if L < 2 or L % 2:
        raise ValueError("azimuth_bins even and >= 2")
    if K < 1 or J < 1:
        raise ValueError("elevation_bins >= 1 and radius_bins >= 1")
    if L * K * J > MAX_BINS:
        raise ValueError("at most 4096 bins")


def tables(radius, min_radius, L, K, J):
    """(e2, ca, sa, q, vol) as the library computes them (sf_usc_tables: host only, no GPU)."""
    from shot_fpfh_amd import _ffi

    check_shape(radius, min_radius, L, K, J)
    e2, ca, sa, q, vol = np.zeros(J + 1), np.zeros(L // 2), np.zeros(L // 2), np.zeros(K + 1), np.zeros(L * K * J)
    rc = _ffi.load().sf_usc_tables(float(radius), float(min_radius), L, K, J, *(a.ctypes.data_as(C.c_void_p) for a in (e2, ca, sa, q, vol)))
    assert rc == 0, _ffi.last_error()
    return e2, ca, sa, q, vol


def tables_numpy(radius, min_radius, L, K, J):
    """The same five tables from NumPy's own exp / log / cos / sin / cbrt (equal to the library's within a few ulp)."""
    check_shape(radius, min_radius, L, K, J)
    e = np.exp(np.log(min_radius) + (np.arange(J + 1) / J) * np.log(radius / min_radius))
    e[0], e[J] = min_radius, radius
    a = 2.0 * np.pi * np.arange(L // 2) / L
    ct = np.cos(np.pi * np.arange(K + 1) / K)
    ct[0], ct[K] = 1.0, -1.0
    if K % 2 == 0:
        ct[K // 2] = 0.0
    return e * e, np.cos(a), np.sin(a), ct * np.abs(ct), vol_numpy(e, ct, L)


def vol_numpy(e, ct, L):
    """vol's formula on given edges e[J + 1] and ct[K + 1].  The shell volume e[j + 1]^3 - e[j]^3 cancels: it carries an ulp of e
    3 / (1 - (e[j] / e[j + 1])^3) times over (8.6 at R / r0 = 10, J = 16), a third of which reaches vol."""
    K, J = ct.size - 1, e.size - 1
    shell = e[1:] * e[1:] * e[1:] - e[:-1] * e[:-1] * e[:-1]
    cell = (2.0 * np.pi / L) * (ct[:-1] - ct[1:])[:, None] * shell[None, :] / 3.0
    return np.broadcast_to(1.0 / np.cbrt(cell), (L, K, J)).reshape(-1).copy()


def density_weights(points, density_radius):
    """w[i] = 1.0 / (size of point i's ball of density_radius, i included)."""
    from sklearn.neighbors import KDTree

    return 1.0 / KDTree(points).query_radius(points, density_radius, count_only=True).astype(np.float64)


def local_coordinates(d, frame):
    """(r2, lx, ly, lz) of the offsets d (t x 3) in `frame` (3 x 3, columns x y z): elementwise, never `@`."""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    r2 = (dx * dx + dy * dy) + dz * dz
    lx = (dx * frame[0, 0] + dy * frame[1, 0]) + dz * frame[2, 0]
    ly = (dx * frame[0, 1] + dy * frame[1, 1]) + dz * frame[2, 1]
    lz = (dx * frame[0, 2] + dy * frame[1, 2]) + dz * frame[2, 2]
    return r2, lx, ly, lz


def bins(r2, lx, ly, lz, tab, L, K, J):
    """(j, l, k) of neighbours given by their local coordinates, by the comparison rules."""
    e2, ca, sa, q, _ = tab
    j = (r2[:, None] >= e2[None, 1:J]).sum(axis=1)
    h = (ly < 0) | ((ly == 0) & (lx < 0))
    u, v = np.where(h, -lx, lx), np.where(h, -ly, ly)
    l = (ca[None, 1:] * v[:, None] - sa[None, 1:] * u[:, None] >= 0).sum(axis=1) + h * (L // 2)
    k = ((lz * np.abs(lz))[:, None] <= q[None, 1:K] * r2[:, None]).sum(axis=1)
    return j, l, k


def rows(points, keypoints, lists, frames, weight, radius, min_radius=None, L=14, K=14, J=10, normalize=False,
         min_neighborhood_size=0, tab=None):
    """The m x D rows of `keypoints` (m x 3) with neighbourhoods `lists` (index arrays into points), `frames` (m x 3 x 3) and
    per-point `weight`."""
    min_radius = radius / 10 if min_radius is None else min_radius
    tab = tables(radius, min_radius, L, K, J) if tab is None else tab
    vol = tab[4]
    D = L * K * J
    out = np.zeros((len(lists), D))
    for i, nb in enumerate(lists):
        nb = np.asarray(nb, dtype=np.int64)
        r2, lx, ly, lz = local_coordinates(points[nb] - keypoints[i], frames[i])
        keep = r2 != 0
        if not keep.sum() > min_neighborhood_size:
            continue
        j, l, k = bins(r2[keep], lx[keep], ly[keep], lz[keep], tab, L, K, J)
        b = (l * K + k) * J + j
        w = weight[nb[keep]]
        order = np.argsort(b, kind="stable")
        b, w = b[order], w[order]
        starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
        for s, e in zip(starts, np.r_[starts[1:], b.size]):
            out[i, b[s]] = math.fsum(w[s:e]) * vol[b[s]]
        if normalize:
            norm = np.linalg.norm(out[i])
            if norm > 0:
                out[i] /= norm
    return out
