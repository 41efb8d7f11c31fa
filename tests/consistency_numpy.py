"""The geometric-consistency filter of a set of matches, stated in plain NumPy (float64).  What
shot_fpfh_amd.matching.geometric_consistency_filter and K13 (csrc/consistency.hip) are held to, exactly -- not a test file.

With a = scan_keypoints[scan_idx], b = ref_keypoints[ref_idx], both (m, 3), every operation unfused float64 in this order:
    dp(i,j) = sqrt(((ax_i - ax_j)^2 + (ay_i - ay_j)^2) + (az_i - az_j)^2),   dq(i,j) the same on b
    compat(i,j) = i != j  and  |dp - dq| <= distance_threshold  and  min(dp, dq) >= min_edge
    degree[i] = #{ j : member[j] and compat(i,j) }
A comparison that involves a NaN is false.  The group: deg over all columns; seed = the lowest index among the maxima of deg;
member = compat(seed, .) with member[seed] = 1; g = sum member; gdeg = degree over the member columns;
keep[i] = member[i] and gdeg[i] >= float64(group_share) (g - 1).  max(deg) = 0: no group, nothing is kept.
"""
import numpy as np

from ransac_numpy import matched_points

STATUS_OK, STATUS_NO_PAIR, STATUS_TOO_FEW = "done", "no consistent pair", "fewer than two matches"


def lengths(p, rows):
    """|p_i - p_j| for i in rows, every j: (len(rows), m)."""
    dx = p[rows, None, 0] - p[None, :, 0]
    dy = p[rows, None, 1] - p[None, :, 1]
    dz = p[rows, None, 2] - p[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def compat_rows(a, b, rows, distance_threshold, min_edge=None):
    """compat(i, .) for i in rows: bool (len(rows), m)."""
    min_edge = distance_threshold if min_edge is None else min_edge
    rows = np.asarray(rows, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        dp, dq = lengths(a, rows), lengths(b, rows)
        ok = (np.abs(dp - dq) <= np.float64(distance_threshold)) & (np.minimum(dp, dq) >= np.float64(min_edge))
    ok[np.arange(rows.shape[0]), rows] = False
    return ok


def degree(a, b, distance_threshold, min_edge=None, member=None, chunk=256):
    """degree[i] over the columns of `member` (None: all), uint32."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = a.shape[0]
    cols = np.ones(m, dtype=bool) if member is None else np.asarray(member).astype(bool)
    out = np.zeros(m, dtype=np.uint32)
    for r0 in range(0, m, chunk):
        rows = np.arange(r0, min(r0 + chunk, m))
        out[rows] = np.count_nonzero(compat_rows(a, b, rows, distance_threshold, min_edge) & cols[None, :], axis=1)
    return out


def first_max(values):
    best, arg = -1, -1
    for i, v in enumerate(values):
        if v > best:  # strict: the lowest index among the maxima
            best, arg = int(v), i
    return arg


def group(a, b, distance_threshold, min_edge=None, group_share=0.4):
    """dict: status, seed, seed_degree, degree (uint32), member (uint8), g, group_degree (uint32), keep (ascending positions)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = a.shape[0]
    none = dict(seed=-1, seed_degree=0, degree=np.zeros(m, dtype=np.uint32), member=np.zeros(m, dtype=np.uint8), g=0,
                group_degree=np.zeros(m, dtype=np.uint32), keep=np.zeros(0, dtype=np.int64))
    if m < 2:
        return dict(none, status=STATUS_TOO_FEW)
    deg = degree(a, b, distance_threshold, min_edge)
    seed = first_max(deg)
    if deg[seed] == 0:
        return dict(none, status=STATUS_NO_PAIR)
    member = compat_rows(a, b, [seed], distance_threshold, min_edge)[0]
    member[seed] = True
    g = int(np.count_nonzero(member))
    gdeg = degree(a, b, distance_threshold, min_edge, member=member)
    keep = member & (gdeg.astype(np.float64) >= np.float64(group_share) * np.float64(g - 1))
    return dict(status=STATUS_OK, seed=seed, seed_degree=int(deg[seed]), degree=deg, member=member.astype(np.uint8), g=g,
                group_degree=gdeg, keep=np.flatnonzero(keep).astype(np.int64))


def geometric_consistency_filter(scan_idx, ref_idx, scan_kp, ref_kp, distance_threshold, min_edge=None, group_share=0.4):
    """(scan indices kept, reference indices kept, the dict of `group`), the kept ones in input order."""
    scan_idx, ref_idx = np.asarray(scan_idx), np.asarray(ref_idx)
    a, b = matched_points(scan_idx, ref_idx, scan_kp, ref_kp)
    out = group(a, b, distance_threshold, min_edge, group_share)
    return scan_idx[out["keep"]], ref_idx[out["keep"]], out


def synthetic_truth(m, inlier_share, seed=0):
    """Positions of the true matches of ransac_numpy.synthetic_matches(m, inlier_share, seed=seed): its generator replayed up to
    the draw that decides them (the scan keypoints drawn on the way are returned too, for the caller to check the replay)."""
    rng = np.random.default_rng(seed)
    rng.normal(size=(3, 3))
    rng.uniform(-0.5, 0.5, 3)
    scan_kp = rng.random((m, 3))
    return np.flatnonzero(rng.random(m) < inlier_share).astype(np.int64), scan_kp


# ---- small constructed sets that both test files use ------------------------------------------------------------------------------
def lattice_set(m, seed=0):
    """(a, b, distance_threshold, min_edge): points on the 2^-3 lattice of ONE axis, so every length and every difference of two
    lengths is exact -- pairs sit exactly on the threshold (|dp - dq| = 1/8), exactly on min_edge (a length of 1/8) and on top
    of each other (shared keypoints, length 0)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 24, m)
    y = x + rng.integers(-1, 2, m)
    a, b = np.zeros((m, 3)), np.zeros((m, 3))
    a[:, 1], b[:, 1] = x / 8.0, y / 8.0 + 3.0
    return a, b, 0.125, 0.125


def tie_set(m, junk=5, seed=0):
    """(a, b, distance_threshold, min_edge): rows junk .. m-1 are distinct points of the 2^-3 lattice in 3-D and b = a + a
    lattice vector there, so they are all compatible with each other, exactly, and tie for the maximum; rows 0 .. junk-1 have
    b = 3 a + 100, whose lengths agree with nothing.  The seed is row `junk`."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(16 ** 3)[:m]
    a = np.stack([cells % 16, (cells // 16) % 16, cells // 256], axis=1) / 8.0
    b = a + np.array([0.5, -0.25, 1.0])
    b[:junk] = 3.0 * a[:junk] + 100.0
    return a, b, 2.0 ** -10, 2.0 ** -10
