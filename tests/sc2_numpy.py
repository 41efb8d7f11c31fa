"""Second-order consistency (SC2; Chen, Sun, Yang, Tao, CVPR 2022) of a set of matches, stated in plain NumPy.  What
shot_fpfh_amd.matching.second_order_consistency_filter and K14 (csrc/consistency.hip) are held to, exactly -- not a test file.

With a, b and compat(i, j) exactly as in consistency_numpy (min_edge included; a NaN row is compatible with nothing):
    C[i,j]   = 1 if compat(i,j) else 0                        (symmetric, zero diagonal)
    N[i,j]   = sum_k C[i,k] C[j,k]
    SC2[i,j] = C[i,j] N[i,j]
    s2[i]    = sum_j SC2[i,j]                                 (uint32: at most (m-1)(m-2) < 2^30 for m <= MAX_MATCHES)
    seed     = the LOWEST index among the maxima of s2;  max s2 = 0: status "no consistent triple", nothing kept
    member   = C[seed,.] with member[seed] = 1;  g = sum member
    row[j]   = SC2[seed,j]                                    (zero at the seed and outside the group)
    top      = max_j row[j]
    keep[j]  = j == seed  or  (row[j] >= 1 and float64(row[j]) >= float64(group_share) * float64(top))
s2[i] counts the pairs (j, k) compatible with i and with each other: twice the triangles through i in the compatibility graph.
group_degree is K13's: the degree over the member columns, for every row; for a member j other than the seed it is row[j] + 1
(the seed is one of the member columns and compatible with j), which is how the public call gets `row` from the device's output.
"""
import numpy as np

import consistency_numpy as C1

STATUS_OK, STATUS_NO_TRIPLE, STATUS_TOO_FEW = "done", "no consistent triple", "fewer than three matches"
MAX_MATCHES = 32768  # SF_SC2_MAX_MATCHES
TILE = 256           # SF_SC2_TILE: the device's matrix is padded to a multiple of it


def compat_matrix(a, b, distance_threshold, min_edge=None, chunk=512):
    """C as uint8 (m, m)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = a.shape[0]
    out = np.zeros((m, m), dtype=np.uint8)
    for r0 in range(0, m, chunk):
        rows = np.arange(r0, min(r0 + chunk, m))
        out[rows] = C1.compat_rows(a, b, rows, distance_threshold, min_edge)
    return out


def second_order(cmat):
    """(s2 as uint32, SC2 as int64 (m, m)) of ANY 0/1 matrix: s2[i] = sum_j C[i,j] sum_k C[i,k] C[j,k].  N is a float32 BLAS
    product of 0/1 matrices: every partial sum is an integer of at most m, exact below 2^24."""
    cmat = np.asarray(cmat)
    m = cmat.shape[0]
    assert cmat.shape == (m, m) and m < 2 ** 24 and np.isin(cmat, (0, 1)).all()
    cf = cmat.astype(np.float32)
    n = cf @ cf.T
    assert n.dtype == np.float32 and (n.max(initial=0) <= m)
    sc2 = n.astype(np.int64) * cmat.astype(np.int64)
    s2 = sc2.sum(axis=1)
    assert s2.max(initial=0) < 2 ** 32
    return s2.astype(np.uint32), sc2


def group(a, b, distance_threshold, min_edge=None, group_share=0.5):
    """dict: status, seed, seed_score, second_degree (uint32), member (uint8), g, group_degree (uint32), seed_row (uint32),
    keep (ascending positions)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = a.shape[0]
    none = dict(seed=-1, seed_score=0, second_degree=np.zeros(m, dtype=np.uint32), member=np.zeros(m, dtype=np.uint8), g=0,
                group_degree=np.zeros(m, dtype=np.uint32), seed_row=np.zeros(m, dtype=np.uint32), keep=np.zeros(0, dtype=np.int64))
    if m < 3:
        return dict(none, status=STATUS_TOO_FEW)
    assert m <= MAX_MATCHES
    cmat = compat_matrix(a, b, distance_threshold, min_edge)
    s2, sc2 = second_order(cmat)
    seed = C1.first_max(s2)
    if s2[seed] == 0:
        return dict(none, status=STATUS_NO_TRIPLE)
    member = cmat[seed].copy()
    member[seed] = 1
    g = int(member.sum())
    gdeg = cmat[:, member.astype(bool)].sum(axis=1, dtype=np.int64).astype(np.uint32)
    row = sc2[seed]
    top = int(row.max())
    keep = (row >= 1) & (row.astype(np.float64) >= np.float64(group_share) * np.float64(top))
    keep[seed] = True
    return dict(status=STATUS_OK, seed=seed, seed_score=int(s2[seed]), second_degree=s2, member=member, g=g, group_degree=gdeg,
                seed_row=row.astype(np.uint32), keep=np.flatnonzero(keep).astype(np.int64))


def second_order_consistency_filter(scan_idx, ref_idx, scan_kp, ref_kp, distance_threshold, min_edge=None, group_share=0.5):
    """(scan indices kept, reference indices kept, the dict of `group`), the kept ones in input order."""
    from ransac_numpy import matched_points

    scan_idx, ref_idx = np.asarray(scan_idx), np.asarray(ref_idx)
    a, b = matched_points(scan_idx, ref_idx, scan_kp, ref_kp)
    out = group(a, b, distance_threshold, min_edge, group_share)
    return scan_idx[out["keep"]], ref_idx[out["keep"]], out
