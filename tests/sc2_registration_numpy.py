"""SC2 registration -- one Kabsch fit per second-order seed, ranked by inliers over all matches -- stated in plain NumPy.  What
shot_fpfh_amd.matching.sc2_registration and K15 (csrc/consistency.hip) are held to -- not a test file.

With a, b, compat, C, N, SC2 and s2 exactly as in sc2_numpy:
    seeds     the n_seeds matches of the largest s2, s2 descending and position ascending, those with s2 > 0 only
    row_s[j]  = C[seed_s, j] sum_k C[seed_s, k] C[j, k]                      (integers; sum_j row_s[j] = s2[seed_s])
    top       = max_j row_s[j]
    member j  iff j == seed_s or (row_s[j] >= 1 and float64(row_s[j]) >= float64(group_share) * float64(top))
    size_s    = the member count; fewer than 3: status 1
    fit       Kabsch over the members, centroids first (sums by math.fsum), then the centred cross-covariance:
              R = argmax tr(R H), t = bbar - R abar; gap <= 1e-6 s1 or a result that is not finite: status 2; else status 0
    scoring   the status-0 transforms in seed order, |a R^T + t - b| <= distance_threshold (ransac_numpy.residual_norms) over ALL
              matches; the FIRST maximum wins
    refit     ransac_numpy.refit, refit_iterations times
"""
import numpy as np

import ransac_numpy as N
import sc2_numpy as S

MAX_SEEDS = 1024   # SF_SC2_MAX_SEEDS
SEED_TILE = 64     # SF_SC2_SEED_TILE: seeds of a workgroup of the device's seed-row GEMM
STATUS_OK, STATUS_NO_TRIPLE, STATUS_TOO_FEW, STATUS_NO_FIT = "done", "no consistent triple", "fewer than three matches", "no seed gave a fit"


def seeds_of(s2, n_seeds):
    """int64 (n_seeds,): the positions of the n_seeds largest s2 > 0, s2 descending and position ascending, then -1."""
    s2 = np.asarray(s2).astype(np.int64)
    order = np.lexsort((np.arange(s2.shape[0]), -s2))  # (primary key last)
    order = order[s2[order] > 0][:n_seeds]
    out = np.full(n_seeds, -1, dtype=np.int64)
    out[:order.shape[0]] = order
    return out


def seed_rows(cmat, seeds):
    """int64 (len(seeds), m) of ANY 0/1 matrix: row_s[j] = C[seed_s, j] sum_k C[seed_s, k] C[j, k]; a seed of -1: zeros."""
    cmat = np.asarray(cmat)
    m = cmat.shape[0]
    assert cmat.shape == (m, m) and m < 2 ** 24 and np.isin(cmat, (0, 1)).all()
    seeds = np.asarray(seeds, dtype=np.int64)
    cf = cmat.astype(np.float32)
    picked = np.maximum(seeds, 0)
    n = (cf[picked] @ cf.T).astype(np.int64)  # (partial sums are integers of at most m: exact in float32)
    return n * cmat[picked].astype(np.int64) * (seeds >= 0)[:, None]


def members_of(row, seed, group_share):
    """bool (m,): the consensus set of one seed from its row -- the filter's rule."""
    row = np.asarray(row)
    top = int(row.max(initial=0))
    keep = (row >= 1) & (row.astype(np.float64) >= np.float64(group_share) * np.float64(top))
    keep[seed] = True
    return keep


def fit_members(a, b, mask):
    """(status, Rt row (zeros unless status 0), the dict of ransac_numpy.refit_sums, s1 / gap)."""
    sums = N.refit_sums(a, b, mask)
    zero = np.zeros(12)
    if sums["count"] < 3:
        return 1, zero, sums, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        h = sums["h"]
        if not np.isfinite(h).all():
            return 2, zero, sums, np.inf
        sv = np.linalg.svd(h, compute_uv=False)
        gap = sv[1] + np.sign(np.linalg.det(h)) * sv[2]
        if not gap > N.GAP_TOL * sv[0]:
            return 2, zero, sums, np.inf
        rt = N.fit_from_sums(h, sums["abar"], sums["bbar"])
    if not np.isfinite(rt).all():
        return 2, zero, sums, np.inf
    return 0, rt, sums, float(sv[0] / gap)


def hypotheses(a, b, distance_threshold, min_edge=None, n_seeds=256, group_share=0.5):
    """dict: second_degree (uint32), seeds (int64, -1 after the found ones), n_found, rows (int64 (n_seeds, m)), member (uint8
    (n_seeds, m)), size (int32), status (uint8: 0, 1, 2, and 3 for a slot without a seed), rt ((n_seeds, 12)), sums (list of dicts),
    cond (s1 / gap per seed)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m = a.shape[0]
    assert m <= S.MAX_MATCHES and 1 <= n_seeds <= MAX_SEEDS
    cmat = S.compat_matrix(a, b, distance_threshold, min_edge)
    s2 = S.second_order(cmat)[0] if m else np.zeros(0, dtype=np.uint32)
    seeds = seeds_of(s2, n_seeds)
    rows = seed_rows(cmat, seeds) if m else np.zeros((n_seeds, 0), dtype=np.int64)
    member = np.zeros((n_seeds, m), dtype=np.uint8)
    size, status = np.zeros(n_seeds, dtype=np.int32), np.full(n_seeds, 3, dtype=np.uint8)
    rt, sums, cond = np.zeros((n_seeds, 12)), [None] * n_seeds, np.full(n_seeds, np.inf)
    for s, seed in enumerate(seeds):
        if seed < 0:
            continue
        assert int(rows[s].sum()) == int(s2[seed])
        mask = members_of(rows[s], seed, group_share)
        member[s], size[s] = mask, int(mask.sum())
        status[s], rt[s], sums[s], cond[s] = fit_members(a, b, mask)
    return dict(second_degree=s2, seeds=seeds, n_found=int((seeds >= 0).sum()), rows=rows, member=member, size=size, status=status,
                rt=rt, sums=sums, cond=cond)


def sc2_registration(scan_idx, ref_idx, scan_kp, ref_kp, distance_threshold, min_edge=None, n_seeds=256, group_share=0.5,
                     refit_iterations=2):
    """(inlier ratio, R, t, record dict) -- R NOT re-normalised.  record: status, the dict of `hypotheses` (its per-seed status
    as seed_status), slot_seed (the seed positions scored, ascending), counts per slot, winner_rank, winner_seed, winner_size,
    winner_inliers, refit_inliers.  Nothing scored: (0.0, None, None, record) with the status saying why."""
    a, b = N.matched_points(scan_idx, ref_idx, scan_kp, ref_kp)
    m = a.shape[0]
    none = dict(slot_seed=np.zeros(0, dtype=np.int64), counts=np.zeros(0, dtype=np.int64), winner_rank=-1, winner_seed=-1,
                winner_size=0, winner_inliers=0, refit_inliers=[])
    if m < 3:
        return 0.0, None, None, dict(none, status=STATUS_TOO_FEW)
    hyp = hypotheses(a, b, distance_threshold, min_edge, n_seeds, group_share)
    hyp["seed_status"] = hyp.pop("status")
    slot_seed = np.flatnonzero(hyp["seed_status"] == 0).astype(np.int64)
    if slot_seed.size == 0:
        return 0.0, None, None, dict(none, **hyp, status=STATUS_NO_TRIPLE if hyp["n_found"] == 0 else STATUS_NO_FIT)
    counts = N.score(a, b, hyp["rt"][slot_seed], distance_threshold)
    w = N.first_max(counts)
    rank = int(slot_seed[w])
    best, count, kept = N.refit(a, b, hyp["rt"][rank], int(counts[w]), distance_threshold, refit_iterations)
    record = dict(hyp, status=STATUS_OK, slot_seed=slot_seed, counts=counts, winner_rank=rank, winner_seed=int(hyp["seeds"][rank]),
                  winner_size=int(hyp["size"][rank]), winner_inliers=int(counts[w]), refit_inliers=kept)
    return count / m, best[:9].reshape(3, 3), best[9:], record
