"""The calls tests/test_hip_plumbing_pin.py holds to a recording (tests/golden/plumbing_pin.npz, written by
tools/gen_golden_plumbing_pin.py): every entry point whose host side stages operands, calls a rocPRIM primitive or maps between
the caller's order and the cell-sorted one.  Per call three things are kept: the SHA-256 of every output array, how often the
host waited for the stream (sf_sync_count) and which timer names gained how many launches (profiling off: the counts alone).

The clouds are integer arithmetic that is exact in float64 -- coordinates ((i i + 3 i + 1) K_c mod 2^20) / 2^20 with an odd K_c
per axis -- so they are formed again by whoever needs them and only the results are stored.  Sizes: 0 where the entry point
takes it, 2, 257 (one past a 256-thread block) and 5000; the radii keep every ball between 1 and 255 points, which `cloud_of`
checks with a float64 count whenever it makes a cloud."""
import hashlib
import os

import numpy as np

K_AXES = np.array([421337, 736481, 918273], dtype=np.int64)
SIZES = (0, 2, 257, 5000)
RADII = {0: (0.25, 0.125), 2: (1.0, 0.5), 257: (0.25, 0.1875), 5000: (0.09375, 0.0625)}  # per size: (larger, smaller), dyadic
SLOT_QUERIES, SLOT_RADIUS = 8 * 2048, 0.1015625  # the fewest queries that take the search's single sweep; lists of 9 .. 41
FAR_QUERY =(50.0, -50.0, 50.0)  # far outside the unit box: k-NN answers it only after its retries
_CLOUDS = {}


def points_of(n, first=0):
    i = np.arange(first, first + n, dtype=np.int64)
    return (((i * i + 3 * i + 1)[:, None] * K_AXES) % 2 ** 20) / 2.0 ** 20


def normals_of(n):
    """Unit vectors from another stretch of the same sequence (multiplications, two additions in a fixed order, one correctly
    rounded root and division each: the same bits wherever NumPy runs)."""
    v = points_of(n, first=7919) - 0.5
    return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]


def ball_sizes(p, r):
    """|{j : |p_j - p_i| <= r}| in float64, by the project's ball rule d2 = (dx dx + dy dy) + dz dz <= r r."""
    out = np.zeros(p.shape[0], dtype=np.int64)
    for a in range(0, p.shape[0], 500):
        d = p[a:a + 500, None, :] - p[None, :, :]
        out[a:a + 500] = np.count_nonzero((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= r * r, axis=1)
    return out


def cloud_of(n):
    """(points, normals) of size n; asserts, once per size, that both radii of the size keep every ball within 1 .. 255 points."""
    if n not in _CLOUDS:
        p = points_of(n)
        for r in RADII[n]:
            k = ball_sizes(p, r)
            assert n == 0 or (k.min() >= 1 and k.max() <= 255), (n, r, int(k.min()), int(k.max()))
        _CLOUDS[n] = (p, normals_of(n))
    return _CLOUDS[n]


class Recorder:
    """Runs calls on one engine and keeps, per call, {"sha256": [...], "syncs": int, "launches": {name: count}}."""

    def __init__(self, eng):
        self.eng, self.rows = eng, {}

    def _launches(self):
        return {name: v[0] for name, v in self.eng.profile_report().items()}

    def call(self, name, fn):
        """fn() -> an array, a DeviceArray, None or a tuple of those: measured across fn alone, device arrays fetched after."""
        from shot_fpfh_amd.engine import DeviceArray

        assert name not in self.rows, name
        before = self._launches()
        s0 = self.eng.lib.sf_sync_count()
        out = fn()
        syncs = int(self.eng.lib.sf_sync_count() - s0)
        after = self._launches()
        arrays = []
        for x in out if isinstance(out, tuple) else (out,):
            if isinstance(x, DeviceArray):
                x = x.to_host()
            if isinstance(x, np.ndarray):
                arrays.append(np.ascontiguousarray(x))
        sha = [hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest() for a in arrays]
        gained = {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}
        self.rows[name] = {"sha256": sha, "syncs": syncs, "launches": gained}
        return out


def group_upload(rec):
    eng = rec.eng
    for n in SIZES:
        p, nrm = cloud_of(n)
        plain = rec.call(f"upload_{n}", lambda: eng.cloud(p))
        rec.call(f"set_normals_{n}", lambda: plain.set_normals(nrm))
        both = rec.call(f"upload_normals_{n}", lambda: eng.cloud(p, nrm))
        if n:  # what the uploads left, read through the grid: cell-sorted position -> caller index
            plain.build_grid(RADII[n][0])
            both.build_grid(RADII[n][0])
            rec.call(f"perm_{n}", lambda: (plain.perm(), both.perm()))
        plain.free()
        both.free()


def group_iss(rec):
    for n in SIZES:
        big, small = RADII[n]
        c = rec.eng.cloud(cloud_of(n)[0])
        sal = rec.call(f"iss_saliency_{n}", lambda: c.iss_saliency(big, min_neighbors=2))
        rec.call(f"iss_saliency_counts_{n}", lambda: c.iss_saliency(big, min_neighbors=2, return_counts=True))
        rec.call(f"iss_select_{n}", lambda: c.iss_select(sal, small, min_neighbors=1))
        rec.call(f"iss_keypoints_{n}", lambda: c.iss_keypoints(big, small, min_neighbors=2))
        rec.call(f"iss_keypoints_saliency_{n}", lambda: c.iss_keypoints(big, small, min_neighbors=2, return_saliency=True))
        c.free()


def group_outliers(rec):
    for n in SIZES:
        big, small = RADII[n]
        c = rec.eng.cloud(cloud_of(n)[0])
        if n >= 2:
            k = min(4, n - 1)
            rec.call(f"knn_mean_distance_{n}", lambda: c.knn_mean_distance(k))
            rec.call(f"statistical_outliers_{n}", lambda: c.statistical_outliers(k, 0.5, return_stats=True))
        rec.call(f"ball_counts_{n}", lambda: c.ball_counts(small))
        rec.call(f"radius_outliers_{n}", lambda: c.radius_outliers(big, 3, return_counts=True))
        c.free()


def group_usc(rec):
    eng = rec.eng
    for n in SIZES:
        big, small = RADII[n]
        p, nrm = cloud_of(n)
        c = eng.cloud(p, nrm)
        w = rec.call(f"usc_weights_{n}", lambda: c.usc_weights(small))
        dw = eng.empty((max(n, 1),)).from_host(np.zeros(max(n, 1)))
        rec.call(f"usc_weights_device_{n}", lambda: c.usc_weights(small, out=dw))
        if n:
            nb = c.radius_search(p[: min(n, 64)], big)
            rec.call(f"usc_rows_{n}", lambda: nb.usc(w, big / 8, azimuth_bins=2, elevation_bins=1, radius_bins=1))
            nb.free()
        dw.free()
        c.free()


def group_search(rec):
    for n in SIZES[1:]:
        big = RADII[n][0]
        p = cloud_of(n)[0]
        c = rec.eng.cloud(p)
        q = p[::3] + 2.0 ** -12
        for which in ("planned", "recorded"):  # the second search of a radius sizes its slots from the first one's record
            nb = rec.call(f"radius_search_{which}_{n}", lambda: c.radius_search(q, big))
            rec.call(f"radius_search_{which}_export_{n}", lambda: nb.export(return_distance=True))
            nb.free()
        nb = rec.call(f"radius_search_none_{n}", lambda: c.radius_search(np.zeros((0, 3)), big))
        rec.call(f"radius_search_none_export_{n}", lambda: nb.export())
        nb.free()
        if n == 5000:
            # 8 x 2048 queries and more take the single sweep into slots; slots of 32 entries (the switch the suite forces the
            # slot size with) leave a minority of the lists to the select + scan + refill of the overflowed ones.  The first
            # search sizes its slots from a counted sample, the second from the first one's statistics.
            q = points_of(SLOT_QUERIES, first=10000)
            os.environ["SF_K2_CAP"] = "32"
            try:
                for which in ("sampled", "hinted"):
                    nb = rec.call(f"radius_search_slots_{which}", lambda: c.radius_search(q, SLOT_RADIUS))
                    assert 0 < np.count_nonzero(nb.counts() > 32) < SLOT_QUERIES // 2
                    rec.call(f"radius_search_slots_{which}_export", lambda: nb.export(return_distance=True))
                    nb.free()
            finally:
                del os.environ["SF_K2_CAP"]
        c.free()


def group_fpfh(rec):
    eng = rec.eng
    for n in SIZES[1:]:
        big = RADII[n][0]
        p, nrm = cloud_of(n)
        c = eng.cloud(p, nrm)
        nb = rec.call(f"radius_search_self_{n}", lambda: c.radius_search_self(big))
        sp = eng.spfh(c, 5, nb.max_count, big)
        rec.call(f"spfh_compute_{n}", lambda: sp.compute(nb) and None)
        rec.call(f"spfh_export_{n}", lambda: sp.export())
        rec.call(f"fpfh_all_{n}", lambda: sp.fpfh(nb))
        kp = (np.arange(0, n, 5, dtype=np.int64) * 7) % n
        rec.call(f"fpfh_keypoints_{n}", lambda: sp.fpfh(nb, keypoints_indices=kp))
        out = eng.empty((kp.shape[0] + 2, 125))
        rec.call(f"fpfh_keypoints_device_{n}", lambda: sp.fpfh(nb, keypoints_indices=kp, out=out, out_row=1).rows_to_host(1, kp.shape[0]))
        out.free()
        sp.free()
        nb.free()
        c.free()


def group_knn(rec):
    for n in SIZES[1:]:
        p = cloud_of(n)[0]
        c = rec.eng.cloud(p)
        q = np.vstack([p[:64] + 2.0 ** -12, [FAR_QUERY]])
        nb = rec.call(f"knn_3_{n}", lambda: c.knn_search(q, min(3, n)))
        rec.call(f"knn_3_export_{n}", lambda: nb.export(return_distance=True))
        nb.free()
        if n == 5000:  # beyond the LDS buffer of the one-wave kernel: count, fill, segmented sort
            nb = rec.call("knn_2000_5000", lambda: c.knn_search(q[:8], 2000))
            rec.call("knn_2000_export_5000", lambda: nb.export(return_distance=True))
            nb.free()
        c.free()


def group_normals(rec):
    for n in SIZES[1:]:
        big = RADII[n][0]
        p, nrm = cloud_of(n)
        c = rec.eng.cloud(p)
        q = p[::2]
        rec.call(f"normals_radius_{n}", lambda: c.normals_radius(q, big))
        rec.call(f"normals_radius_pre_{n}", lambda: c.normals_radius(q, big, pre_computed_normals=nrm[::2]))
        rec.call(f"normals_radius_none_{n}", lambda: c.normals_radius(np.zeros((0, 3)), big))
        out = rec.eng.empty((n, 3))
        rec.call(f"normals_radius_self_{n}", lambda: c.normals_radius_self(big, out))
        out.free()
        c.free()


def group_shot(rec):
    eng = rec.eng
    i = np.arange(-40, 41, dtype=np.float64)
    rec.call("azimuth_idx", lambda: eng.azimuth_idx(np.tile(i, 81) / 32.0, np.repeat(i, 81) / 32.0))
    rec.call("azimuth_idx_none", lambda: eng.azimuth_idx(np.zeros(0), np.zeros(0)))
    for n in SIZES[1:]:
        big = RADII[n][0]
        p, nrm = cloud_of(n)
        c = eng.cloud(p, nrm)
        nb = c.radius_search(p[: min(n, 300)], big)
        rec.call(f"shot_serial_{n}", lambda: nb.shot_serial(min_neighborhood_size=3))
        rec.call(f"shot_serial_bins_{n}", lambda: nb.shot_serial(min_neighborhood_size=3, n_cosine_bins=5))
        out = eng.empty((nb.m, 32 * 5))
        rec.call(f"shot_serial_bins_device_{n}", lambda: nb.shot_serial(min_neighborhood_size=3, n_cosine_bins=5, out=out))
        out.free()
        rec.call(f"shot_single_scale_{n}", lambda: nb.shot_single_scale(min_neighborhood_size=3))
        out, lrf = eng.empty((nb.m, 352)), eng.empty((nb.m, 9))
        rec.call(f"shot_single_scale_device_{n}", lambda: (nb.shot_single_scale(min_neighborhood_size=3, out=out, lrf_out=lrf), lrf))
        out.free()
        lrf.free()
        nb.free()
        c.free()


def group_voxels(rec):
    from shot_fpfh_amd.core import grid_subsampling, voxel_closest_to_barycentre  # (keypoint_selection's grid_subsampling path)

    for n in SIZES:
        p = cloud_of(n)[0]
        rec.call(f"grid_subsampling_{n}", lambda: grid_subsampling(p, RADII[n][0], engine=rec.eng))
        rec.call(f"voxel_closest_by_index_{n}", lambda: voxel_closest_to_barycentre(p, RADII[n][1], within_voxel_order="index", engine=rec.eng))


def group_match(rec):
    """sf_match_argmin and sf_ransac_score, with host operands and with resident ones."""
    eng = rec.eng
    for m in (2, 257):
        a = points_of(11 * m).reshape(m, 33)
        b = points_of(11 * (m + 3), first=4001).reshape(m + 3, 33)
        rec.call(f"match_argmin_{m}", lambda: eng.match_argmin(a, b, want_dist=True, want_col=True))
        rec.call(f"match_argmin_plain_{m}", lambda: eng.match_argmin(a, b, want_dist=False)[0])
        p = points_of(m)
        q = p + np.array([0.25, 0.0, -0.125])
        rt = np.tile(np.concatenate([np.eye(3).reshape(9), [0.25, 0.0, -0.125]]), (5, 1))
        rt[:, 9] += np.arange(5) / 256.0  # draw j is off by j 2^-8 along x: inside the threshold for j = 0, 1, 2
        rec.call(f"ransac_score_{m}", lambda: eng.ransac_score(p, q, rt, 0.01))
        dev = [eng.empty(x.shape).from_host(x) for x in (a, b, p, q, rt)]
        idx, dist, col, inl = eng.empty((m,), np.int64), eng.empty((m,)), eng.empty((m + 3,), np.int64), eng.empty((5,), np.int64)
        rec.call(f"match_argmin_device_{m}", lambda: (eng.match_argmin_device(dev[0], dev[1], idx, dist, col), idx, dist, col)[1:])
        rec.call(f"ransac_score_device_{m}", lambda: eng.ransac_score_device(dev[2], dev[3], m, dev[4], 5, 0.01, inl))
        for d in dev + [idx, dist, col, inl]:
            d.free()


GROUPS = dict(upload=group_upload, iss=group_iss, outliers=group_outliers, usc=group_usc, search=group_search, fpfh=group_fpfh,
              knn=group_knn, normals=group_normals, shot=group_shot, voxels=group_voxels, match=group_match)


def run_group(name):
    """The calls of one group on a fresh engine: {call: {"sha256", "syncs", "launches"}}."""
    from shot_fpfh_amd.engine import Engine

    eng = Engine()
    try:
        rec = Recorder(eng)
        GROUPS[name](rec)
        return rec.rows
    finally:
        eng.close()
