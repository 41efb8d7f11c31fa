"""The clouds, radii and keypoints of the SHOT tie tests (test_shot_ties_host.py, test_hip_shot_ties.py) and of
tools/gen_golden_shot_ties.py: lattice clouds, where every list holds neighbours at bit-equal distance.

All coordinates are small integers times a power-of-two pitch, exact in float64; squared distances in units of the pitch are
integers, so a radius r with (r / pitch)^2 and (r / 2 / pitch)^2 away from the integers puts no point on the ball or on the
shell boundary r / 2, and the list lengths below are exact counts (asserted).  No engine import."""
import functools

import numpy as np

PITCH = 1.0 / 16
THIN_SIDE, THIN_KEEP, THIN_SEED = 20, 0.6, 20251
FULL_SIDE, FULL_X, FULL_KEYPOINT = 12, 3.3, (5, 6, 5)
DUP_N, DUP_SEED, DUP_PITCH, DUP_RADIUS = 300, 20252, 1.0 / 4096, 0.3
MAX_KEYPOINTS = 200
NORMAL_KINDS = ("constant", "random", "estimated")
CONSTANT_NORMAL = np.array([0.35, -0.48, 0.8]) / np.linalg.norm([0.35, -0.48, 0.8])

# class -> (radius in pitches, the interval the longest list of the whole cloud lies in, the K5 launches a self search takes)
CLASSES = {
    "c64": (2.3, 1, 64, ("k5_shot",)),
    "mid": (2.9, 65, 128, ("k5_shot", "k5_shot_mid")),  # <= 2 % of the lists need a second chunk: a launch of their own
    "c128": (3.3, 65, 128, ("k5_shot",)),
    "c192": (3.95, 129, 192, ("k5_shot",)),
    "c255": (4.45, 193, 255, ("k5_shot",)),
    "team4": (5.8, 256, 768, ("k5_shot", "k5_shot_tail")),
    "team8": (7.8, 769, 1536, ("k5_shot", "k5_shot_tail")),
    "team16": (9.9, 1537, 3072, ("k5_shot", "k5_shot_tail")),
    "stream": (12.3, 3073, 1 << 30, ("k5_shot", "k5_shot_tail", "k5_shot_tail_stream")),
}
IMPORT_CLASSES = {"import150": 3.95, "import450": 5.8}  # lists handed in: k_shot_long<., false> as the main launch
GOLDEN_CLASSES = ("c64", "c128", "c255")


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def thinned_lattice():
    """(ijk int16 (n, 3), points float64): a 20^3 lattice of pitch 1/16, every point kept with probability 0.6."""
    rng = np.random.default_rng(THIN_SEED)
    g = np.stack(np.meshgrid(*[np.arange(THIN_SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ijk = g[rng.random(g.shape[0]) < THIN_KEEP].astype(np.int16)
    return ijk, ijk.astype(np.float64) * PITCH


@functools.lru_cache(maxsize=None)
def _thin_d2():
    ijk = thinned_lattice()[0].astype(np.int32)
    return ((ijk[:, None, :] - ijk[None, :, :]) ** 2).sum(-1)


def check_radius(x):
    """x = r / pitch: no squared lattice distance on the ball's or the shell's boundary."""
    for v in (x * x, x * x / 4):
        assert abs(v - round(v)) > 1e-3, (x, v)
    return x * PITCH


@functools.lru_cache(maxsize=None)
def thin_counts(x):
    """List lengths (the point itself included) of every point of the thinned lattice at radius x pitches: exact."""
    check_radius(x)
    return (_thin_d2() <= x * x).sum(1)


def thin_lists(x, rows):
    """CSR lists (ascending caller index) of the given rows at radius x pitches."""
    inside = _thin_d2()[rows] <= x * x
    off = np.concatenate([[0], np.cumsum(inside.sum(1))])
    return off.astype(np.int64), np.nonzero(inside)[1].astype(np.int32)


def thin_keypoints(x):
    """At most 200 rows of the thinned lattice for radius x pitches: the interior ones (the whole ball inside the lattice) where
    there are any, else those nearest the centre -- the longest lists."""
    ijk = thinned_lattice()[0].astype(np.int32)
    lo = int(np.ceil(x))
    inter = np.flatnonzero(np.all((ijk >= lo) & (ijk <= THIN_SIDE - 1 - lo), axis=1))
    if inter.size == 0:
        c2 = ((2 * ijk - (THIN_SIDE - 1)) ** 2).sum(1)
        inter = np.sort(np.argsort(c2, kind="stable")[:MAX_KEYPOINTS])
    if inter.size > MAX_KEYPOINTS:
        inter = np.sort(np.random.default_rng(int(x * 100)).choice(inter, MAX_KEYPOINTS, replace=False))
    return inter


def thin_normals(kind, estimate=None):
    """constant: every neighbour in one cosine bin; random; estimated: estimate(points) -> (n, 3), the cloud's own normals."""
    _, p = thinned_lattice()
    if kind == "constant":
        return np.tile(CONSTANT_NORMAL, (p.shape[0], 1))
    if kind == "random":
        return _unit(np.random.default_rng(THIN_SEED + 1).standard_normal(p.shape))
    nr = np.asarray(estimate(p), dtype=np.float64)
    assert np.isfinite(nr).all() and np.abs(np.linalg.norm(nr, axis=1) - 1).max() < 1e-9
    return nr


def rotations(m, seed):
    """m seeded random rotations (orthonormal to rounding, determinant +1), (m, 3, 3)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return np.ascontiguousarray(q)


@functools.lru_cache(maxsize=None)
def full_lattice():
    """12^3 points, pitch 1/16; with the identity frame every neighbour of a keypoint sits on a bin boundary and ties up to
    48-fold.  (ijk, points, normals, keypoint row, radius)"""
    g = np.stack(np.meshgrid(*[np.arange(FULL_SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    nr = _unit(np.random.default_rng(THIN_SEED + 2).standard_normal(g.shape))
    row = int(np.flatnonzero((g == np.array(FULL_KEYPOINT)).all(1))[0])
    return g, g.astype(np.float64) * PITCH, nr, row, check_radius(FULL_X)


@functools.lru_cache(maxsize=None)
def duplicated_points():
    """300 random points on a 4096^3 lattice, each present three times (rows i, i + 300, i + 600) with three independent
    normals: equal geometry, unequal cosines.  (ijk, points, normals, radius)"""
    rng = np.random.default_rng(DUP_SEED)
    one = rng.integers(0, 4096, (DUP_N, 3)).astype(np.int16)
    ijk = np.tile(one, (3, 1))
    x = DUP_RADIUS / DUP_PITCH
    for v in (x * x, x * x / 4):
        assert abs(v - round(v)) > 1e-3
    return ijk, ijk.astype(np.float64) * DUP_PITCH, _unit(rng.standard_normal((3 * DUP_N, 3))), DUP_RADIUS


def brute_lists(ijk, rows, x):
    """CSR lists (ascending index) on any integer cloud at radius x pitches."""
    a = ijk.astype(np.int64)
    inside = ((a[rows][:, None, :] - a[None, :, :]) ** 2).sum(-1) <= x * x
    off = np.concatenate([[0], np.cumsum(inside.sum(1))])
    return off.astype(np.int64), np.nonzero(inside)[1].astype(np.int32)
