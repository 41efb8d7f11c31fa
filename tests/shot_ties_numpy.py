"""The SHOT contract for neighbours at equal distance, executable on the host.

`shot_row` states compute_single_shot_descriptor (shot.py:211-306) statement by statement in NumPy -- the same operations in the
same order on the same library, in the wording of this project's own NumPy form (oracle/numpy_shaped.py) -- with the one line that
leaves ties open, `order = np.argsort(rho)` (shot.py:218), as an argument: `order_fn(rho, index)` receives the distances of the
neighbours at non-zero distance and their indices in the caller's cloud array and returns the permutation in which the ten
`D[idx] += val` statements see them.

The contract the kernels are held to is `contract_order`: ascending rho, and among bit-equal rho ascending index -- ONE order for
all ten statements, so the last writer of a bin is the farthest neighbour and, among equally far ones, the one with the largest
index.  `reversed_ties` turns the ties round (the sensitivity probe); `recorded` replays a permutation written down elsewhere.

No engine import: NumPy alone."""
import numpy as np

PI = np.pi


def contract_order(rho, index):
    return np.lexsort((index, rho))


def reversed_ties(rho, index):
    return np.lexsort((-np.asarray(index), rho))


def recorded(perm):
    return lambda rho, index: np.asarray(perm)


def _octant(x, y):
    """get_azimuth_idx, shot.py:51-70 (three boolean maps combined into 0..7)."""
    a = (y > 0) | ((y == 0) & (x < 0))
    return 4 * a + 2 * np.logical_xor((x > 0) | ((x == 0) & (y > 0)), a) + np.where(
        (x * y > 0) | (x == 0), np.abs(x) < np.abs(y), np.abs(x) > np.abs(y))


def _shells(d, r):
    """interpolate_on_adjacent_husks, shot.py:73-118: (towards the outer shell, towards the inner shell, own shell)."""
    h = r / 2
    cur = (d < h) * (1 - np.abs(d - r / 4) / h) + (d > h) * (1 - np.abs(d - r * 3 / 4) / h)
    return ((d < h) & (d > r / 4)) * (d - r / 4) / h, ((d > h) & (d < r * 3 / 4)) * (r * 3 / 4 - d) / h, cur


def _elevations(phi, z):
    """interpolate_vertical_volumes, shot.py:121-171: (towards the upper half, towards the lower half, own half)."""
    q, near = PI / 2, np.abs(phi - PI / 2) < 1e-10
    up = (((phi > q) | (near & (z <= 0))) & (phi <= PI * 3 / 4)) * (PI * 3 / 4 - phi) / q
    lo = (((phi < q) & (~near | (z > 0))) & (phi >= PI / 4)) * (phi - PI / 4) / q
    cur = (phi < q) * (1 - np.abs(phi - PI / 4) / q) + (phi >= q) * (1 - np.abs(phi - PI * 3 / 4) / q)
    return up, lo, cur


def shot_row(p, pts, nrm, radius, frame, normalize, min_nb, order_fn=contract_order, index=None, details=None, n=11):
    """One row of 32 n bins (n = 11: the 352 bins of compute_single_shot_descriptor; any n: the serial variant's statements,
    shot.py:386-497, which are the same with n in place of 11).  pts, nrm: the neighbours and their normals; index: their indices
    in the caller's cloud array (default: their position in `pts`); details: a dict that receives, in evaluation order, what decides a neighbour's bins."""
    D = np.zeros((n, 8, 2, 2))
    index = np.arange(pts.shape[0]) if index is None else np.asarray(index)
    rho = np.linalg.norm(pts - p, axis=1)
    if (rho > 0).sum() > min_nb:
        keep = rho > 0
        loc = (pts[keep] - p) @ frame
        cosv = np.clip(nrm[keep] @ frame[:, 2].T, -1, 1)
        rho, index = rho[keep], index[keep]
        order = order_fn(rho, index)
        rho, loc, cosv = rho[order], loc[order], cosv[order]
        theta = np.arctan2(loc[:, 1], loc[:, 0])
        phi = np.arccos(np.clip(loc[:, 2] / rho, -1, 1))
        cpos = (cosv + 1.0) * n / 2.0 - 0.5
        ci = np.rint(cpos).astype(int)
        ti = _octant(loc[:, 0], loc[:, 1])
        pi_ = (loc[:, 2] > 0).astype(int)
        ri = (rho > radius / 2).astype(int)
        if details is not None:
            details.update(rho=rho, local=loc, cos_bin_pos=cpos, index=index[order])
        dc = cpos - ci
        sc = np.sign(dc)
        adc = sc * dc
        D[(ci + sc).astype(int) % n, ti, pi_, ri] += adc * ((ci > -0.5) & (ci < n - 0.5))  # S1
        D[ci, ti, pi_, ri] += 1 - adc  # S2
        outer, inner, cur = _shells(rho, radius)
        D[ci, ti, pi_, 1] += outer * (ri == 0)  # S3
        D[ci, ti, pi_, 0] += inner * (ri == 1)  # S4
        D[ci, ti, pi_, ri] += cur  # S5
        up, lo, curv = _elevations(phi, loc[:, 2])
        D[ci, ti, 1, ri] += up * (pi_ == 0)  # S6
        D[ci, ti, 0, ri] += lo * (pi_ == 1)  # S7
        D[ci, ti, pi_, ri] += curv  # S8
        size = 2 * PI / 8
        dt = np.clip((theta - (-PI + ti * size)) / size - 0.5, -0.5, 0.5)
        st = np.sign(dt)
        adt = st * dt
        D[ci, (ti + st).astype(int) % 8, pi_, ri] += adt  # S9
        D[ci, ti, pi_, ri] += 1 - adt  # S10
        if (nr := np.linalg.norm(D)) > 0:
            return D.ravel() / nr if normalize else D.ravel()
    return np.zeros(32 * n)


def edge_margin(details, radius):
    """How far the bin-deciding quantities of one call stay from their edges, the smallest over its neighbours: lx, ly, lz,
    |lx| - |ly| and rho - r/2 relative to the radius; cos_bin_pos against the half-integers (its scale is 1)."""
    lc, rho, cpos = details["local"], details["rho"], details["cos_bin_pos"]
    geo = np.minimum.reduce([np.abs(lc[:, 0]), np.abs(lc[:, 1]), np.abs(lc[:, 2]), np.abs(np.abs(lc[:, 0]) - np.abs(lc[:, 1])),
                             np.abs(rho - radius / 2)]) / radius
    half = np.abs(cpos - np.floor(cpos) - 0.5)
    return float(min(geo.min(), half.min()))
