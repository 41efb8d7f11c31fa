"""The NumPy statement of spin images (K24): what tests/test_spin_host.py checks against closed forms and the unquantised
bilinear image, and tests/test_hip_spin.py holds the device to, bit for bit.  Modelled on pcl::SpinImageEstimation (Johnson,
Hebert 1999), decided here so that a row is a pure function of the cloud: bin contents are integers, so a row never depends on
the order of a list or of the cloud.

All arithmetic is IEEE float64, unfused, elementwise, in the order written.

Parameters: radius R > 0; image_width W, 1 <= W <= 44; signed_beta; min_cos (optional); normalize; min_neighborhood_size.
Scale:   inv_bin = (W sqrt(2.0)) / R  (sf_spin_scale -- `scale`; PCL's bin_size = R / W / sqrt 2).  The image covers the cylinder
         of radius and half-height R / sqrt 2, inscribed in the search ball.
Shape:   (W + 1) x NV nodes, NV = 2 W + 1 (signed) or W + 1 (unsigned); node (iu, iv) at iu NV + iv; D = (W + 1) NV <= 4096.
A keypoint p with axis n (used as given), per list entry at x with normal m:
      1. d = x - p;  d2 = (dx dx + dy dy) + dz dz;  beta = (nx dx + ny dy) + nz dz
      2. a2 = d2 - beta beta, 0 when negative;  alpha = sqrt(a2);  u = alpha inv_bin
      3. t = beta inv_bin (signed), |beta| inv_bin (unsigned)
      4. it contributes iff d2 > 0 and u <= W and |t| <= W, and with min_cos given: c = (nx mx + ny my) + nz mz,
         c >= min_cos (signed), |c| >= min_cos (unsigned).  Positive tests: a NaN contributes nothing.
      5. v = t + W (signed), t (unsigned)
      6. iu = floor(u), qu = floor((u - iu) 65536.0) in [0, 65535]; iv, qv from v alike.  Integer weights
         (65536 - qu)(65536 - qv) -> (iu, iv);  qu (65536 - qv) -> (iu + 1, iv);  (65536 - qu) qv -> (iu, iv + 1);
         qu qv -> (iu + 1, iv + 1);  a zero weight is not added (u = W gives qu = 0: no node outside the image is addressed).
         The four sum to exactly 2^32.
Row:     c = the number of contributing entries.  c <= min_neighborhood_size: zeros.  Else row[b] = float(count[b]) 2^-32, or with
         normalize float(count[b]) / (float(c) 2^32): one correctly rounded conversion, then an exact scaling or one division.
A list of 2^24 entries or more is refused.
"""
import ctypes as C

import numpy as np

MAX_WIDTH = 44
MAX_LIST = 1 << 24  # a list this long or longer is refused
ONE = 1 << 16       # the fixed-point unit of a bilinear fraction
TWO32 = 4294967296.0


def scale(R, W):
    """inv_bin as the library computes it (sf_spin_scale: host only, no GPU)."""
    from shot_fpfh_amd import _ffi

    out = C.c_double(0.0)
    rc = _ffi.load().sf_spin_scale(float(R), int(W), C.byref(out))
    if rc != 0:
        raise ValueError(_ffi.last_error())
    return out.value


def shape(W, signed_beta=True):
    """(NV, D) of an image of width W."""
    if not 1 <= W <= MAX_WIDTH:
        raise ValueError("1 <= image_width <= 44")
    NV = 2 * W + 1 if signed_beta else W + 1
    return NV, (W + 1) * NV


def entry_coords(p, n, x, m, inv_bin, W, signed_beta=True, min_cos=None):
    """Steps 1-5 for arrays of entries (x, m: k x 3) of one keypoint p with axis n: a dict of keep, u, v, t, d2, beta, alpha, c."""
    p, n = np.asarray(p, dtype=np.float64), np.asarray(n, dtype=np.float64)
    x, m = np.asarray(x, dtype=np.float64).reshape(-1, 3), np.asarray(m, dtype=np.float64).reshape(-1, 3)
    Wd = np.float64(W)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - p[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        beta = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2]
        a2 = d2 - beta * beta
        a2 = np.where(a2 < 0.0, 0.0, a2)
        alpha = np.sqrt(a2)
        u = alpha * inv_bin
        t = (beta if signed_beta else np.abs(beta)) * inv_bin
        keep = (d2 > 0.0) & (u <= Wd) & (np.abs(t) <= Wd)
        c = (n[0] * m[:, 0] + n[1] * m[:, 1]) + n[2] * m[:, 2]
        if min_cos is not None:
            keep &= (c if signed_beta else np.abs(c)) >= np.float64(min_cos)
        v = t + Wd if signed_beta else t
    return dict(keep=keep, u=u, v=v, t=t, d2=d2, beta=beta, alpha=alpha, c=c)


def entry_weights(u, v):
    """Step 6 for contributing entries: (iu, iv, w), w a k x 4 int64 array of the weights to (iu, iv), (iu + 1, iv), (iu, iv + 1),
    (iu + 1, iv + 1)."""
    fu_, fv_ = np.floor(u), np.floor(v)
    qu = np.floor((u - fu_) * 65536.0).astype(np.int64)
    qv = np.floor((v - fv_) * 65536.0).astype(np.int64)
    w = np.stack([(ONE - qu) * (ONE - qv), qu * (ONE - qv), (ONE - qu) * qv, qu * qv], axis=1)
    return fu_.astype(np.int64), fv_.astype(np.int64), w


def counts(p, n, x, m, inv_bin, W, signed_beta=True, min_cos=None):
    """The D integer counters (int64: a list has fewer than 2^24 entries of 2^32 each, so below 2^56 and never rounded) of one
    keypoint, and its contributing count c."""
    NV, D = shape(W, signed_beta)
    f = entry_coords(p, n, x, m, inv_bin, W, signed_beta, min_cos)
    keep = f["keep"]
    iu, iv, w = entry_weights(f["u"][keep], f["v"][keep])
    cnt = np.zeros(D, dtype=np.int64)
    base = iu * NV + iv
    for j, step in enumerate((0, NV, 1, NV + 1)):
        nz = w[:, j] != 0  # (a zero weight is not added: its node may lie outside the image)
        node = base[nz] + step
        assert node.size == 0 or (0 <= node.min() and node.max() < D)
        np.add.at(cnt, node, w[nz, j])
    return cnt, int(keep.sum())


def to_row(cnt, c, normalize=False, min_neighborhood_size=0):
    """The read-out of one keypoint's counters."""
    if c <= min_neighborhood_size:
        return np.zeros(len(cnt))
    as_double = cnt.astype(np.float64)  # (one correctly rounded conversion per node)
    if normalize:
        return as_double / (np.float64(c) * TWO32)
    return as_double * (1.0 / TWO32)


def rows(points, normals, keypoints, axes, lists, R, W=8, signed_beta=True, min_cos=None, normalize=False,
         min_neighborhood_size=0, return_counts=False, inv_bin=None):
    """The m x D rows of the neighbourhoods `lists` (index arrays into points) of the keypoints (m x 3) with axes (m x 3);
    normals may be None when min_cos is."""
    inv_bin = scale(R, W) if inv_bin is None else inv_bin
    NV, D = shape(W, signed_beta)
    points = np.asarray(points, dtype=np.float64)
    out = np.zeros((len(lists), D))
    cs = np.zeros(len(lists), dtype=np.int32)
    for i, nb in enumerate(lists):
        nb = np.asarray(nb, dtype=np.int64)
        if nb.size >= MAX_LIST:
            raise ValueError("a list of 2^24 entries or more")
        m = normals[nb] if normals is not None else np.zeros((nb.size, 3))
        cnt, c = counts(keypoints[i], axes[i], points[nb], m, inv_bin, W, signed_beta, min_cos)
        cs[i] = c
        out[i] = to_row(cnt, c, normalize, min_neighborhood_size)
    return (out, cs) if return_counts else out


def bilinear_float(p, n, x, m, inv_bin, W, signed_beta=True, min_cos=None):
    """The direct floating-point bilinear image of one keypoint, fractions unquantised: (D doubles, c).  Same contributing
    entries, weights (1 - fu)(1 - fv), fu (1 - fv), (1 - fu) fv, fu fv."""
    NV, D = shape(W, signed_beta)
    f = entry_coords(p, n, x, m, inv_bin, W, signed_beta, min_cos)
    keep = f["keep"]
    u, v = f["u"][keep], f["v"][keep]
    iu, iv = np.floor(u), np.floor(v)
    fu, fv = u - iu, v - iv
    base = iu.astype(np.int64) * NV + iv.astype(np.int64)
    img = np.zeros(D)
    for step, w in ((0, (1 - fu) * (1 - fv)), (NV, fu * (1 - fv)), (1, (1 - fu) * fv), (NV + 1, fu * fv)):
        nz = w != 0
        np.add.at(img, base[nz] + step, w[nz])
    return img, int(keep.sum())
