"""K7 on the int8 matrix cores (k_fpfh_mc, k_fpfh_mc_sparse, k_fpfh_mcl: fpfh_mc.h, fpfh.hip) held to the bits the MI355X returned
before the pieces its four bodies share -- the LDS-DMA statement, the transposing read, the MFMA steps, the lane maps, the weight,
the exponent, 1 / k, the two recombinations, the own term and the row epilogue -- were given one definition each
(tests/golden/k7_rows_pin.npz, written by tools/gen_golden_k7_pin.py).  Any change of an operation or of the order of the additions in
one of the forms moves a bit here.

Per case the file holds the SHA-256 of the rows' bytes and of the list counts, the longest list, the K7 launch names the engine's
profiler reported, and 16 rows as uint64 for diagnosis; a case with the frame moments also the SHA-256 of the six moments of every
query and the moments of those 16 queries (all of them would be 288 KB a case).  The clouds are conftest's synth_cloud and
test_hip_round5's dense_cloud, formed again by whoever needs them.  Radii and seeds were chosen on the CPU from a float64 count of
the balls; what they were chosen for is asserted while recording (by the generator and by the test alike) and again on the file
(`stored_conditions`)."""
import hashlib
import os

import numpy as np
import pytest

from conftest import load_golden, synth_cloud

PIN = "k7_rows_pin.npz"
K7_NAMES = ("k7_fpfh", "k7_fpfh_mid", "k7_fpfh_tail")
SHORT_N, SHORT_SEED = 6000, 73
# chunks of 64 neighbours the longest list needs -> radius (all below 0.2: alpha stays in its central bin, at most two blocks live).
# Three and four chunks cross the refill of the sparse form's four-step buffer at step 4.
SHORT_RADII = {1: 0.10, 2: 0.15, 3: 0.175, 4: 0.19}
MOMENT_CHUNKS = (1, 2, 3)
INDEX_RADIUS, INDEX_M = SHORT_RADII[4], (1, 5, 203)
EDGE_LENGTHS = tuple(e + d for e in (32, 64, 96, 128, 192) for d in (-1, 0, 1))  # a step more or less of 32 neighbours
LONER = (1.5, 1.5, 1.5)
LONG_N, LONG_SEED = 30000, 22
LONG_RADII = {"random": 0.2, "consistent": 0.09}  # test_k7_matrix_core_form_for_long_lists
LONG_EDGES = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025)  # 256, 512: the super-chunks of the full and the sparse long form
WINDOW_BINS, WINDOW_RADII = (6, 7, 8), ((0.05, 1500), (0.17, 400))  # test_fpfh_six_to_eight_bins_...


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def _sample(m):
    return np.unique(np.linspace(0, m - 1, 16).astype(np.int64)) if m else np.zeros(0, dtype=np.int64)


class _Dense:
    """SF_FPFH_DENSE as a table is to be created under (spfh_create reads it): every block live, K7's full form."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.pop("SF_FPFH_DENSE", None)
        if self.on:
            os.environ["SF_FPFH_DENSE"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("SF_FPFH_DENSE", None)
        if self.old is not None:
            os.environ["SF_FPFH_DENSE"] = self.old


def _table(cloud, nb, n_bins, radius, dense=False):
    from shot_fpfh_amd.engine import Spfh

    with _Dense(dense):
        sp = Spfh(cloud, n_bins, nb.max_count, radius)
    return sp.compute(nb)


def _launched(eng, fn):
    """fn()'s result and the K7 launch names the profiler saw under it."""
    eng.profile(True)
    eng.profile_reset()
    try:
        res = fn()
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    return res, np.array(sorted(n for n, (launches, _) in rep.items() if n in K7_NAMES and launches > 0))


def _store(out, case, sp, rows, names, nb_counts, longest, moments=None):
    pick = _sample(rows.shape[0])
    out[f"{case}__elem_bytes"] = np.array([sp.elem_bytes], dtype=np.int64)
    out[f"{case}__rows_sha"], out[f"{case}__counts_sha"] = _sha(rows), _sha(np.asarray(nb_counts, dtype=np.int64))
    out[f"{case}__launches"], out[f"{case}__longest"] = names, np.array([longest], dtype=np.int64)
    out[f"{case}__rows16"] = np.ascontiguousarray(rows[pick]).view(np.uint64)
    if moments is not None:
        out[f"{case}__moments_sha"] = _sha(moments)
        out[f"{case}__moments16"] = np.ascontiguousarray(moments[pick]).view(np.uint64)


def _short_cloud(loner=False):
    p, nr, _ = synth_cloud(SHORT_N, SHORT_SEED)
    if loner:
        p, nr = np.vstack([p, [LONER]]), np.vstack([nr, [[0.0, 0.0, 1.0]]])
    return p, nr


def record_short(eng, chunks):
    """Every point a keypoint, lists of at most 64 `chunks` points: the sparse form, the full form (SF_FPFH_DENSE), and for up to
    three chunks the sparse form that carries the frame moments."""
    out = {}
    p, nr = _short_cloud()
    r = SHORT_RADII[chunks]
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(r)
        counts = nb.counts()
        assert 64 * (chunks - 1) < nb.max_count <= min(64 * chunks, 255) and nb.max_count == counts.max(), (chunks, nb.max_count)
        for dense in (False, True):
            sp = _table(cloud, nb, 5, r, dense)
            try:
                rows, names = _launched(eng, lambda: sp.fpfh(nb))
                _store(out, f"short{chunks}_{'dense' if dense else 'sparse'}", sp, rows, names, counts, nb.max_count)
                if not dense and chunks in MOMENT_CHUNKS:
                    assert sp.fpfh_carries_moments(nb)
                    d_rows, d_mom = eng.empty((nb.m, 125)), eng.empty((nb.m, 6))
                    try:
                        taken, names = _launched(eng, lambda: sp.fpfh_moments(nb, d_rows, d_mom))
                        assert taken
                        _store(out, f"moments{chunks}", sp, d_rows.to_host(), names, counts, nb.max_count, d_mom.to_host()[: nb.m])
                    finally:
                        d_rows.free()
                        d_mom.free()
            finally:
                sp.free()
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def index_keypoints(cnt):
    """203 keypoints of the cloud with the loner (its last point): one list of each of EDGE_LENGTHS (the first point that has it),
    the loner, and every 31st other point; 5: the loner and lists of 32, 64, 128, 192; 1: the loner."""
    edge = [int(np.flatnonzero(cnt == e)[0]) for e in EDGE_LENGTHS if (cnt == e).any()]
    head = edge + [SHORT_N]
    fill = [i for i in range(0, SHORT_N, 31) if i not in head]
    kp = np.array((head + fill)[: INDEX_M[2]], dtype=np.int64)
    return {1: kp[[len(edge)]], 5: kp[[len(edge), 1, 4, 10, 13]] if len(edge) == 15 else kp[:5], 203: kp}, cnt[edge]


def record_index(eng):
    """Keypoints by index (one launch of the four-chunk form: waves of a workgroup without a keypoint), a list that is its point
    alone among them (k = 1, every weight 0), and lists that end one before, at and one after a step of 32 neighbours."""
    out = {}
    p, nr = _short_cloud(loner=True)
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(INDEX_RADIUS)
        counts = nb.counts()
        cnt = counts[np.argsort(cloud.perm())]
        assert cnt[SHORT_N] == 1 and 192 < nb.max_count <= 255, (cnt[SHORT_N], nb.max_count)
        kps, found = index_keypoints(cnt)
        assert tuple(found.tolist()) == EDGE_LENGTHS, found.tolist()
        out["index__edge_lengths"] = found.astype(np.int64)
        sp = _table(cloud, nb, 5, INDEX_RADIUS)
        try:
            for m in INDEX_M:
                assert kps[m].shape == (m,) and np.unique(kps[m]).size == m and SHORT_N in kps[m]
                rows, names = _launched(eng, lambda: sp.fpfh(nb, kps[m]))
                _store(out, f"index{m}", sp, rows, names, counts, nb.max_count)
        finally:
            sp.free()
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def long_keypoints(cnt):
    """test_k7_matrix_core_form_for_long_lists's: the 60 longest and the 10 shortest lists, a dozen from two below each of
    LONG_EDGES on, 200 drawn."""
    order = np.argsort(cnt, kind="stable")
    picks = [order[-60:], order[:10]]
    for edge in LONG_EDGES:
        lo = np.searchsorted(cnt[order], edge - 2)
        picks.append(order[lo:lo + 12])
    return np.unique(np.concatenate(picks + [np.random.default_rng(3).choice(cnt.shape[0], 200, replace=False)]))


def record_long(eng, normals):
    """Lists above 255 points (k_fpfh_mcl, and the HI instantiations of the short forms beside it): keypoints by index and all
    points, on the table as K6 leaves it and with every block live."""
    from test_hip_round5 import dense_cloud

    out = {}
    p, nr = dense_cloud(LONG_N, LONG_SEED, normals == "consistent")
    r = LONG_RADII[normals]
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(r)
        counts = nb.counts()
        cnt = counts[np.argsort(cloud.perm())]
        assert cnt.max() > 600 and (cnt > 255).sum() > 1000, (cnt.max(), (cnt > 255).sum())
        kp = long_keypoints(cnt)
        out[f"long_{normals}__edge_lengths"] = np.intersect1d(cnt[kp], LONG_EDGES).astype(np.int64)
        for dense in (False, True):
            sp = _table(cloud, nb, 5, r, dense)
            try:
                for how, arg in (("index", kp), ("all", None)):
                    rows, names = _launched(eng, lambda: sp.fpfh(nb, arg))
                    assert "k7_fpfh_tail" in names, names
                    _store(out, f"long_{normals}_{how}_{'dense' if dense else 'table'}", sp, rows, names, counts, nb.max_count)
            finally:
                sp.free()
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def record_window(eng, n_bins):
    """6, 7 and 8 bins: a window of 72, 49 and 128 of the bins in the byte table -- rows with holes, and at 8 bins the padding
    column from a constant operand; at the second radius lists above 255 points.  (7 bins at that radius: alpha reaches three of
    its bins, 147 columns -- no window, the 16-bit table and the vector form of K7, k_fpfh, which shares the weight and 1 / k.)"""
    out = {}
    p, nr, rng = synth_cloud(20000, 40 + n_bins)
    cloud, nb = eng.cloud(p, nr), None
    try:
        for r, nkp in WINDOW_RADII:
            kp = np.sort(rng.choice(p.shape[0], nkp, replace=False))
            nb = cloud.radius_search_self(r)
            counts = nb.counts()
            assert (nb.max_count > 255) == (r > 0.1), (r, nb.max_count)
            sp = _table(cloud, nb, n_bins, r)
            try:
                for how, arg in (("index", kp), ("all", None)):
                    rows, names = _launched(eng, lambda: sp.fpfh(nb, arg))
                    assert rows.shape[1] == n_bins ** 3 and ("k7_fpfh_tail" in names) == (r > 0.1 and sp.elem_bytes == 1), names
                    _store(out, f"window{n_bins}_{r}_{how}", sp, rows, names, counts, nb.max_count)
            finally:
                sp.free()
            nb.free()
            nb = None
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


RECORDERS = {f"short{c}": (record_short, c) for c in SHORT_RADII}
RECORDERS["index"] = (record_index,)
RECORDERS.update({f"long_{k}": (record_long, k) for k in LONG_RADII})
RECORDERS.update({f"window{b}": (record_window, b) for b in WINDOW_BINS})


def record(eng, family=None):
    out = {}
    for name, (fn, *args) in RECORDERS.items():
        if family in (None, name):
            out.update(fn(eng, *args))
    return out


def stored_conditions(g):
    """What the pin asks of what it holds, without a device: every case of every family is there with its launches; the short
    cases have the longest lists they were chosen for; the full form's rows are the sparse form's and the rows with the moments the
    rows without; the keypoints by index hold every step edge; the long cases hold lists at the super-chunk sizes."""
    cases = sorted(k[: -len("__rows_sha")] for k in g.files if k.endswith("__rows_sha"))
    want = [f"short{c}_{f}" for c in SHORT_RADII for f in ("sparse", "dense")] + [f"moments{c}" for c in MOMENT_CHUNKS]
    want += [f"index{m}" for m in INDEX_M] + [f"long_{k}_{h}_{t}" for k in LONG_RADII for h in ("index", "all") for t in ("table", "dense")]
    want += [f"window{b}_{r}_{h}" for b in WINDOW_BINS for r, _ in WINDOW_RADII for h in ("index", "all")]
    assert cases == sorted(want), set(cases) ^ set(want)
    for c in cases:
        names = g[f"{c}__launches"].tolist()
        assert names and set(names) <= set(K7_NAMES) and g[f"{c}__rows_sha"].shape == (32,) and g[f"{c}__counts_sha"].shape == (32,), c
        assert 1 <= g[f"{c}__rows16"].shape[0] <= 16
    for c in SHORT_RADII:
        longest = int(g[f"short{c}_sparse__longest"][0])
        assert 64 * (c - 1) < longest <= min(64 * c, 255)
        assert np.array_equal(g[f"short{c}_sparse__rows_sha"], g[f"short{c}_dense__rows_sha"])
    for c in MOMENT_CHUNKS:
        assert np.array_equal(g[f"moments{c}__rows_sha"], g[f"short{c}_sparse__rows_sha"]) and g[f"moments{c}__moments16"].shape == (16, 6)
    assert tuple(g["index__edge_lengths"].tolist()) == EDGE_LENGTHS
    assert g["index1__rows16"].shape == (1, 125) and g["index203__launches"].tolist() == ["k7_fpfh"]
    for k in LONG_RADII:
        found = g[f"long_{k}__edge_lengths"].tolist()
        assert any(e in found for e in LONG_EDGES[:3]) and any(e in found for e in LONG_EDGES[3:6]), (k, found)
        for h in ("index", "all"):
            assert "k7_fpfh_tail" in g[f"long_{k}_{h}_table__launches"].tolist()
            assert np.array_equal(g[f"long_{k}_{h}_table__rows_sha"], g[f"long_{k}_{h}_dense__rows_sha"])
    for c in cases:
        assert int(g[f"{c}__elem_bytes"][0]) == (2 if c.startswith("window7_0.17") else 1), c
    for b in WINDOW_BINS:
        assert ("k7_fpfh_tail" in g[f"window{b}_0.17_all__launches"].tolist()) == (b != 7) and "k7_fpfh_tail" not in g[f"window{b}_0.05_all__launches"].tolist()
        assert g[f"window{b}_0.17_index__rows16"].shape[1] == b ** 3


def test_the_pin_holds_what_it_is_meant_to():
    stored_conditions(load_golden(PIN))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(RECORDERS))
def test_k7_rows_are_the_recorded_bits(family):
    from shot_fpfh_amd.engine import default_engine

    want = load_golden(PIN)
    got = record(default_engine(), family)
    assert got and set(got) <= set(want.files)
    for name, x in got.items():
        print(name, x.tolist() if x.size <= 32 else x.shape)
    for name, x in got.items():
        assert x.dtype == want[name].dtype and x.shape == want[name].shape and np.array_equal(x, want[name]), (
            name, np.argwhere(x != want[name]).tolist()[:8] if x.shape == want[name].shape else (x.shape, want[name].shape))
