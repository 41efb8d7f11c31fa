"""K5, the SHOT descriptor (k_shot_cached, k_shot_team, k_shot_long: shot.hip; k_shot_bins: shot_bins.hip), held to the bits the
MI355X returned before the pieces its four bodies share -- the neighbour geometry, the rule for who writes what, the gather of a
chunk, the prologue of the cached and team forms, the keypoint pick, the row epilogue, the Newton root -- were given one definition
each in shot_core.h (tests/golden/k5_rows_pin.npz, written by tools/gen_golden_k5_pin.py).  Any change of an operation or of the
order of the additions in one of the forms moves a bit here.

Per case the file holds the SHA-256 of the rows' bytes, of the frames' bytes where the call returns frames, and of the list counts,
the longest list, the K5 launch names the engine's profiler reported, and 16 rows as uint64 for diagnosis.  The clouds are
conftest's synth_cloud, formed again by whoever needs them.  Radii were chosen on the CPU from a float64 count of the balls; what
they were chosen for is asserted while recording (by the generator and by the test alike) and again on the file
(`stored_conditions`).

Two things the cases' plan could not have as written, and what stands in their place:
  * a radius search is always planned (plan_dispatch, search.hip), so its main launch is a cached instantiation and its long lists
    go to the tail launches: `k_shot_long<., false>` as "k5_shot" is reached by lists that were NOT searched for.  `stream_main`
    hands the lists of its radius search back through Cloud.import_neighbors, which dispatches by the longest list as a whole.
  * `short1`'s lists hold at most 64 points, so with min_neighborhood_size 100 its unfused rows are all zero.  The other three
    short cases pass the gate both ways at 100; `short1` records a second unfused run at min_neighborhood_size 25, which does."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, synth_cloud

PIN = "k5_rows_pin.npz"
K5_NAMES = ("k5_shot", "k5_shot_mid", "k5_shot_tail", "k5_shot_tail_stream", "k5_shot_bins")
SHORT_N, SHORT_SEED = 6000, 73
SHORT_RADII = {1: 0.10, 2: 0.15, 3: 0.175, 4: 0.19}  # test_hip_k7_pin's: chunks of 64 the longest list needs -> radius
SHORT1_GATE = 25  # (see above)
INDEX_RADIUS, INDEX_M = SHORT_RADII[4], (1, 5, 203)
EDGE_LENGTHS = tuple(e + d for e in (64, 128, 192) for d in (-1, 0, 1))
LONER, FAR = (1.5, 1.5, 1.5), (5.0, 5.0, 5.0)
TEAM_N = 14000
# case -> (mean_k of test_k5_team_of_waves_for_long_lists, the interval the longest list lies in, factor on that test's radius)
TEAM = {"team4": (380, 255, 768, 1.0), "team8": (800, 768, 1536, 1.0), "team16": (1500, 1536, 3072, 1.0),
        "stream_tail": (3300, 3072, 1 << 30, 1.0)}
TEAM_EDGES = (255, 256, 257, 320, 384, 385, 576, 577, 767, 768, 769, 960, 1152, 1153, 1535, 1536, 1537, 2048, 3071, 3072, 3073)
STREAM_MAIN = (4000, 61, 200, 0.3)  # test_shot_large_neighbourhoods_streaming_kernel: cloud, seed, keypoints, radius
BINS_N, BINS_SEED, BINS_RADIUS, BINS = 2000, 74, 0.27, (1, 2, 11, 12, 64)


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def _sample(m):
    return np.unique(np.linspace(0, m - 1, 16).astype(np.int64)) if m else np.zeros(0, dtype=np.int64)


def _launched(eng, fn):
    """fn()'s result and the K5 launch names the profiler saw under it."""
    eng.profile(True)
    eng.profile_reset()
    try:
        res = fn()
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    return res, np.array(sorted(n for n, (launches, _) in rep.items() if n in K5_NAMES and launches > 0))


def _store(out, case, rows, names, counts, longest, frames=None):
    out[f"{case}__rows_sha"], out[f"{case}__counts_sha"] = _sha(rows), _sha(np.asarray(counts, dtype=np.int64))
    out[f"{case}__launches"], out[f"{case}__longest"] = names, np.array([longest], dtype=np.int64)
    out[f"{case}__rows16"] = np.ascontiguousarray(rows[_sample(rows.shape[0])]).view(np.uint64)
    out[f"{case}__zero_rows"] = np.array([int((~np.any(rows, axis=1)).sum()), rows.shape[0]], dtype=np.int64)
    if frames is not None:
        out[f"{case}__frames_sha"] = _sha(frames)


def _fused(eng, nb, normalize, min_nb):
    """Neighbors.shot_single_scale with rows and frames: (rows, frames (m, 9)), launch names."""
    d_rows, d_lrf = eng.empty((max(nb.m, 1), 352)), eng.empty((max(nb.m, 1), 9))
    try:
        _, names = _launched(eng, lambda: nb.shot_single_scale(normalize, min_nb, out=d_rows, lrf_out=d_lrf))
        return (d_rows.to_host()[: nb.m].copy(), d_lrf.to_host()[: nb.m].copy()), names
    finally:
        d_rows.free()
        d_lrf.free()


def _unfused(eng, nb, normalize, min_nb):
    """shot_lrf, then shot on those frames: rows, launch names."""
    lrf = nb.shot_lrf()
    rows, names = _launched(eng, lambda: np.array(nb.shot(lrf, normalize, min_nb)))
    return rows, names


def _both(eng, out, case, nb, counts, fused_args, unfused_args):
    (rows, frames), names = _fused(eng, nb, *fused_args)
    _store(out, f"{case}_fused", rows, names, counts, nb.max_count, frames)
    rows, names = _unfused(eng, nb, *unfused_args)
    _store(out, f"{case}_unfused", rows, names, counts, nb.max_count)
    return rows


def _short_cloud(loner=False):
    p, nr, _ = synth_cloud(SHORT_N, SHORT_SEED)
    if loner:
        p, nr = np.vstack([p, [LONER]]), np.vstack([nr, [[0.0, 0.0, 1.0]]])
    return p, nr


def _gate_both_ways(rows, what):
    zero = int((~np.any(rows, axis=1)).sum())
    assert 0 < zero < rows.shape[0], (what, zero, rows.shape[0])


def record_short(eng, chunks):
    """Every point a keypoint, lists of at most 64 `chunks` points (k_shot_cached<chunks, .>, and <4, .> as k5_shot_mid where the
    search splits the launch): fused with rows and frames, and frames first then rows, where the gate is taken both ways."""
    out = {}
    p, nr = _short_cloud()
    r = SHORT_RADII[chunks]
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(r)
        counts = nb.counts()
        assert 64 * (chunks - 1) < nb.max_count <= min(64 * chunks, 255) and nb.max_count == counts.max(), (chunks, nb.max_count)
        rows = _both(eng, out, f"short{chunks}", nb, counts, (True, 5), (False, 100))
        if chunks == 1:
            assert not rows.any()  # (no list of more than 100 points)
            rows, names = _unfused(eng, nb, False, SHORT1_GATE)
            _store(out, "short1_unfused_gate", rows, names, counts, nb.max_count)
        _gate_both_ways(rows, f"short{chunks}")
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def index_queries(p, cnt):
    """203 external queries on the cloud with the loner (its last point): a point far from every other (k = 0), the loner (k = 1),
    one cloud point whose list has each of EDGE_LENGTHS, and every 31st other point; 5: the far point, the loner and lists of 64,
    128, 192; 1: the loner."""
    edge = [int(np.flatnonzero(cnt == e)[0]) for e in EDGE_LENGTHS if (cnt == e).any()]
    fill = [i for i in range(0, SHORT_N, 31) if i not in edge]
    rows = (edge + [SHORT_N] + fill)[: INDEX_M[2] - 1]
    q = np.vstack([[FAR], p[rows]])
    five = [0, len(edge) + 1, 2, 5, 8] if len(edge) == 9 else list(range(5))
    return {1: q[[len(edge) + 1]], 5: q[five], 203: q}, cnt[edge]


def record_index(eng):
    """External queries (Cloud.radius_search): an empty list (identity frame, zero row), a list of the point alone (the gate fails,
    the frame is still written), lists one below, at and one above 64, 128 and 192, and an odd number of queries, which leaves a wave
    of the last workgroup without a keypoint."""
    out = {}
    p, nr = _short_cloud(loner=True)
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(INDEX_RADIUS)
        cnt = nb.counts()[np.argsort(cloud.perm())]
        assert cnt[SHORT_N] == 1 and 192 < nb.max_count <= 255, (cnt[SHORT_N], nb.max_count)
        nb.free()
        nb = None
        queries, found = index_queries(p, cnt)
        assert tuple(found.tolist()) == EDGE_LENGTHS, found.tolist()
        out["index__edge_lengths"] = found.astype(np.int64)
        for m in INDEX_M:
            assert queries[m].shape == (m, 3)
            nb = cloud.radius_search(queries[m], INDEX_RADIUS)
            counts = nb.counts()
            if m == INDEX_M[2]:
                assert counts[0] == 0 and counts[10] == 1 and tuple(counts[1:10].tolist()) == EDGE_LENGTHS, counts[:11].tolist()
            _both(eng, out, f"index{m}", nb, counts, (True, 5), (False, 100))
            nb.free()
            nb = None
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def team_cloud(case):
    mean_k, _, _, factor = TEAM[case]
    p, nr, _ = synth_cloud(TEAM_N, 60 + mean_k)
    ext = p.max(0) - p.min(0)
    return p, nr, float((mean_k * ext.prod() / TEAM_N / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)) * 1.08 * factor


def team_keypoints(cnt, mean_k):
    """test_k5_team_of_waves_for_long_lists's: the 25 longest and the 5 shortest lists, 40 drawn, five around every boundary of
    the wave count."""
    order = np.argsort(cnt)
    picks = [order[-25:], order[:5], np.random.default_rng(mean_k).choice(cnt.shape[0], 40, replace=False)]
    for edge in TEAM_EDGES:
        lo = np.searchsorted(cnt[order], edge)
        picks.append(order[max(lo - 2, 0):lo + 3])
    return np.unique(np.concatenate(picks))


def record_team(eng, case):
    """Lists above 255 points: the team of 4, 8 or 16 waves (k_shot_team), and beyond 3 072 points the streaming form over the
    selection (k_shot_long<., true>): every point a keypoint, fused; a subset as external queries, frames first."""
    out = {}
    mean_k, lo, hi, _ = TEAM[case]
    p, nr, r = team_cloud(case)
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(r)
        counts = nb.counts()
        cnt = counts[np.argsort(cloud.perm())]
        assert lo < nb.max_count <= hi and nb.max_count == counts.max(), (case, nb.max_count)
        (rows, frames), names = _fused(eng, nb, True, 100)
        assert "k5_shot_tail" in names and ("k5_shot_tail_stream" in names) == (case == "stream_tail"), names
        _store(out, f"{case}_fused", rows, names, counts, nb.max_count, frames)
        nb.free()
        nb = cloud.radius_search(p[team_keypoints(cnt, mean_k)], r)
        rows, names = _unfused(eng, nb, True, 100)
        assert "k5_shot_tail" in names, names
        _store(out, f"{case}_unfused", rows, names, nb.counts(), nb.max_count)
        out[f"{case}__radius"] = np.array([r])
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def record_stream_main(eng):
    """The streaming form as the main launch (k_shot_long<., false>): lists of about 450 points that were not searched for, so
    that their longest list decides the form of all of them."""
    out = {}
    n, seed, nkp, r = STREAM_MAIN
    p, nr, rng = synth_cloud(n, seed)
    kp = p[rng.choice(n, nkp, replace=False)]
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search(kp, r)
        off, idx = nb.export()
        nb.free()
        nb = cloud.import_neighbors(kp, [idx[off[i]:off[i + 1]] for i in range(nkp)], r)
        assert nb.max_count > 256, nb.max_count
        rows = _both(eng, out, "stream_main", nb, nb.counts(), (True, 10), (False, 400))
        for f in ("fused", "unfused"):
            assert out[f"stream_main_{f}__launches"].tolist() == ["k5_shot"], out[f"stream_main_{f}__launches"]
        _gate_both_ways(rows, "stream_main")
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


def record_bins(eng):
    """The serial SHOT: k_shot_bins at 1, 2, 11, 12 and 64 cosine bins and the fixed-bin form, on lists that end in the first, the
    second and the third step of the sweep of 128."""
    out = {}
    p, nr, _ = synth_cloud(BINS_N, BINS_SEED)
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(BINS_RADIUS)
        counts = nb.counts()
        assert counts.min() < 64 and counts.max() > 128 and nb.max_count <= 255, (counts.min(), counts.max())
        for n in BINS:
            rows, names = _launched(eng, lambda: np.array(nb.shot_serial(10, n_cosine_bins=n)))  # (IndexError: SF_ERR_BIN_RANGE)
            assert rows.shape == (BINS_N, 32 * n) and names.tolist() == ["k5_shot_bins"], (rows.shape, names)
            _store(out, f"bins{n}", rows, names, counts, nb.max_count)
        rows, names = _launched(eng, lambda: np.array(nb.shot_serial(10)))
        assert "k5_shot" in names and "k5_shot_bins" not in names, names
        _store(out, "bins_fixed", rows, names, counts, nb.max_count)
        out["bins__shortest"] = np.array([counts.min()], dtype=np.int64)
    finally:
        if nb is not None:
            nb.free()
        cloud.free()
    return out


RECORDERS = {f"short{c}": (record_short, c) for c in SHORT_RADII}
RECORDERS["index"] = (record_index,)
RECORDERS.update({case: (record_team, case) for case in TEAM})
RECORDERS["stream_main"] = (record_stream_main,)
RECORDERS["bins"] = (record_bins,)


def record(eng, family=None):
    out = {}
    for name, (fn, *args) in RECORDERS.items():
        if family in (None, name):
            out.update(fn(eng, *args))
    return out


def stored_conditions(g):
    """What the pin asks of what it holds, without a device: every case of every family is there with its launches; the short
    cases have the longest lists they were chosen for, take the gate both ways and launch the four-chunk form over a selection at
    least once; the external queries hold every chunk edge, the empty list and the loner; the team cases have their longest list
    in their team's interval and only the last one streams; the streaming main launch is alone; the serial form's lists span
    three steps of its sweep."""
    cases = sorted(k[: -len("__rows_sha")] for k in g.files if k.endswith("__rows_sha"))
    pairs = [f"short{c}" for c in SHORT_RADII] + [f"index{m}" for m in INDEX_M] + list(TEAM) + ["stream_main"]
    want = [f"{c}_{f}" for c in pairs for f in ("fused", "unfused")] + ["short1_unfused_gate", "bins_fixed"] + [f"bins{n}" for n in BINS]
    assert cases == sorted(want), set(cases) ^ set(want)
    for c in cases:
        names = g[f"{c}__launches"].tolist()
        assert names and set(names) <= set(K5_NAMES) and g[f"{c}__rows_sha"].shape == (32,) and g[f"{c}__counts_sha"].shape == (32,), c
        assert 1 <= g[f"{c}__rows16"].shape[0] <= 16 and (f"{c}__frames_sha" in g.files) == c.endswith("_fused"), c
    zero = lambda c: tuple(g[f"{c}__zero_rows"].tolist())
    for c in SHORT_RADII:
        longest = int(g[f"short{c}_fused__longest"][0])
        assert 64 * (c - 1) < longest <= min(64 * c, 255)
        gate = "short1_unfused_gate" if c == 1 else f"short{c}_unfused"
        assert 0 < zero(gate)[0] < zero(gate)[1] == SHORT_N and zero(f"short{c}_fused")[1] == SHORT_N, (c, zero(gate))
    assert zero("short1_unfused") == (SHORT_N, SHORT_N)
    assert any("k5_shot_mid" in g[f"short{c}_{f}__launches"].tolist() for c in SHORT_RADII for f in ("fused", "unfused"))
    assert tuple(g["index__edge_lengths"].tolist()) == EDGE_LENGTHS
    assert g["index1_fused__rows16"].shape == (1, 352) and zero("index1_fused") == (1, 1)
    assert zero("index203_fused")[1] == 203 and zero("index203_fused")[0] >= 2 and zero("index5_unfused")[1] == 5
    for case, (_, lo, hi, _) in TEAM.items():
        for f in ("fused", "unfused"):
            names = g[f"{case}_{f}__launches"].tolist()
            assert "k5_shot_tail" in names and lo < int(g[f"{case}_{f}__longest"][0]) <= hi, (case, f, names)
        assert ("k5_shot_tail_stream" in g[f"{case}_fused__launches"].tolist()) == (case == "stream_tail"), case
        assert g[f"{case}__radius"].shape == (1,)
    for f in ("fused", "unfused"):
        assert g[f"stream_main_{f}__launches"].tolist() == ["k5_shot"] and int(g[f"stream_main_{f}__longest"][0]) > 256
    assert 0 < zero("stream_main_unfused")[0] < zero("stream_main_unfused")[1]
    assert int(g["bins__shortest"][0]) < 64 and 128 < int(g["bins_fixed__longest"][0]) <= 255
    for n in BINS:
        assert g[f"bins{n}__launches"].tolist() == ["k5_shot_bins"] and g[f"bins{n}__rows16"].shape[1] == 32 * n
    assert "k5_shot_bins" not in g["bins_fixed__launches"].tolist()


def test_the_pin_holds_what_it_is_meant_to():
    stored_conditions(load_golden(PIN))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(RECORDERS))
def test_k5_rows_are_the_recorded_bits(family):
    from shot_fpfh_amd.engine import default_engine

    want = load_golden(PIN)
    got = record(default_engine(), family)
    assert got and set(got) <= set(want.files)
    for name, x in got.items():
        print(name, x.tolist() if x.size <= 32 else x.shape)
    for name, x in got.items():
        assert x.dtype == want[name].dtype and x.shape == want[name].shape and np.array_equal(x, want[name]), (
            name, np.argwhere(x != want[name]).tolist()[:8] if x.shape == want[name].shape else (x.shape, want[name].shape))
