"""The sums and small fits that RANSAC (K11), FGR (K12), SC2 registration (K15) and ICP (I1, K17, K18) share, held to the bits the
MI355X returned before their block sums, Kabsch tails and refit sums were folded into one definition each
(tests/golden/registration_sums_pin.npz, written by tools/gen_golden_registration_pin.py).  Any change of an operation, of its
order or of the order of the additions in one of those kernels moves a bit here.

The inputs are integer arithmetic that is exact in float64 -- coordinates ((i i + 3 i + 1) K_c mod 2^20) / 2^20 with an odd K_c per
axis, moved by a quarter turn about z and a dyadic translation, with an exact offset on three rows of every four -- so they are
formed again here and only the results are stored; the ICP calls run on the inputs tests/golden/icp_plain_sums.npz already holds."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

PIN = "registration_sums_pin.npz"
R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
T0 = np.array([0.25, -0.5, 0.125])
RT0 = np.concatenate([R0.reshape(9), T0])
THR = 0.01            # keeps the untouched rows and the offsets of 1 .. 5 x 2^-10, drops 11 x 2^-10 and 8
REFIT_M = (1, 3, 64, 257, 70001)   # 70 001: past the 256 x 256 threads of one grid pass
DRAW_SIZES = tuple(range(3, 9))    # SF_RANSAC_MIN_DRAW_SIZE .. SF_RANSAC_MAX_DRAW_SIZE
HYP_M, HYP_LINE, EDGE_SIMILARITY = 64, 48, 0.9
FGR_K = (3, 257, 70001)            # (sf_fgr_sums refuses fewer than 3 rows)
FGR_STATE = np.concatenate([[0.5, 0.5, 0.5], [-0.25, 0.0, 0.625], [2.0], R0.reshape(9), [0.0, 0.0, 0.0], [0.25]])
SC2_M, SC2_SHARE = (3, 130, 470), 0.5
ICP_SCALE, ICP_TRIM = 0.02, 0.8
ICP_KEPT = ((134, 37), (397, 106), (120, 34))  # pairs inside d_max per (state, all rows / selection): icp_plain_sums.npz


def matched(m, line=None):
    """m matched pairs (a, b): b is a moved by (R0, T0) exactly; row i has on coordinate i % 3 of b the offset 0, 1 .. 5 x 2^-10, 8
    or 11 x 2^-10 for i % 4 = 0, 1, 2, 3.  `line` = (first, count): those rows lie on one line, untouched."""
    i = np.arange(m, dtype=np.int64)
    a = (((i * i + 3 * i + 1)[:, None] * np.array([421337, 736481, 918273])) % 2 ** 20) / 2.0 ** 20
    off = np.choose(i % 4, [np.zeros(m), ((7 * i) % 5 + 1) / 1024.0, np.full(m, 8.0), np.full(m, 11 / 1024.0)])
    if line:
        rows = np.arange(line[0], line[0] + line[1])
        a[rows] = np.column_stack([(rows - line[0]) / 16.0, np.full(line[1], 0.5), np.full(line[1], 0.25)])
        off[rows] = 0.0
    b = np.column_stack([0.25 - a[:, 1], a[:, 0] - 0.5, a[:, 2] + 0.125])
    b[i, i % 3] += off
    return a, b


def draws_of(size):
    """The draws of one size over the HYP_M rows of matched(HYP_M, line=(HYP_LINE, 16)): four of untouched rows, six of any rows,
    two on the line, one row three times over, and one each with the index m and -1."""
    j = np.arange(size)
    clean = [4 * ((d + 5 * j) % 12) for d in range(4)]
    mixed = [(11 * d + 3 * j + d * j) % HYP_LINE for d in range(6)]
    line = [HYP_LINE + (d + 5 * j) % 16 for d in range(2)]
    same = [np.full(size, 9)]
    bad = [np.where(j == 1, HYP_M, clean[0]), np.where(j == size - 1, -1, clean[1])]
    return np.array(clean + mixed + line + same + bad, dtype=np.int64)


def fgr_selection(k, m):
    sel = (np.arange(k, dtype=np.int64) ** 2 + 3 * np.arange(k, dtype=np.int64)) % m
    sel[k // 2] = m  # one row outside [0, m)
    return sel


def sc2_case(m, pad):
    """(seeds, rows) for sf_sc2_seed_fits on matched(m, line=(64, 16)) (m = 3: no line): made by hand, which the call allows."""
    j = np.arange(m, dtype=np.int64)
    if m == 3:
        seeds, body = [0, 1, -1, 2], [[0, 2, 2], [0, 0, 0], [0, 0, 0], [1, 0, 0]]
    else:
        seeds = [0, 64, -1, 7, 100, 3]
        body = [(j * 2654435761 + 40503) % 8,                 # about half the rows at share 0.5, offsets of every kind among them
                np.where((j > 64) & (j < 80), 3, 0),          # the line: no unique rotation
                np.zeros(m),                                  # no seed in this slot
                np.where(j == 8, 1, 0),                       # the seed and one more: fewer than three
                np.where(j % 4 == 0, 5, 0),                   # untouched rows only
                np.where(j % 4 < 2, 2 + j % 3, 0)]            # untouched rows and the small offsets
    rows = np.zeros((len(seeds), pad), dtype=np.uint32)
    rows[:, :m] = np.asarray(body)
    return np.array(seeds, dtype=np.int32), rows


class _Held:
    """Device arrays freed together."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def new(self, shape, dtype=np.float64, values=None):
        d = self.eng.empty(shape, dtype)
        self.held.append(d)
        return d if values is None else d.from_host(np.ascontiguousarray(values, dtype=dtype))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in self.held:
            h.free()


def record_refit(eng):
    out = {}
    a, b = matched(max(REFIT_M))
    with _Held(eng) as dev:
        da, db = dev.new(a.shape, values=a), dev.new(b.shape, values=b)
        for m in REFIT_M:
            out[f"refit_{m}"] = eng.ransac_refit_sums(da, db, m, RT0, THR)
    return out


def record_hypotheses(eng):
    out = {}
    a, b = matched(HYP_M, line=(HYP_LINE, 16))
    with _Held(eng) as dev:
        da, db = dev.new(a.shape, values=a), dev.new(b.shape, values=b)
        for size in DRAW_SIZES:
            draws = draws_of(size)
            n = draws.shape[0]
            status, rt = dev.new((n,), np.uint8, np.full(n, 9)), dev.new((n, 12), values=np.full((n, 12), 9.0))
            eng.ransac_hypotheses_device(da, db, HYP_M, dev.new(draws.shape, np.int64, draws), n, size, EDGE_SIMILARITY, status, rt)
            out[f"hyp_status_{size}"], out[f"hyp_rt_{size}"] = status.to_host(), rt.to_host()
    return out


def record_fgr(eng):
    """All rows, and a selection with repeats and one row outside [0, m): the call then fails AFTER it has written the sums."""
    out = {}
    a, b = matched(max(FGR_K))
    state = np.ascontiguousarray(FGR_STATE)
    with _Held(eng) as dev:
        da, db = dev.new(a.shape, values=a), dev.new(b.shape, values=b)
        for k in FGR_K:
            out[f"fgr_all_{k}"] = eng.fgr_sums(da, db, k, state)
            m = min(k + 2, 257)
            sums = np.zeros(32)
            rc = eng.lib.sf_fgr_sums(eng.h, da.ptr, db.ptr, m, dev.new((k,), np.int64, fgr_selection(k, m)).ptr, k,
                                     state.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p))
            assert rc == -1, rc  # SF_ERR_ARG: the row outside
            out[f"fgr_sel_{k}"] = sums
    return out


def record_sc2(eng):
    out = {}
    for m in SC2_M:
        a, b = matched(m, line=(64, 16) if m > 80 else None)
        seeds, rows = sc2_case(m, eng.sc2_padded(m))
        n = seeds.shape[0]
        with _Held(eng) as dev:
            res = [dev.new((n,), np.uint8, np.full(n, 9)), dev.new((n,), np.int32), dev.new((n, 12)), dev.new((n, 24)),
                   dev.new((n, m), np.uint8, np.full((n, m), 9))]
            eng.sc2_seed_fits_device(dev.new(a.shape, values=a), dev.new(b.shape, values=b), m, dev.new((n,), np.int32, seeds),
                                     dev.new(rows.shape, np.uint32, rows), n, SC2_SHARE, *res)
            for name, x in zip(("status", "size", "rt", "sums", "member"), res):
                out[f"sc2_{name}_{m}"] = x.to_host()
    return out


def record_icp(eng):
    """[mode, state, all rows / selection, 48] of sf_icp_accumulate_robust (Cauchy) and sf_icp_accumulate_trimmed (no loss)."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import LOSSES, _Registration

    g = load_golden("icp_plain_sums.npz")
    robust, trimmed = np.zeros((3, 3, 2, 48)), np.zeros((3, 3, 2, 48))
    reg = _Registration(g["scan"], g["ref"], g["ref_normals"], engine=eng, scan_normals=g["scan_normals"])
    try:
        for mode in range(3):
            for si in range(3):
                by = None if si == 0 else RigidTransform(g["rotations"][si], g["translations"][si])
                for ri, rows in enumerate((None, g["selection"])):
                    kw = dict(moved_by=by, rows=rows, epsilon=float(g["epsilon"]))
                    robust[mode, si, ri] = reg.pairs(mode, float(g["d_max"]), loss=LOSSES["cauchy"], scale=ICP_SCALE, **kw).raw
                    trimmed[mode, si, ri] = reg.pairs(mode, float(g["d_max"]), trim=ICP_TRIM, **kw).raw
    finally:
        reg.close()
    return dict(icp_robust=robust, icp_trimmed=trimmed)


RECORDERS = dict(refit=record_refit, hypotheses=record_hypotheses, fgr=record_fgr, sc2=record_sc2, icp=record_icp)


def record(eng):
    out = {}
    for fn in RECORDERS.values():
        out.update(fn(eng))
    return out


def stored_conditions(g):
    """What the pin asks of what it holds, without a device: every refit keeps some rows and, from 3 rows on, drops some; every
    draw size has every status; the FGR row counts are k and k - 1; the SC2 cases hold a fit, a set under three, a degenerate
    set and an empty slot; the ICP calls kept the fixture's pairs and the trimmed ones used a proper share of them."""
    for m in REFIT_M:
        kept = g[f"refit_{m}"][0]
        assert 0 < kept <= m and (m < 3 or kept < m), (m, kept)
        assert kept == np.count_nonzero(np.isin(np.arange(m) % 4, (0, 1)))
    for size in DRAW_SIZES:
        status, rt = g[f"hyp_status_{size}"], g[f"hyp_rt_{size}"]
        assert status.shape == (15,) and rt.shape == (15, 12) and set(status.tolist()) == {0, 1, 2, 3}, (size, status)
        assert list(status[:4]) == [0] * 4 and list(status[10:]) == [2, 2, 2, 3, 3] and not rt[status != 0].any()
    for k in FGR_K:
        assert g[f"fgr_all_{k}"][29] == k and g[f"fgr_sel_{k}"][29] == k - 1
        sel = fgr_selection(k, min(k + 2, 257))
        assert k < 257 or np.unique(sel).size < k - 1  # repeats
    for m in SC2_M:
        status, size, member = g[f"sc2_status_{m}"], g[f"sc2_size_{m}"], g[f"sc2_member_{m}"]
        assert {1, 3} <= set(status.tolist()) and (m == 3 or set(status.tolist()) == {0, 1, 2, 3}), (m, status)
        assert np.array_equal(member.sum(axis=1), size) and np.array_equal(size < 3, np.isin(status, (1, 3)))
        assert not g[f"sc2_rt_{m}"][status != 0].any() and not g[f"sc2_sums_{m}"][status == 3].any()
    assert g["icp_robust"][..., 0].tolist() == [[list(x) for x in ICP_KEPT]] * 3
    used, inside = g["icp_trimmed"][..., 0], g["icp_trimmed"][..., 37]
    assert inside.tolist() == [[list(x) for x in ICP_KEPT]] * 3 and np.all(used < inside) and np.all(used >= 0.75 * inside)


def test_the_pin_holds_what_it_is_meant_to():
    stored_conditions(load_golden(PIN))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(RECORDERS))
def test_registration_sums_are_the_recorded_bits(family):
    from shot_fpfh_amd.engine import default_engine

    want = load_golden(PIN)
    got = RECORDERS[family](default_engine())
    assert got and set(got) <= set(want.files)
    for name, x in got.items():
        assert x.dtype == want[name].dtype and np.array_equal(x, want[name]), (name, np.argwhere(x != want[name]).tolist())
