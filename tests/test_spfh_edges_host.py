"""SPFH bin decisions at the histogram edges, on the CPU (no GPU needed): the C oracle and the reference-shaped NumPy baseline
against tests/golden/spfh_edges.npz (tools/gen_golden_spfh_edges.py, the reference's own rows).

The pair features are alpha = v . n_j, phi = (c . u) / |c|, theta = atan2(n_j . w, n_j . u) (fpfh.py:52-57).  The reference
forms alpha and theta's numerator with np.einsum, (x0 y0 + x2 y2) + x1 y1, and phi's numerator and theta's denominator with
`.dot(u)`, an OpenBLAS gemv.  The contract the oracle and K6 keep: einsum's order bit for bit, the two dot products in
index order with a zero result made +0.0 (a BLAS accumulator starts from +0), theta from the C library's (correctly
rounded) atan2.  The fixture's contract rows are that; its reference rows differ from them only where gemv's rounding or
numpy's SIMD arctan2 moves a phi or theta bin (the generator asserts it and counts the rows), which happens on the tilted
planes at even bin counts, on a few pairs of general orientation and on a few exact theta edges."""
import numpy as np
import pytest

from conftest import load_golden

ISOLATED = ("signed_zero", "edge_pt_", "edge_a_", "reach_")


@pytest.fixture(scope="module")
def G():
    return load_golden("spfh_edges.npz")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def cases(G, prefixes=None):
    return [str(c) for c in G["cases"] if prefixes is None or str(c).startswith(prefixes)]


def dense(G, key, rows, n):
    out = np.zeros(rows * n**3)
    out[G[key + "_i"]] = G[key + "_v"]
    return out.reshape(rows, n**3)


def case_data(G, case):
    p, nr = G[f"{case}_points"], G[f"{case}_normals"]
    kp = G[f"{case}_kp"].astype(np.int64) if f"{case}_kp" in G else np.arange(p.shape[0])
    sel = G[f"{case}_spfh_sel"].astype(np.int64) if f"{case}_spfh_sel" in G else np.arange(p.shape[0])
    return p, nr, kp, sel


def runs(G, case):
    """(j, radius, n_bins, ndiff) of every run of a case."""
    return [(j, float(r), int(n), int(d)) for j, (r, n, d) in enumerate(G[f"{case}_runs"])]


def expected(G, case, j, n, kp, sel, ndiff):
    con = dense(G, f"{case}_r{j}_con", len(kp), n)
    ref = dense(G, f"{case}_r{j}_ref", len(kp), n) if ndiff else con
    return con, ref, dense(G, f"{case}_r{j}_spfh", len(sel), n)


def test_the_fixture_covers_what_it_should(G):
    names = cases(G)
    for n in (2, 3, 4, 5, 6, 7, 8, 9, 11, 16):
        assert f"edge_pt_{n}" in names and f"edge_a_{n}" in names
    for n in (2, 3, 4, 5, 6, 8, 9, 11):
        assert all(f"reach_{n}_{s}" in names for s in range(3))
    assert {"signed_zero", "plane_t0", "plane_t1", "plane_t2", "theta_cancel_0", "theta_cancel_1"} <= set(names)
    # the one place parity with the reference is out of reach: gemv's rounding on the planes at even bin counts
    for t in range(3):
        for j, _, n, nd in runs(G, f"plane_t{t}"):
            assert (nd == 0) == (n % 2 == 1), (t, n, nd)
    # isolated pairs with an axis-aligned u: the dot products are exact, reference == contract -- but for the odd exact theta
    # edge where numpy's SIMD arctan2 rounds an ulp away from the C library's (one pair: two rows)
    for case in cases(G, ("signed_zero", "reach_")):
        assert all(nd == 0 for _, _, _, nd in runs(G, case)), case
    assert sum(nd for c in cases(G, ("edge_pt_", "edge_a_")) for *_, nd in runs(G, c)) <= 8


@pytest.mark.parametrize("family", ["signed_zero", "edge_pt_", "edge_a_", "reach_", "plane_t", "theta_cancel_"])
def test_oracle_equals_the_contract_rows(G, O, family):
    """Every run: SPFH bit for bit, FPFH within 1e-12; and the reference's own rows wherever the fixture says they are the
    contract's (isolated pairs, odd-count planes)."""
    for case in cases(G, family):
        p, nr, kp, sel = case_data(G, case)
        for j, r, n, nd in runs(G, case):
            con, ref, spfh = expected(G, case, j, n, kp, sel, nd)
            got, got_spfh = O.compute_fpfh_descriptor(kp, p, nr, r, n, return_spfh=True)
            assert np.array_equal(got_spfh[sel], spfh), (case, r, n, np.flatnonzero(np.any(got_spfh[sel] != spfh, 1))[:8])
            assert np.abs(got - con).max() <= 1e-12, (case, r, n, np.abs(got - con).max())
            if not nd:
                assert np.abs(got - ref).max() <= 1e-12, (case, r, n)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_oracle_on_the_exact_tilted_plane(G, O, n):
    """The plane of 1 500 points with a constant normal: every feature is a rounding residue around 0.  Odd counts equal the
    reference row for row; even counts equal the contract (the reference's rows there move with gemv's rounding)."""
    p, nr, kp, sel = case_data(G, "plane_t0")
    (j, r, _, nd), = [x for x in runs(G, "plane_t0") if x[2] == n]
    con, ref, _ = expected(G, "plane_t0", j, n, kp, sel, nd)
    got = O.compute_fpfh_descriptor(kp, p, nr, r, n)
    assert np.abs(got - (ref if n % 2 else con)).max() <= 1e-12


def test_the_signed_zero_pair_of_the_issue(G, O):
    """Normals (-0, -0, -1) at i and (1, 0, 0) at j, 0.1 apart: j -> i has n . u = -0 in plain index order, and atan2(+0, -0)
    = pi would drop the pair; the reference's BLAS gives +0 and counts it (theta = 0)."""
    p, nr, _, _ = case_data(G, "signed_zero")
    for j, r, n, _ in runs(G, "signed_zero"):
        con = dense(G, f"signed_zero_r{j}_con", p.shape[0], n)[:2]
        got = O.compute_fpfh_descriptor(np.arange(2), p, nr, r, n)
        assert np.abs(got - con).max() <= 1e-12 and con[1].sum() > 0.0, n


@pytest.mark.parametrize("family", ISOLATED)
def test_numpy_shaped_baseline_equals_the_reference_rows(G, family):
    """oracle/numpy_shaped.py restates the reference with the same NumPy calls: on the isolated pairs its rows are the
    reference's (this guards the fixture as much as the baseline)."""
    from oracle.numpy_shaped import fpfh_numpy_shaped

    for case in cases(G, family):
        p, nr, kp, sel = case_data(G, case)
        for j, r, n, nd in runs(G, case)[:3]:
            _, ref, _ = expected(G, case, j, n, kp, sel, nd)
            got = fpfh_numpy_shaped(kp, p, nr, r, n)
            assert np.abs(got - ref).max() <= 1e-12, (case, r, n)
