"""K6 (SPFH) bin decisions at the histogram edges on the GPU, against tests/golden/spfh_edges.npz (see
tests/test_spfh_edges_host.py for the contract): every case through compute_fpfh_descriptor and the Spfh export, with the
default dispatch and with each fast form switched off (SF_FPFH_NO_ALPHA_SHORTCUT, SF_FPFH_DENSE, SF_FPFH_NO_WINDOW); SPFH
bit for bit against the contract rows, FPFH within 1e-12 relative.  One case also through the sharded DescriptorJob (world 2).

One gap is allowed and pinned down: the device's atan2 is not correctly rounded, so a theta placed within a few ulps of a
(non-zero) interior theta edge may land on the other side of it than the C library's atan2 puts it.  Only the isolated pairs
of edge_pt_* / edge_a_* hold such thetas; a mismatch there must belong to such a pair, and every other row must match."""
import math

import numpy as np
import pytest

from conftest import load_golden
from test_spfh_edges_host import case_data, cases, expected, runs

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "no_shortcut": {"SF_FPFH_NO_ALPHA_SHORTCUT": "1"}, "dense": {"SF_FPFH_DENSE": "1"},
        "no_window": {"SF_FPFH_NO_WINDOW": "1"}}
FAMILIES = ["signed_zero", "edge_pt_", "edge_a_", "reach_", "plane_t", "theta_cancel_"]


@pytest.fixture(scope="module")
def G():
    return load_golden("spfh_edges.npz")


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


def close(got, want):
    return np.abs(got - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0))


def atan2_edge_points(G, case, n):
    """Points of an isolated-pair case (pairs stored as rows 2 t, 2 t + 1) whose pair has a contract theta, in either
    direction, within 4 ulps of a non-zero interior theta edge: where a not correctly rounded atan2 may decide otherwise."""
    if not case.startswith(("edge_pt_", "edge_a_")):
        return np.zeros(0, dtype=np.int64)
    p, nr = G[f"{case}_points"], G[f"{case}_normals"]
    et = np.linspace(-np.pi / 2, np.pi / 2, n + 1)[1:-1]
    et = et[et != 0.0]
    out = []
    for i in range(p.shape[0]):
        j = i ^ 1
        c, u, nj = p[j] - p[i], nr[i], nr[j]
        w = np.cross(u, np.cross(c, u))
        a = (nj[0] * w[0] + nj[2] * w[2]) + nj[1] * w[1]
        b = ((nj[0] * u[0] + nj[1] * u[1]) + nj[2] * u[2]) + 0.0
        t = math.atan2(a, b)
        if et.size and np.min(np.abs(t - et) / np.spacing(np.abs(et))) <= 4:
            out += [i, j]
    return np.unique(np.array(out, dtype=np.int64))


def mismatches(G, case, n, kp, sel, got, got_spfh, con, spfh):
    """Rows (of kp / of sel) that differ from the contract, and whether they all fall on atan2's allowance."""
    fr = np.flatnonzero([not close(got[t], con[t]) for t in range(len(kp))])
    sr = np.flatnonzero(np.any(got_spfh[sel] != spfh, axis=1))
    allowed = atan2_edge_points(G, case, n)
    return fr.size + sr.size, bool(np.isin(kp[fr], allowed).all() and np.isin(sel[sr], allowed).all())


def set_env(monkeypatch, env):
    for k in ("SF_FPFH_NO_ALPHA_SHORTCUT", "SF_FPFH_DENSE", "SF_FPFH_NO_WINDOW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("family", FAMILIES)
def test_k6_matches_the_contract_rows(G, eng, monkeypatch, family, env):
    import shot_fpfh_amd as s

    set_env(monkeypatch, env)
    bad, atan2_rows = [], 0
    for case in cases(G, family):
        p, nr, kp, sel = case_data(G, case)
        for j, r, n, nd in runs(G, case):
            con, _, spfh = expected(G, case, j, n, kp, sel, nd)
            got, got_spfh = s.compute_fpfh_descriptor(kp, p, nr, r, n, verbose=False, return_spfh=True, engine=eng)
            rows, allowed = mismatches(G, case, n, kp, sel, got, got_spfh, con, spfh)
            if rows and not allowed:
                bad.append((case, r, n, rows))
            atan2_rows += rows if allowed else 0
    assert not bad, f"{len(bad)} runs differ (case, radius, n_bins, rows): {bad[:12]}"
    print(f"{family} {env}: {atan2_rows} rows on atan2's allowance")


def test_spfh_export_and_the_forms_that_ran(G, eng, monkeypatch):
    """The Spfh table directly (windowed byte table for 9 / 11 bins, the alpha pair form for even counts, the generic kernels
    for 16), its export against the contract, and the profile report naming the K6 / K7 launches."""
    from shot_fpfh_amd.engine import Spfh

    set_env(monkeypatch, "default")
    seen = {}
    for case in ("edge_pt_4", "edge_pt_5", "edge_pt_9", "edge_pt_11", "edge_pt_16", "reach_11_0", "signed_zero"):
        p, nr, kp, sel = case_data(G, case)
        for j, r, n, nd in runs(G, case)[:3]:
            _, _, spfh = expected(G, case, j, n, kp, sel, nd)
            cloud = eng.cloud(p, nr)
            try:
                nb = cloud.radius_search_self(r)
                table = Spfh(cloud, n, nb.max_count, r)
                eng.sync(); eng.profile_reset(); eng.profile(True)
                table.compute(nb)
                eng.sync(); eng.profile(False)
                names = {k for k, v in eng.profile_report().items() if v[0]}
                got = table.export()
                seen[(case, n)] = (table.elem_bytes, names)
                sr = np.flatnonzero(np.any(got[sel] != spfh, axis=1))
                assert np.isin(sel[sr], atan2_edge_points(G, case, n)).all(), (case, r, n, sr)
                table.free()
                nb.free()
            finally:
                cloud.free()
    assert all("k6_spfh" in names for _, names in seen.values()), seen
    assert seen[("edge_pt_9", 9)][0] == 1 and seen[("edge_pt_11", 11)][0] == 1  # the windowed byte table
    assert seen[("edge_pt_16", 16)][0] == 4  # the generic kernels' 32-bit table
    assert seen[("edge_pt_4", 4)][0] == 1 and "k6_spfh_pack" in seen[("edge_pt_4", 4)][1]  # alpha pinned: blocks known


def test_sharded_job_on_one_device_matches_the_contract(G, eng):
    """One edge case through DescriptorJob in neighbour mode, two blocks on one device (world 2, halo exchange)."""
    from shot_fpfh_amd.sharding import DescriptorJob

    case = "signed_zero"
    p, nr, kp, sel = case_data(G, case)
    (j, r, n, nd), = [x for x in runs(G, case) if x[2] == 4]
    con, _, _ = expected(G, case, j, n, kp, sel, nd)
    got = np.full((p.shape[0], n**3), np.nan)
    for rank in range(2):
        job = DescriptorJob(eng, p, nr, r, n_bins=n, min_neighborhood_size=1, world=2, rank=rank, spfh_exchange="halo")
        job.step()
        got[job.block_original_indices()] = job.fpfh_out.to_host()
        job.close()
    assert close(got[kp], con)
