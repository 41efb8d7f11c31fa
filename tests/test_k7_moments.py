"""The frame moments of the SHOT step taken from K7's weight pass (DescriptorJob._step_k7_moments, sf_fpfh_moments) against the
same build's usual order, K6 with the moments (SF_FPFH_NO_K7_MOMENTS=1): the moments, the frames, the FPFH rows and the SHOT
rows must be EQUAL, bit for bit -- the weight pass repeats K6's arithmetic on the same pairs in the same order.  And the
wave reductions rewritten on the lane-swap instructions against the rows the build before them returned.

Clouds (neighbourhood sizes counted from a search of their own, so that no case passes by never reaching the body it names):
uniform points in the unit cube with random unit normals at radii that give one, two and three chunks of 64 neighbours, one
with a handful of lists in a launch of their own (sf_dispatch::mid_sel), 64 duplicated points (neighbours at distance 0), a
point alone in its ball; and the cases the new order must decline: a list above 192 points, and a radius of 0.2 or more, at
which alpha is no longer pinned to one bin, K6's data decides the table's block mask and K7 runs its full form (the step then
computes the table a second time, with the moments)."""
import numpy as np
import pytest

from conftest import load_golden, synth_cloud

pytestmark = pytest.mark.gpu


def _with_duplicates():
    p, nr, rng = synth_cloud(4096, 11)
    pick = rng.choice(4096, 64, replace=False)
    return np.vstack([p, p[pick]]), np.vstack([nr, nr[pick]])


def _with_loner():
    p, nr, _ = synth_cloud(4096, 11)
    return np.vstack([p, [[1.5, 1.5, 1.5]]]), np.vstack([nr, [[0.0, 0.0, 1.0]]])


# name: (cloud, radius, the new order is taken, check of the neighbourhood sizes: (counts, longest) -> bool)
CASES = {
    "one_chunk": (lambda: synth_cloud(4096, 11)[:2], 0.12, True, lambda c, mx: 20 <= mx <= 64),
    "two_chunks": (lambda: synth_cloud(4096, 11)[:2], 0.175, True,
                   lambda c, mx: 64 < mx <= 128 and (c > 64).sum() > 2000 and (c <= 40).sum() > 100),
    "two_chunks_and_mid_launch": (lambda: synth_cloud(4096, 11)[:2], 0.18, True,
                                  lambda c, mx: 128 < mx <= 192 and 0 < (c > 128).sum() * 50 <= c.size),
    "three_chunks": (lambda: synth_cloud(4096, 11)[:2], 0.195, True, lambda c, mx: 128 < mx <= 192 and (c > 128).sum() * 50 > c.size),
    "duplicates": (_with_duplicates, 0.12, True, lambda c, mx: mx <= 64),
    "loner": (_with_loner, 0.12, True, lambda c, mx: c.min() == 1),
    "radius_unpins_alpha": (lambda: synth_cloud(3000, 11)[:2], 0.205, False, lambda c, mx: 128 < mx <= 192),
    "issue_radius_0.21": (lambda: synth_cloud(4096, 11)[:2], 0.21, False, lambda c, mx: mx > 128),
    "above_192": (lambda: synth_cloud(4096, 11)[:2], 0.24, False, lambda c, mx: mx > 192),
}


def _outputs(job):
    return {"moments": job.moments.to_host()[: job.m], "frames": job.lrf_out.to_host(), "fpfh": job.fpfh_out.to_host(),
            "shot": job.shot_out.to_host()}


def _run(eng, p, nr, radius, steps):
    """Outputs after each of `steps` passes of a fresh job (the first computes a new table, the later ones a resident one),
    and whether each pass took the frame moments from K7."""
    from shot_fpfh_amd.sharding import DescriptorJob

    job = DescriptorJob(eng, p, nr, radius, n_bins=5, normalize=True, min_neighborhood_size=10)
    try:
        res = []
        for _ in range(steps):
            job.step()
            res.append((job.last_k7_moments, _outputs(job)))
        return res
    finally:
        job.close()


@pytest.mark.parametrize("name", list(CASES))
def test_moments_from_k7_equal_k6s(name, monkeypatch):
    from shot_fpfh_amd.engine import default_engine

    make, radius, taken, sizes_ok = CASES[name]
    p, nr = make()
    eng = default_engine()
    cloud = eng.cloud(p, nr)
    try:
        cloud.build_grid(radius)
        nb = cloud.radius_search_self(radius, 0, cloud.n)
        try:
            counts, longest = nb.counts(), nb.max_count
        finally:
            nb.free()
    finally:
        cloud.free()
    hist = np.bincount(np.minimum((counts - 1) // 64, 4), minlength=5)
    print(name, "radius", radius, "longest", longest, "lists of 1, 2, 3, 4, more chunks", hist.tolist())
    assert longest == counts.max() and sizes_ok(counts, longest), (longest, hist.tolist())
    assert (counts == 1).any() == (name == "loner")

    monkeypatch.setenv("SF_FPFH_NO_K7_MOMENTS", "1")
    (old_taken, ref), = _run(eng, p, nr, radius, 1)
    assert not old_taken
    monkeypatch.delenv("SF_FPFH_NO_K7_MOMENTS")
    for step, (new_taken, got) in enumerate(_run(eng, p, nr, radius, 2)):
        assert new_taken == taken, (name, step)
        for key in ("moments", "frames", "fpfh", "shot"):
            assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (name, step, key)
    if name == "duplicates":  # (the pairs at distance 0 count in the moments: a frame of a duplicated point is not its twin's by accident)
        assert np.isfinite(ref["moments"]).all() and np.abs(ref["moments"]).max() > 0
    if name == "loner":
        assert (np.abs(ref["moments"]).sum(axis=1) == 0).sum() == 1  # its own list: all six moments exactly 0


def test_wave_sums_on_lane_swaps_keep_their_bits():
    """compute_normals(radius=): barycentre through sf_wave_sum4, covariance through sf_wave_sum8, on the rows recorded from the
    build before the reductions moved onto v_permlane32_swap / v_permlane16_swap (tools/gen_golden_k7_moments.py)."""
    import shot_fpfh_amd as s

    g = load_golden("normals_radius_sums.npz")
    p, _, _ = synth_cloud(2000, 29)
    for i, r in enumerate(g["radii"]):
        got = s.compute_normals(p, p, radius=float(r))
        assert np.array_equal(got, g[f"normals_{i}"]), (r, np.abs(got - g[f"normals_{i}"]).max())
