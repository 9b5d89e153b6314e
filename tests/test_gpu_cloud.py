"""The point-cloud stage on the MI355X (ssrlcv_hip_knn / _neighbor_distance_filter / _point_normals, csrc/cloud.hip) held
to the numpy restatement of its contract (tests/cloud_ref.py): k-NN bit for bit, filter mask and order exact, statistics
to 1e-12, normals to 1e-5 rad; then the real config[4] flow and the C++ MeshFactory."""
import os
import subprocess

import numpy as np
import pytest
import torch

import cloud_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


def _dev(p):
    return torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()


def _gpu_knn(capi, p, k, cell=0.0):
    nbr, d2, far = capi.knn(_dev(p), k, cell, far=True)
    return nbr.cpu().numpy().view(np.uint32), d2.cpu().numpy(), int(far.item())


def _cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "cube":
        return rng.random((20000, 3)).astype(np.float32)
    if name == "terrain":
        return R.terrain_cloud(40000, seed=3)[0]
    if name == "lattice":  # all ties: the index breaks them
        return np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    if name == "duplicates":
        return np.repeat(rng.random((1500, 3)).astype(np.float32), rng.integers(1, 6, 1500), 0)
    if name == "cell_boundaries":  # every coordinate a multiple of the explicit cell size 0.25
        return (rng.integers(0, 24, (6000, 3)) * 0.25).astype(np.float32)
    if name == "collinear":
        t = rng.random(3000).astype(np.float32) * 100
        return np.stack([t, 2 * t, -t], 1).astype(np.float32)
    if name == "k_plus_one":
        return rng.random((17, 3)).astype(np.float32)
    if name == "nonfinite":
        p = rng.random((5000, 3)).astype(np.float32)
        p[rng.integers(0, 5000, 120), rng.integers(0, 3, 120)] = np.nan
        p[rng.integers(0, 5000, 40), 0] = np.inf
        p[rng.integers(0, 5000, 40), 2] = -np.inf
        return p
    raise KeyError(name)


CASES = [("cube", 16, 0.0), ("cube", 5, 0.0), ("terrain", 16, 0.0), ("terrain", 32, 0.0), ("lattice", 8, 0.0),
         ("lattice", 26, 1.0), ("duplicates", 16, 0.0), ("cell_boundaries", 12, 0.25), ("cell_boundaries", 8, 0.0),
         ("collinear", 16, 0.0), ("k_plus_one", 16, 0.0), ("nonfinite", 16, 0.0), ("nonfinite", 1, 0.0)]


@pytest.mark.parametrize("name,k,cell", CASES)
def test_knn_bit_equal_to_reference(capi, name, k, cell):
    p = _cloud(name)
    nbr, d2, far = _gpu_knn(capi, p, k, cell)
    rn, rd = R.knn(p, k)
    bad = np.nonzero((nbr != rn).any(1) | (d2.view(np.uint32) != rd.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (name, len(bad), bad[:5], nbr[bad[:2]], rn[bad[:2]])


def test_knn_independent_of_cell_size(capi):
    """three explicit cell sizes (fine enough that many queries take the far path, about right, coarse) and automatic"""
    p = _cloud("terrain")
    base = _gpu_knn(capi, p, 16, 0.0)
    fars = []
    for cell in (0.01, 0.3, 3.0):
        got = _gpu_knn(capi, p, 16, cell)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)), cell
        fars.append(got[2])
    assert fars[0] > 0, fars   # the exact far scan was exercised
    print("far-path queries at cell 0.01 / 0.3 / 3.0 km / automatic: %s / %d of %d" % (fars, base[2], len(p)))


def test_two_runs_bit_identical(capi):
    p = _dev(R.terrain_cloud(100000, seed=11)[0])
    runs = []
    for _ in range(2):
        nbr, d2, _ = capi.knn(p, 16)
        out = capi.neighbor_distance_filter(p, d2, 16, 2.0)
        runs.append([nbr.cpu(), d2.cpu(), out["stats"].cpu(), out["mean"].cpu(), out["count"].cpu(),
                     out["index"].cpu()[: int(out["count"].item())]])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_filter_on_terrain_with_outliers(capi):
    """k = 16, sigma = 2 on terrain + 1 % outliers displaced 1-5 km: mask and kept order equal to the reference's for
    the GPU's own threshold, {mu, std} within 1e-12 of numpy float64, >= 99 % of the outliers and <= 5 % of the terrain
    removed (the reference on the CPU: 100 % and 0 % at 3e5 points); normals passed in are compacted alongside."""
    p, out, _ = R.terrain_cloud(300000, seed=5)
    pd = _dev(p)
    nbr, d2, _ = capi.knn(pd, 16)
    fake_normals = torch.arange(3 * len(p), dtype=torch.float32, device="cuda").view(-1, 3)
    res = capi.neighbor_distance_filter(pd, d2, 16, 2.0, fake_normals)
    rn, rd = R.knn(p, 16)
    assert np.array_equal(nbr.cpu().numpy().view(np.uint32), rn)
    m = res["mean"].cpu().numpy()
    rm = R.mean_distance(rd, 16)
    assert np.array_equal(m.view(np.uint32), rm.view(np.uint32))
    mu, std, t = res["stats"].cpu().numpy()
    rmu, rstd, _ = R.filter_stats(rm, 2.0)
    assert abs(mu - rmu) <= 1e-12 * abs(rmu) and abs(std - rstd) <= 1e-12 * abs(rstd), (mu, rmu, std, rstd)
    assert t == mu + np.float64(np.float32(2.0)) * std
    keep = R.filter_mask(rm, t)
    c = int(res["count"].item())
    idx = res["index"].cpu().numpy()[:c]
    assert c == keep.sum() and np.array_equal(idx, np.nonzero(keep)[0])
    assert np.array_equal(res["points"].cpu().numpy()[:c], p[idx])
    assert np.array_equal(res["normals"].cpu().numpy()[:c], fake_normals.cpu().numpy()[idx])
    removed_out, removed_terrain = (~keep[out]).mean(), (~keep[~out]).mean()
    print("filter: %.2f %% of %d outliers and %.3f %% of the terrain removed (mu %.4g std %.4g t %.4g km)" %
          (100 * removed_out, out.sum(), 100 * removed_terrain, mu, std, t))
    assert removed_out >= 0.99 and removed_terrain <= 0.05


def test_normals_against_eigh(capi):
    p, _, up = R.terrain_cloud(60000, seed=9)
    rng = np.random.default_rng(4)
    extra = np.repeat(p[:1] + np.float32(3.0) * up.astype(np.float32), 20, 0)    # 20 coincident points, away from all
    line = (p[1] + np.outer(rng.random(40), [0.05, 0.0, 0.0])).astype(np.float32)  # a collinear group
    bad = rng.random((30, 3)).astype(np.float32) + p[2]
    bad[:, 1] = np.nan
    cloud = np.concatenate([p, extra, line, bad]).astype(np.float32)
    vp = (cloud[:len(p)].astype(np.float64).mean(0) + 400.0 * up).astype(np.float32)
    k = 16
    pd = _dev(cloud)
    nbr, _, _ = capi.knn(pd, k, dist2=False)
    n = capi.point_normals(pd, nbr, k, vp).cpu().numpy().astype(np.float64)
    rn, gap = R.normals(cloud, nbr.cpu().numpy().view(np.uint32), k, vp)
    zero = (np.abs(rn).sum(1) == 0)
    assert np.array_equal(np.abs(n).sum(1) == 0, zero)
    assert zero[len(p):len(p) + 20].all() and zero[-30:].all()
    nz = ~zero
    assert np.allclose(np.linalg.norm(n[nz], axis=1), 1.0, atol=1e-6)
    good = nz & (gap > 1e-3)
    ang = np.arctan2(np.linalg.norm(np.cross(n[good], rn[good]), axis=1), (n[good] * rn[good]).sum(1))
    assert good.sum() > 0.9 * len(p) and ang.max() < 1e-5, (good.sum(), ang.max())
    to_v = vp.astype(np.float64) - cloud.astype(np.float64)
    dots = (n * to_v).sum(1) / np.linalg.norm(to_v, axis=1)
    sure = nz & (np.abs(dots) > 1e-6)
    assert (dots[sure] > 0).all()


def test_config4_flow_filter_cloud():
    """The 2048^2 config[4] pushbroom flow as test_config4_pushbroom_flow_against_ground_truth runs its filtered leg
    (twelve bundle-error passes), then pipeline.filter_cloud: the fraction within 0.2 km of the ground truth does not
    fall, and the kept points are an in-order subset."""
    import scene
    from ssrlcv_amd import pipeline
    from test_gpu_configs import _ground_truth_error
    S, V = 2048, 3
    imgs, pbs, rig, sc = scene.pushbroom_views(V, S)
    seed, _ = H.load_seed_features()
    res = pipeline.reconstruct(imgs, None, seed_features=seed, mode=0, pushbroom=pbs, filters=[("statistical", 3.0, 0.1)] * 12)
    mm, kp, pts_d = res["matches"], res["keypoints"], res["points"]
    pts = pts_d.cpu().numpy()
    err = _ground_truth_error(rig, sc, mm, kp, pts)
    f = pipeline.filter_cloud(pts_d, k=16, sigma=2.0)
    idx = f["index"].cpu().numpy()
    assert f["count"] == len(idx) > 0 and (np.diff(idx) > 0).all()
    assert np.array_equal(f["points"].cpu().numpy(), pts[idx])
    before, after = float((err < 0.2).mean()), float((err[idx] < 0.2).mean())
    print("config[4] flow: %d bundle-filtered points, %.2f %% within 0.2 km; after filter_cloud %d points, %.2f %%"
          % (len(pts), 100 * before, len(idx), 100 * after))
    assert after >= before


def test_mesh_factory_through_class_api(tmp_path):
    """MeshFactory (tests/cpp/mesh_factory_test.cpp): setPoints -> filterByNeighborDistance -> computeNormals -> savePoints
    gives the points, normals and statistics of pipeline.filter_cloud + pipeline.cloud_normals, bit for bit."""
    from ssrlcv_amd import pipeline
    p, _, up = R.terrain_cloud(50000, seed=13)
    vp = (p.astype(np.float64).mean(0) + 400.0 * up).astype(np.float32)
    path = str(tmp_path / "cloud.bin")
    with open(path, "wb") as fh:
        fh.write(np.uint64(len(p)).tobytes() + p.tobytes())
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "csrc"), "release"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "ssrlcv_amd", "host"), "_build/mesh_factory_test"])
    exe = os.path.join(H.ROOT, "ssrlcv_amd", "host", "_build", "mesh_factory_test")
    out = subprocess.check_output([exe, "run", path, str(tmp_path), "16", "2"] + ["%.9g" % v for v in vp]).decode()
    lines = out.splitlines()
    assert lines[-1] == "ok", out
    stats = [float(x) for x in next(l for l in lines if l.startswith("stats ")).split()[1:]]
    text = open(tmp_path / "cloud.ply").read().splitlines()
    head = text.index("end_header")
    assert "property float nx" in text[:head]
    rows = np.array([[np.float32(x) for x in l.split()] for l in text[head + 1:]], np.float32)
    f = pipeline.filter_cloud(_dev(p), k=16, sigma=2.0)
    nrm = pipeline.cloud_normals(f["points"], k=16, viewpoint=vp).cpu().numpy()
    assert np.array_equal(np.array(stats), np.array(f["stats"]))
    assert rows.shape == (f["count"], 6)
    assert np.array_equal(rows[:, :3], f["points"].cpu().numpy()) and np.array_equal(rows[:, 3:], nrm)
