"""GPU parity: the HIP path, called through the C ABI, against the CPU oracle and the golden vectors.

Bars: indices (FPS, ball query, three_nn, top-k) and pure copies (gather/group) are BIT-EXACT;
gradients (fp32 atomics, order unspecified in the reference too) and MLP features are compared at
the tolerance BASELINE.json states (1e-4).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ext(dev):
    import spsnet_amd.pointnet2_batch_cuda as e
    return e


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    return gpu_util


@pytest.fixture
def mlp_precision(request):
    """Runs a test body in the requested grouped-MLP arithmetic (fused.set_precision) and restores the previous one."""
    from spsnet_amd import fused
    old = fused.set_precision(request.param)
    yield request.param
    fused.check_overflow()
    fused.set_precision(old)


BOTH_PRECISIONS = pytest.mark.parametrize("mlp_precision", ["fp32", "fp16x2"], indirect=True)


@pytest.fixture
def train_precision(request):
    """Runs a test body in the requested arithmetic of the fused TRAIN-mode kernels (fused.set_train_precision: "fp32" =
    exact, the reference's and the default; "fp16x2" = split-fp16 operands) and restores the previous one."""
    from spsnet_amd import fused
    old = fused.set_train_precision(request.param)
    yield request.param
    fused.set_train_precision(old)


BOTH_TRAIN_PRECISIONS = pytest.mark.parametrize("train_precision", ["fp32", "fp16x2"], indirect=True)
SPLIT_FP16_TRAINING = pytest.mark.parametrize("train_precision", ["fp16x2"], indirect=True)


def gather_xyz(xyz, idx):
    return np.take_along_axis(xyz, idx[..., None].astype(np.int64).repeat(3, axis=2), axis=1)


def cloud(rng, B, N, dup=0.0, lattice=False):
    if lattice:  # coordinates on a coarse lattice: masses of exactly equal distances
        xyz = rng.integers(-4, 5, (B, N, 3)).astype(np.float32) * 0.25
    else:
        xyz = rng.uniform(-3, 3, (B, N, 3)).astype(np.float32)
    if dup > 0:
        k = int(N * dup)
        for b in range(B):
            dst = rng.choice(N, k, replace=False)
            xyz[b, dst] = xyz[b, rng.integers(0, N, k)]
    return xyz


# ------------------------------------------------------------------ FPS
@pytest.mark.parametrize("N,m", [(1, 1), (2, 2), (3, 5), (37, 10), (63, 63), (64, 16), (65, 30), (100, 100),
                                 (511, 64), (512, 128), (1000, 200), (1023, 77), (1024, 256), (1025, 100),
                                 (2048, 512), (4096, 1024), (5000, 300), (9000, 200), (12288, 64), (16384, 512),
                                 (16385, 40), (20480, 50), (24576, 30)])
def test_fps_matches_oracle(ext, G, oracle, N, m):
    rng = np.random.default_rng(N * 7 + m)
    xyz = cloud(rng, 3, N, dup=0.1)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    got, got_t = G.fps(ext, xyz, m)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("N,m", [(30000, 40), (65536, 24)])
def test_fps_streaming_fallback(ext, G, oracle, N, m):
    xyz = cloud(np.random.default_rng(N), 2, N, dup=0.05)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    got, got_t = G.fps(ext, xyz, m)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("N", [48, 700, 1024, 4096, 16384])
def test_fps_all_ties_lattice(ext, G, oracle, N):
    # every step is decided by the block-size-dependent tie rule (bit-reversed thread, then index)
    xyz = cloud(np.random.default_rng(N + 1), 2, N, lattice=True)
    m = min(N, 200)
    np.testing.assert_array_equal(G.fps(ext, xyz, m)[0], oracle.fps(xyz, m))


def test_fps_respects_caller_temp(ext, G, oracle):
    rng = np.random.default_rng(5)
    xyz = cloud(rng, 2, 3000)
    temp = rng.uniform(0.0, 2.0, (2, 3000)).astype(np.float32)
    want, want_t = oracle.fps(xyz, 100, temp=temp, return_temp=True)
    got, got_t = G.fps(ext, xyz, 100, temp=temp)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)


def test_fps_nan_and_inf_points_never_win(ext, G, oracle):
    xyz = cloud(np.random.default_rng(6), 1, 2000)
    xyz[0, 5] = np.nan
    xyz[0, 900, 1] = np.inf
    np.testing.assert_array_equal(G.fps(ext, xyz, 64)[0], oracle.fps(xyz, 64))


@pytest.mark.parametrize("N,m", [(5, 3), (64, 20), (300, 64), (1024, 100), (2000, 50)])
def test_fps_with_dist(ext, G, oracle, N, m):
    rng = np.random.default_rng(N)
    d = rng.uniform(0, 4, (2, N, N)).astype(np.float32)
    d[:, :, N // 2] = d[:, :, 0]
    np.testing.assert_array_equal(G.fps_with_dist(ext, d, m), oracle.fps_with_dist(d, m))


def test_fps_kitti_full_size(ext, G, oracle):
    """BASELINE config 2, layer 0 and 1: 8 x 16 384 -> 4 096 -> 1 024, bit-exact."""
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 8, 16384, seed0=0, dup_fraction=0.01)
    i0 = G.fps(ext, xyz, 4096)[0]
    np.testing.assert_array_equal(i0, oracle.fps(xyz, 4096))
    # size-independent properties: distinct while distinct points remain, first index 0
    assert (i0[:, 0] == 0).all()
    x1 = gather_xyz(xyz, i0)
    i1 = G.fps(ext, x1, 1024)[0]
    np.testing.assert_array_equal(i1, oracle.fps(x1, 1024))


# ------------------------------------------------------------------ ball query
@pytest.mark.parametrize("N,M,r,ns", [(1, 1, 1.0, 4), (7, 3, 0.5, 1), (100, 64, 0.8, 16), (1000, 65, 0.5, 32),
                                      (4096, 512, 0.3, 16), (4097, 1000, 1.5, 32), (16384, 300, 0.2, 16), (50, 200, 9.0, 64)])
def test_ball_query(ext, G, oracle, N, M, r, ns):
    rng = np.random.default_rng(N + M)
    xyz = cloud(rng, 2, N, dup=0.05)
    new_xyz = np.concatenate([xyz[:, rng.integers(0, N, M // 2 + 1)], cloud(rng, 2, M, 0)], 1)[:, :M].copy()
    new_xyz[:, -1] = 100.0  # guaranteed empty ball
    np.testing.assert_array_equal(G.ball_query(ext, r, ns, xyz, new_xyz), oracle.ball_query(r, ns, xyz, new_xyz))


def test_ball_query_boundary_is_strict(ext, G, oracle):
    xyz = np.zeros((1, 6, 3), np.float32)
    xyz[0, :, 0] = [0.0, 0.5, 1.0, 1.5, 2.0, 0.25]
    ctr = np.array([[[0.0, 0, 0], [10.0, 0, 0], [1.0, 0, 0]]], np.float32)
    got = G.ball_query(ext, 1.0, 4, xyz, ctr)
    assert got[0].tolist() == [[0, 1, 5, 0], [0, 0, 0, 0], [1, 2, 3, 5]]
    np.testing.assert_array_equal(got, oracle.ball_query(1.0, 4, xyz, ctr))


def test_ball_query_leaves_empty_rows_untouched(ext, dev):
    xyz = torch.zeros(1, 4, 3, device=dev)
    ctr = torch.full((1, 2, 3), 50.0, device=dev)
    idx = torch.full((1, 2, 3), -7, dtype=torch.int32, device=dev)
    ext.ball_query_wrapper(1, 4, 2, 1.0, 3, ctr, xyz, idx)
    assert (idx == -7).all()  # the caller's zero-fill is what makes empty balls group point 0


@pytest.mark.parametrize("rmax,rmin", [(0.8, 0.0), (0.8, 0.3), (1.6, 0.8)])
def test_ball_query_dilated(ext, G, oracle, rmax, rmin):
    rng = np.random.default_rng(11)
    xyz = cloud(rng, 2, 3000, dup=0.1)
    new_xyz = xyz[:, rng.integers(0, 3000, 257)].copy()
    np.testing.assert_array_equal(G.ball_query(ext, rmax, 16, xyz, new_xyz, dilated_min=rmin),
                                  oracle.ball_query_dilated(rmax, rmin, 16, xyz, new_xyz))


# ------------------------------------------------------------------ ball query through the cell grid
@pytest.mark.parametrize("N,M,r,ns", [(1, 1, 1.0, 4), (7, 3, 0.5, 1), (100, 64, 0.8, 16), (1000, 65, 0.5, 32),
                                      (4097, 1000, 1.5, 32), (16384, 4100, 0.2, 16), (20000, 3000, 0.01, 3),
                                      (50, 200, 9.0, 64), (70000, 1500, 0.4, 16), (3000, 5000, 1e-4, 8),
                                      (5000, 2000, 1e6, 16)])
def test_ball_query_grid(ext, G, oracle, monkeypatch, N, M, r, ns):
    """csrc/ball_query_grid.hip against the oracle's scan: every launch forced through the grid, including sizes it
    would not normally take, radii far below / above the cloud's extent and a guaranteed-empty ball."""
    monkeypatch.setattr(ext, "BQ_GRID_MIN", (0, 0))
    rng = np.random.default_rng(N + M)
    xyz = cloud(rng, 2, N, dup=0.05)
    new_xyz = np.concatenate([xyz[:, rng.integers(0, N, M // 2 + 1)], cloud(rng, 2, M, 0)], 1)[:, :M].copy()
    new_xyz[:, -1] = 100.0
    np.testing.assert_array_equal(G.ball_query(ext, r, ns, xyz, new_xyz), oracle.ball_query(r, ns, xyz, new_xyz))


@pytest.mark.parametrize("rmax,rmin", [(0.8, 0.0), (0.8, 0.3), (1.6, 0.8)])
def test_ball_query_grid_dilated(ext, G, oracle, monkeypatch, rmax, rmin):
    monkeypatch.setattr(ext, "BQ_GRID_MIN", (0, 0))
    rng = np.random.default_rng(11)
    xyz = cloud(rng, 2, 3000, dup=0.1)
    new_xyz = xyz[:, rng.integers(0, 3000, 257)].copy()
    np.testing.assert_array_equal(G.ball_query(ext, rmax, 16, xyz, new_xyz, dilated_min=rmin),
                                  oracle.ball_query_dilated(rmax, rmin, 16, xyz, new_xyz))


@pytest.mark.parametrize("N,M,ra,nsa,rb,nsb", [(100, 64, 0.8, 16, 1.6, 32), (4097, 1000, 0.2, 16, 0.8, 32),
                                                (16384, 4100, 0.8, 32, 0.2, 16), (70000, 1500, 0.4, 8, 0.41, 8),
                                                (3000, 5000, 1.0, 64, 2.0, 3)])
def test_ball_query_grid_dual_radius(ext, G, oracle, monkeypatch, dev, N, M, ra, nsa, rb, nsb):
    """sps_ball_query_grid2 (two radii from one walk) against two oracle scans; every row written."""
    monkeypatch.setattr(ext, "BQ_GRID_MIN", (0, 0))
    rng = np.random.default_rng(N + M)
    xyz = cloud(rng, 2, N, dup=0.05)
    new_xyz = np.concatenate([xyz[:, rng.integers(0, N, M // 2 + 1)], cloud(rng, 2, M, 0)], 1)[:, :M].copy()
    new_xyz[:, -1] = 100.0
    ia, ib = ext.ball_query_full2(ra, nsa, rb, nsb, G.t(xyz), G.t(new_xyz))
    np.testing.assert_array_equal(G.n(ia), oracle.ball_query(ra, nsa, xyz, new_xyz))
    np.testing.assert_array_equal(G.n(ib), oracle.ball_query(rb, nsb, xyz, new_xyz))


def test_ball_query_grid_self_query_lidar(ext, G, oracle, dev):
    """The DenseEdgeConv launch (surface_feature.py:55): every point is a centroid (same tensor), r = 0.8, K = 16, on
    LiDAR-like scenes -- the default route of ball_query_wrapper at this size; rows of empty balls stay untouched."""
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 3, 16384, seed0=5, dup_fraction=0.01)
    x = G.t(xyz)
    idx = torch.zeros((3, 16384, 16), dtype=torch.int32, device=dev)
    assert ext.BQ_GRID_MIN is not None and 16384 >= max(ext.BQ_GRID_MIN)
    ext.ball_query_wrapper(3, 16384, 16384, 0.8, 16, x, x, idx)
    np.testing.assert_array_equal(G.n(idx), oracle.ball_query(0.8, 16, xyz, xyz))
    far = torch.full((1, 2048, 3), 500.0, device=dev)
    keep = torch.full((1, 2048, 4), -7, dtype=torch.int32, device=dev)
    ext.ball_query_wrapper(1, 16384, 2048, 0.8, 4, far, x[:1].contiguous(), keep)
    assert (keep == -7).all()


def test_ball_query_grid_degenerate_clouds(ext, G, oracle, monkeypatch):
    """All points identical, points on a line, NaN / inf coordinates in points and centroids: same rows as the scan."""
    monkeypatch.setattr(ext, "BQ_GRID_MIN", (0, 0))
    rng = np.random.default_rng(3)
    same = np.full((1, 3000, 3), 1.25, np.float32)
    line = np.zeros((1, 3000, 3), np.float32); line[0, :, 1] = rng.permutation(3000) * 0.01
    bad = cloud(rng, 1, 3000, dup=0.02)
    bad[0, 5] = np.nan; bad[0, 17, 1] = np.inf; bad[0, 99, 2] = -np.inf; bad[0, 1234, 0] = np.nan
    for xyz in (same, line, bad):
        ctr = xyz[:, rng.integers(0, 3000, 700)].copy()
        ctr[0, 3] = np.nan; ctr[0, 8, 0] = np.inf
        with np.errstate(invalid="ignore", over="ignore"):
            want = oracle.ball_query(0.3, 16, xyz, ctr)
        np.testing.assert_array_equal(G.ball_query(ext, 0.3, 16, xyz, ctr), want)


# ------------------------------------------------------------------ gather / group (+grad)
@pytest.mark.parametrize("C,N,M,ns", [(1, 10, 4, 1), (3, 1000, 333, 16), (67, 4096, 1024, 32), (259, 512, 256, 16)])
def test_group_and_gather(ext, G, oracle, C, N, M, ns):
    rng = np.random.default_rng(C + N)
    pts = rng.normal(size=(2, C, N)).astype(np.float32)
    idx = rng.integers(0, N, (2, M, ns)).astype(np.int32)
    np.testing.assert_array_equal(G.group(ext, pts, idx), oracle.group_points(pts, idx))
    np.testing.assert_array_equal(G.gather(ext, pts, idx[:, :, 0].copy()), oracle.gather_points(pts, idx[:, :, 0]))


def test_group_gather_gradients(ext, G, oracle, dev):
    rng = np.random.default_rng(3)
    B, C, N, M, ns = 2, 19, 700, 130, 16
    idx = rng.integers(0, N, (B, M, ns)).astype(np.int32)
    go = rng.normal(size=(B, C, M, ns)).astype(np.float32)
    gp = torch.zeros(B, C, N, device=dev)
    ext.group_points_grad_wrapper(B, C, N, M, ns, G.t(go), G.t(idx), gp)
    np.testing.assert_allclose(G.n(gp), oracle.group_points_grad(go, idx, N), rtol=1e-5, atol=1e-5)
    gi = idx[:, :, 0].copy()
    go2 = rng.normal(size=(B, C, M)).astype(np.float32)
    gp2 = torch.zeros(B, C, N, device=dev)
    ext.gather_points_grad_wrapper(B, C, N, M, G.t(go2), G.t(gi), gp2)
    np.testing.assert_allclose(G.n(gp2), oracle.gather_points_grad(go2, gi, N), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ three_nn / interpolate
@pytest.mark.parametrize("n,m", [(1, 1), (10, 2), (300, 3), (1000, 257), (4096, 1024), (700, 2048), (300, 2049), (5000, 4099)])
def test_three_nn_and_interpolate(ext, G, oracle, dev, n, m):
    rng = np.random.default_rng(n + m)
    unknown = cloud(rng, 2, n, lattice=True)
    known = cloud(rng, 2, m, lattice=True)
    d2 = torch.empty(2, n, 3, device=dev)
    idx = torch.empty(2, n, 3, dtype=torch.int32, device=dev)
    ext.three_nn_wrapper(2, n, m, G.t(unknown), G.t(known), d2, idx)
    want_d2, want_idx = oracle.three_nn(unknown, known)
    np.testing.assert_array_equal(G.n(idx), want_idx)
    np.testing.assert_array_equal(G.n(d2), want_d2)
    feats = rng.normal(size=(2, 9, m)).astype(np.float32)
    w = rng.uniform(0, 1, (2, n, 3)).astype(np.float32)
    out = torch.empty(2, 9, n, device=dev)
    ext.three_interpolate_wrapper(2, 9, m, n, G.t(feats), idx, G.t(w), out)
    np.testing.assert_array_equal(G.n(out), oracle.three_interpolate(feats, want_idx, w))
    go = rng.normal(size=(2, 9, n)).astype(np.float32)
    gp = torch.zeros(2, 9, m, device=dev)
    ext.three_interpolate_grad_wrapper(2, 9, n, m, G.t(go), idx, G.t(w), gp)
    np.testing.assert_allclose(G.n(gp), oracle.three_interpolate_grad(go, want_idx, w, m), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ score + top-k sampler
@pytest.mark.parametrize("N,K,C", [(2, 1, 1), (100, 100, 3), (512, 256, 3), (1000, 300, 2), (1024, 512, 3),
                                   (4096, 2048, 3), (16384, 4096, 1)])
def test_score_topk_bit_exact(ext, G, oracle, N, K, C):
    rng = np.random.default_rng(N + K)
    cls = rng.normal(size=(2, N, C)).astype(np.float32) * 3
    if N > 8:
        cls[:, ::7] = cls[:, 3:4]  # exact score ties -> index-ascending rule
    stds = rng.uniform(0, 40, (2, N)).astype(np.float32)
    idx, sc = ext.score_topk(G.t(cls), K, return_scores=True)
    want_s = oracle.score_ctr(cls)
    np.testing.assert_array_equal(G.n(sc), want_s)
    np.testing.assert_array_equal(G.n(idx), oracle.topk_desc(want_s, K))
    idx, sc = ext.score_topk(G.t(cls), K, stds=G.t(stds), return_scores=True)
    want_s = oracle.score_stability(cls, stds)
    np.testing.assert_array_equal(G.n(sc), want_s)
    np.testing.assert_array_equal(G.n(idx), oracle.topk_desc(want_s, K))


def test_score_topk_saturated_logits(ext, G, oracle):
    cls = np.array([[[-200.0], [200.0], [90.0], [-90.0], [0.0], [200.0]]], np.float32)
    idx, sc = ext.score_topk(G.t(cls), 6, return_scores=True)
    np.testing.assert_array_equal(G.n(sc), oracle.score_ctr(cls))
    np.testing.assert_array_equal(G.n(idx), oracle.topk_desc(oracle.score_ctr(cls), 6))


@pytest.mark.parametrize("N,K", [(600, 64), (1024, 512), (5000, 1000)])
def test_score_topk_nan_scores_are_sampled_first(ext, G, oracle, N, K):
    """torch.max keeps a NaN class score and torch.topk ranks NaN above every number (pointnet2_modules.py:288-291,
    296-302): points with a NaN among their class scores -- or a NaN stability -- lead the sample, in index order; both
    kernels (ranking up to 2048 points, bitonic sort beyond) against the oracle."""
    rng = np.random.default_rng(N)
    cls = rng.normal(size=(2, N, 3)).astype(np.float32)
    stds = rng.uniform(0, 40, (2, N)).astype(np.float32)
    cls[0, [5, 77, N - 1], [0, 2, 1]] = np.nan
    cls[1, 9, 1] = -np.nan
    stds[1, 300] = np.nan
    for kw in ({}, {"stds": G.t(stds)}):
        idx, sc = ext.score_topk(G.t(cls), K, return_scores=True, **kw)
        want_s = oracle.score_stability(cls, stds) if kw else oracle.score_ctr(cls)
        np.testing.assert_array_equal(np.isnan(G.n(sc)), np.isnan(want_s))
        np.testing.assert_array_equal(G.n(idx), oracle.topk_desc(want_s, K))
        assert G.n(idx)[0, :3].tolist() == [5, 77, N - 1]
        assert G.n(idx)[1, :2].tolist() == ([9, 300] if kw else [9, int(G.n(idx)[1, 1])])


# ------------------------------------------------------------------ fused query+group
@pytest.mark.parametrize("C,use_xyz", [(0, True), (1, True), (5, True), (64, True), (7, False)])
def test_query_and_group_fused(ext, G, oracle, C, use_xyz):
    rng = np.random.default_rng(C)
    xyz = cloud(rng, 2, 2000, dup=0.05)
    new_xyz = xyz[:, rng.integers(0, 2000, 301)].copy()
    new_xyz[:, 7] = 99.0
    feats = rng.normal(size=(2, C, 2000)).astype(np.float32) if C else None
    out, idx = ext.query_and_group(0.7, 16, G.t(xyz), G.t(new_xyz), None if feats is None else G.t(feats), use_xyz)
    want_idx = oracle.ball_query(0.7, 16, xyz, new_xyz)
    np.testing.assert_array_equal(G.n(idx), want_idx)
    parts = []
    if use_xyz:
        parts.append(oracle.group_points(np.ascontiguousarray(xyz.transpose(0, 2, 1)), want_idx)
                     - new_xyz.transpose(0, 2, 1)[..., None])
    if C:
        parts.append(oracle.group_points(feats, want_idx))
    np.testing.assert_array_equal(G.n(out), np.concatenate(parts, 1))


# ------------------------------------------------------------------ golden vectors (reference Python layers)
def _load_sd(mod, g):
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    mod.load_state_dict(sd, strict=True)
    return mod


def topk_equivalent(mine, ref, ref_scores, tol):
    for b in range(ref.shape[0]):
        for r in np.flatnonzero(mine[b] != ref[b]):
            assert abs(float(ref_scores[b, mine[b, r]]) - float(ref_scores[b, ref[b, r]])) <= tol, (b, r)


def test_golden_ops_small(ext, G, dev):
    from spsnet_amd import pointnet2_utils as U
    g = np.load(os.path.join(GOLD, "ops_small.npz"))
    xyz, feats = G.t(g["xyz"]), G.t(g["feats"])
    idx = U.furthest_point_sample(xyz, 64)
    np.testing.assert_array_equal(G.n(idx), g["fps_idx"])
    new_xyz = U.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    np.testing.assert_array_equal(G.n(new_xyz), g["new_xyz"])
    np.testing.assert_array_equal(G.n(U.ball_query(0.3, 8, xyz, new_xyz)), g["bq"])
    np.testing.assert_array_equal(G.n(U.ball_query_dilated(0.4, 0.1, 8, xyz, new_xyz)), g["bqd"])
    np.testing.assert_array_equal(G.n(U.ball_query_dilated(0.3, 0.0, 8, xyz, new_xyz)), g["bqd0"])
    np.testing.assert_array_equal(G.n(U.grouping_operation(feats, G.t(g["bq"]))), g["grouped"])
    with torch.no_grad():
        np.testing.assert_array_equal(G.n(U.QueryAndGroup(0.3, 8)(xyz, new_xyz, feats)), g["qg"])
        np.testing.assert_array_equal(G.n(U.QueryAndGroup(0.3, 8)(xyz, new_xyz, None)), g["qg_nofeat"])
    fr = feats.clone().requires_grad_(True)  # autograd path (unfused)
    np.testing.assert_array_equal(G.n(U.QueryAndGroup(0.3, 8)(xyz, new_xyz, fr)), g["qg"])
    dist, nn_idx = U.three_nn(G.t(g["unknown"]), new_xyz)
    np.testing.assert_array_equal(G.n(nn_idx), g["nn_idx"])
    np.testing.assert_allclose(G.n(dist), g["nn_dist"], rtol=2e-7)
    np.testing.assert_array_equal(G.n(U.three_interpolate(G.t(g["known_feats"]), nn_idx, G.t(g["interp_w"]))), g["interp"])
    np.testing.assert_array_equal(G.n(U.furthest_point_sample_with_dist(G.t(g["dmat"]), 16)), g["fps_d"])
    f2 = feats.clone().requires_grad_(True)
    U.grouping_operation(f2, G.t(g["bq"])).backward(G.t(g["group_go"]))
    np.testing.assert_allclose(G.n(f2.grad), g["group_grad"], rtol=1e-5, atol=1e-5)
    f3 = feats.clone().requires_grad_(True)
    U.gather_operation(f3, idx).backward(G.t(g["gather_go"]))
    np.testing.assert_allclose(G.n(f3.grad), g["gather_grad"], rtol=1e-5, atol=1e-5)
    k2 = G.t(g["known_feats"]).requires_grad_(True)
    U.three_interpolate(k2, nn_idx, G.t(g["interp_w"])).backward(G.t(g["interp_go"]))
    np.testing.assert_allclose(G.n(k2.grad), g["interp_grad"], rtol=1e-4, atol=1e-5)


SA_CASES = {
    "config1_sa": dict(npoint_list=[512], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.8], nsamples=[16],
                       mlps=[[1, 16, 16, 32]], aggregation_mlp=[32], confidence_mlp=[16]),
    "sampler_ctr": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['ctr_aware'], radii=[1.6, 4.8],
                        nsamples=[8, 16], mlps=[[6, 8, 16], [6, 8, 24]], aggregation_mlp=[32], confidence_mlp=[16]),
    "sampler_sss": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['sss_aware'], radii=[1.6, 4.8],
                        nsamples=[8, 16], mlps=[[6, 8, 16], [6, 8, 24]], aggregation_mlp=[32], confidence_mlp=[16]),
    "sampler_nogroup": dict(npoint_list=[128], sample_range_list=[-1], sample_type_list=['ctr_aware'], radii=[],
                            nsamples=[], mlps=[], aggregation_mlp=[32], confidence_mlp=None),
    "sampler_dfps_stds_dilated": dict(npoint_list=[128], sample_range_list=[-1], sample_type_list=['D-FPS'],
                                      radii=[0.8, 1.6], nsamples=[8, 8], mlps=[[6, 8, 8], [6, 8, 8]], dilated_group=True,
                                      aggregation_mlp=[16], confidence_mlp=None),
    "sampler_ffps": dict(npoint_list=[64], sample_range_list=[-1], sample_type_list=['F-FPS'], radii=[8.0], nsamples=[8],
                         mlps=[[4, 8, 8]], aggregation_mlp=None, confidence_mlp=None),
    "sampler_fs": dict(npoint_list=[32], sample_range_list=[-1], sample_type_list=['FS'], radii=[8.0], nsamples=[8],
                       mlps=[[4, 8, 8]], aggregation_mlp=None, confidence_mlp=None),
    # the dispatcher's remaining branches (reference :314-419): S-FPS below / above its 3500-distinct-picks fallback,
    # ds-FPS and ry-FPS (FPS inside four sorted partitions)
    "sampler_sfps_fallback": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['S-FPS'], radii=[1.6],
                                  nsamples=[8], mlps=[[2, 8, 8]], aggregation_mlp=None, confidence_mlp=None,
                                  ss_radii=[0.8], ss_nsamples=[8]),
    "sampler_sfps": dict(npoint_list=[4096], sample_range_list=[-1], sample_type_list=['S-FPS'], radii=[1.6], nsamples=[8],
                         mlps=[[2, 8, 8]], aggregation_mlp=None, confidence_mlp=None, ss_radii=[0.15], ss_nsamples=[4]),
    "sampler_dsfps": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['ds-FPS'], radii=[1.6], nsamples=[8],
                          mlps=[[2, 8, 8]], aggregation_mlp=None, confidence_mlp=None),
    "sampler_ryfps": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['ry-FPS'], radii=[1.6], nsamples=[8],
                          mlps=[[2, 8, 8]], aggregation_mlp=None, confidence_mlp=None),
    "sampler_rand": dict(npoint_list=[256], sample_range_list=[-1], sample_type_list=['Rand'], radii=[1.6], nsamples=[8],
                         mlps=[[2, 8, 8]], aggregation_mlp=None, confidence_mlp=None),
}


@pytest.mark.parametrize("name", sorted(SA_CASES))
def test_golden_sa_module(ext, G, dev, name, monkeypatch):
    """PointnetSAModuleMSG_WithSampling against the reference module's outputs on the same weights."""
    from spsnet_amd import pointnet2_modules as M
    g = np.load(os.path.join(GOLD, name + ".npz"))
    if name == "sampler_rand":
        # the reference drew its permutation from torch's CPU generator; hand the same one to the module (its prefix is the
        # fixture's index row) -- what is pinned is everything the branch does with it (pointnet2_modules.py:370-371)
        n = g["xyz"].shape[1]
        head = g["idx"][0].astype(np.int64)
        assert (g["idx"] == g["idx"][:1]).all()
        rest = np.setdiff1d(np.arange(n), head)
        perm = torch.from_numpy(np.concatenate([head, rest]))
        monkeypatch.setattr(torch, "randperm", lambda count, device=None, **kw: perm.to(device) if count == n else None)
    kw = dict(use_xyz=True, dilated_group=False, num_class=3)
    kw.update(SA_CASES[name])
    mod = _load_sd(M.PointnetSAModuleMSG_WithSampling(**kw), g).to(dev).eval()
    fkw = {"stds": G.t(g["kw_stds"])} if "kw_stds" in g.files else {}
    cls_in = G.t(g["cls_in"]) if "cls_in" in g.files else None
    with torch.no_grad():
        new_xyz, new_feat, cls, idx, stds = mod(G.t(g["xyz"]), G.t(g["feats"]), cls_in, **fkw)
    exact = True
    if name in ("sampler_ctr", "sampler_sss", "sampler_nogroup"):
        s = 1.0 / (1.0 + np.exp(-g["cls_in"].max(-1).astype(np.float64)))
        if name == "sampler_sss":
            s = s * (1.0 - 1.0 / (1.0 + np.exp(-(g["kw_stds"].astype(np.float64) / 8 - 3))))
        topk_equivalent(G.n(idx), g["idx"], s, 1e-6)
        exact = bool((G.n(idx) == g["idx"]).all())
    else:
        np.testing.assert_array_equal(G.n(idx), g["idx"])
    if exact:  # a swapped near-tie pair permutes rows; everything downstream is compared only when identical
        np.testing.assert_array_equal(G.n(new_xyz), g["new_xyz"])
        np.testing.assert_allclose(G.n(new_feat), g["new_features"], rtol=1e-4, atol=1e-4)
        if "cls" in g.files:
            np.testing.assert_allclose(G.n(cls), g["cls"], rtol=1e-4, atol=1e-4)
        if "stds_out" in g.files:
            np.testing.assert_array_equal(G.n(stds), g["stds_out"])
    assert idx.dtype == torch.int32 and new_xyz.shape[-1] == 3


def test_golden_stack3(ext, G, dev):
    from spsnet_amd import pointnet2_modules as M, sa_stack
    g = np.load(os.path.join(GOLD, "stack3_small.npz"))
    cfg = sa_stack.scaled_config(npoints=[512, 128, 64])
    cfg['mlps'] = [[[8, 8, 16], [8, 8, 16]], [[16, 16, 32], [16, 24, 32]], [[32, 32, 64], [32, 64, 64]]]
    cfg['aggregation_mlps'] = [[16], [32], [64]]
    cfg['confidence_mlps'] = [[], [32], [64]]
    layers = _load_sd(sa_stack.build_sa_layers(M, cfg, seed=11), g).to(dev).eval()
    with torch.no_grad():
        outs = sa_stack.run_sa_layers(layers, G.t(g["xyz"]), G.t(g["feats"]))
    for k in (0, 1):
        np.testing.assert_array_equal(G.n(outs[k][3]), g[f"l{k}_idx"])
        np.testing.assert_array_equal(G.n(outs[k][0]), g[f"l{k}_new_xyz"])
        np.testing.assert_allclose(G.n(outs[k][1]), g[f"l{k}_new_features"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(G.n(outs[1][2]), g["l1_cls"], rtol=1e-4, atol=1e-4)
    s = 1.0 / (1.0 + np.exp(-g["l1_cls"].max(-1).astype(np.float64)))
    topk_equivalent(G.n(outs[2][3]), g["l2_idx"], s, 1e-5)
    if (G.n(outs[2][3]) == g["l2_idx"]).all():
        np.testing.assert_allclose(G.n(outs[2][1]), g["l2_new_features"], rtol=1e-4, atol=1e-4)


def test_golden_generator_layer_and_fp_module(ext, G, dev):
    from spsnet_amd import pointnet2_modules as M
    g = np.load(os.path.join(GOLD, "generator_layer.npz"))
    mod = _load_sd(M.PointnetSampling(npoint_list=[512], sample_range_list=[-1], sample_type_list=['D-FPS'],
                                      radii=[0.2, 0.8], nsamples=[16, 32], mlps=[[1, 16, 16, 32], [1, 32, 32, 64]],
                                      use_xyz=True, dilated_group=False, aggregation_mlp=[64]), g).to(dev).eval()
    with torch.no_grad():
        nx, nf, idx = mod(G.t(g["xyz"]), G.t(g["feats"]))
    np.testing.assert_array_equal(G.n(idx), g["idx"])
    np.testing.assert_array_equal(G.n(nx), g["new_xyz"])
    np.testing.assert_allclose(G.n(nf), g["new_features"], rtol=1e-4, atol=1e-4)
    g = np.load(os.path.join(GOLD, "fp_module.npz"))
    fp = _load_sd(M.PointnetFPModule(mlp=[10, 16, 8]), g).to(dev).eval()
    with torch.no_grad():
        out = fp(G.t(g["unknown"]), G.t(g["known"]), G.t(g["uf"]), G.t(g["kf"]))
    np.testing.assert_allclose(G.n(out), g["out"], rtol=1e-4, atol=1e-4)


def test_training_step_backward_runs(ext, G, dev):
    """tools/train.py-style use: gradients flow through group/gather into the MLP weights and features."""
    from spsnet_amd import pointnet2_modules as M
    torch.manual_seed(0)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[128], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.5, 1.0], nsamples=[8, 16],
        mlps=[[4, 8, 16], [4, 8, 16]], use_xyz=True, dilated_group=False, aggregation_mlp=[16], confidence_mlp=[8],
        num_class=3).to(dev).train()
    xyz = torch.rand(2, 1000, 3, device=dev) * 4
    feats = torch.randn(2, 4, 1000, device=dev, requires_grad=True)
    new_xyz, nf, cls, idx, _ = mod(xyz, feats)
    (nf.square().mean() + cls.square().mean()).backward()
    assert feats.grad is not None and torch.isfinite(feats.grad).all() and feats.grad.abs().sum() > 0
    assert all(p.grad is not None for p in mod.parameters())


# ------------------------------------------------------------------ fused MFMA grouped MLP
FUSED_CASES = [  # (c_feat, mlp widths, nsample, radius)
    (1, [16, 16, 32], 16, 0.4), (1, [32, 32, 64], 32, 0.9), (64, [64, 64, 128], 16, 0.8), (64, [64, 96, 128], 32, 1.6),
    (128, [128, 128, 256], 16, 1.6), (128, [128, 256, 256], 32, 3.0), (124, [124, 64, 128], 16, 0.8),
    (5, [16, 16, 20], 32, 1.0), (0, [32, 32, 64], 16, 0.7),
    # nsample 64 (BASELINE config 5): a centroid's samples span two kernel units (four waves in the shared-stream kernel)
    (1, [16, 16, 32], 64, 0.9), (64, [64, 96, 128], 64, 1.6), (128, [128, 256, 256], 64, 3.0), (128, [128, 128, 256], 64, 2.0),
    # IA-SSD layer 5 (vote centres): 512- and 1024-wide outputs, shared-stream kernel only
    (256, [256, 256, 512], 16, 2.4), (256, [256, 512, 1024], 32, 3.2),
]


@BOTH_PRECISIONS
@pytest.mark.parametrize("c_feat,widths,ns,radius", FUSED_CASES)
def test_fused_group_mlp_matches_unfused(ext, G, dev, c_feat, widths, ns, radius, mlp_precision):
    """sps_sa_group_mlp (gather + 3 MFMA layers with folded BN + max-pool) against the unfused
    Conv2d/BatchNorm2d/ReLU/max_pool2d path on the same weights (tolerance of BASELINE.json: 1e-4)."""
    from spsnet_amd import pointnet2_modules as M
    torch.manual_seed(c_feat * 100 + ns)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[radius], nsamples=[ns],
        mlps=[[c_feat] + list(widths)], use_xyz=True, dilated_group=False, aggregation_mlp=None, confidence_mlp=None,
        num_class=3).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    for m_ in mod.modules():
        if isinstance(m_, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m_.running_mean.copy_(torch.randn(m_.num_features, generator=gen) * 0.2)
                m_.running_var.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.weight.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.bias.copy_(torch.randn(m_.num_features, generator=gen) * 0.2)
    rng = np.random.default_rng(ns + c_feat)
    xyz = G.t(cloud(rng, 2, 3000, dup=0.02))
    feats = G.t(rng.normal(size=(2, c_feat, 3000)).astype(np.float32)) if c_feat else None   # c_feat 0: grouped xyz only
    with torch.no_grad():
        assert mod._fused_plan(xyz, xyz[:, :256].contiguous(), feats) is not None, "fused path not taken"
        new_xyz, fused, _, idx, _ = mod(xyz, feats)
        from spsnet_amd import fused as fused_mod
        plan, generic = mod._fused_plan, fused_mod.generic_mlp_pool
        mod._fused_plan = lambda *a, **k: None  # force the unfused path ...
        fused_mod.generic_mlp_pool = lambda *a, **k: None   # ... all the way down to the torch modules
        try:
            _, unfused, _, idx2, _ = mod(xyz, feats)
        finally:
            mod._fused_plan, fused_mod.generic_mlp_pool = plan, generic
    assert torch.equal(idx, idx2)
    scale = max(1.0, float(unfused.abs().max()))
    assert float((fused - unfused).abs().max()) <= 1e-4 * scale
    assert fused.shape == unfused.shape


@BOTH_PRECISIONS
def test_fused_full_width_stack_against_cpu_oracle(ext, G, dev, mlp_precision):
    """IA-SSD L0-L2 at full channel widths (fused MFMA path) against the CPU oracle stack, in the library's default strict
    fp32 and in the opt-in split-fp16 arithmetic."""
    from oracle import cpu_stack
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    cfg = sa_stack.scaled_config(npoints=[1024, 256, 128])
    layers = sa_stack.build_sa_layers(M, cfg, seed=5)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 4096, seed0=77, dup_fraction=0.01)
    want = cpu_stack.sa_stack_cpu(cpu_stack.cpu_copy(layers), xyz, feats)
    layers = layers.to(dev)
    with torch.no_grad():
        got = sa_stack.run_sa_layers(layers, G.t(xyz), G.t(feats))
    for k in (0, 1):
        np.testing.assert_array_equal(G.n(got[k][3]), want[k][3])
        np.testing.assert_array_equal(G.n(got[k][0]), want[k][0])
        ref = want[k][1]
        assert float(np.abs(G.n(got[k][1]) - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(G.n(got[1][2]), want[1][2], rtol=1e-4, atol=1e-4)


def _check_stack_against_cpu_oracle(G, dev, layers, want, got, score_layer_inputs):
    """Bars of the full-size stack tests: D-FPS layers' indices and centroids bit-exact, features / class scores 1e-4; the
    score-sampled last layer matched by sampled index on the shared picks, then alone on the ORACLE's previous-layer outputs
    (identical inputs on both sides): indices bit-exact, every row within 1e-4."""
    from spsnet_amd import fused
    from tests.gpu_util import compare_matched_rows
    for k in (0, 1):   # D-FPS layers: indices and centroids exact
        np.testing.assert_array_equal(G.n(got[k][3]), want[k][3])
        np.testing.assert_array_equal(G.n(got[k][0]), want[k][0])
    achieved = {}
    for k in (0, 1):
        ref = want[k][1]
        achieved[f"layer{k}_max_abs_err"] = float(np.abs(G.n(got[k][1]) - ref).max())
        achieved[f"layer{k}_feature_scale"] = float(np.abs(ref).max())
        assert achieved[f"layer{k}_max_abs_err"] <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    achieved["layer1_cls_max_abs_err"] = float(np.abs(G.n(got[1][2]) - want[1][2]).max())
    np.testing.assert_allclose(G.n(got[1][2]), want[1][2], rtol=1e-4, atol=1e-4)
    # layer 2 samples by score: same set up to near-ties of the scores (which carry the 1e-4 feature tolerance); rows are
    # matched by sampled index and compared on the intersection
    overlap = compare_matched_rows(G.n(got[2][3]), want[2][3], [(G.n(got[2][0]), want[2][0], 0.0, 1),
                                                               (G.n(got[2][1]), want[2][1], 1e-4, 2),
                                                               (G.n(got[2][2]), want[2][2], 1e-4, 1)])
    assert overlap >= 0.99
    # ... and layer 2 alone at full size on the ORACLE's layer-1 outputs (identical inputs on both sides): indices
    # bit-exact, every feature / class-score row within 1e-4 -- the 128-wide kernels at M = 512, N = 1024
    x1, f1, c1 = G.t(want[1][0]), fused.attach_point_major_twin(G.t(want[1][1])), G.t(want[1][2])
    with torch.no_grad():
        nx, nf, nc, ni, _ = layers[2](x1, f1, c1, **score_layer_inputs)
    np.testing.assert_array_equal(G.n(ni), want[2][3])
    np.testing.assert_array_equal(G.n(nx), want[2][0])
    ref = want[2][1]
    achieved["layer2_on_oracle_inputs_max_abs_err"] = float(np.abs(G.n(nf) - ref).max())
    achieved["layer2_feature_scale"] = float(np.abs(ref).max())
    achieved["layer2_picks_shared_in_stack"] = overlap
    assert float(np.abs(G.n(nf) - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(G.n(nc), want[2][2], rtol=1e-4, atol=1e-4)
    assert not fused.check_overflow()
    _log_achieved_error(dict(achieved, precision=fused.PRECISION, scenes=int(want[0][3].shape[0]),
                             centroids_layer0=int(got[0][3].shape[1]), test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]))


def _log_achieved_error(rec):
    """The absolute error the full-size comparisons ACHIEVED (the bar is 1e-4 x max(1, max |ref|)): appended, one JSON line
    per test, to gpurun_out/parity_achieved_error.jsonl when that scratch directory exists (copied to profiles/roundN/)."""
    import json
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_achieved_error.jsonl"), "a") as fh:
            fh.write(json.dumps(rec) + "\n")


@pytest.mark.parametrize("scenes_n,dataset", [(2, "kitti-lidar-v1"), (8, "kitti-lidar-v1"), (2, "uniform-v1")])
@BOTH_PRECISIONS
def test_full_size_stack_against_cpu_oracle(ext, G, dev, mlp_precision, scenes_n, dataset):
    """BASELINE config 2 at full size (16 384 points, IA-SSD widths; 2 scenes and the bench's 8; KITTI-shaped and SURVEY 8d's
    uniform-v1, the ball query's worst case) against the CPU oracle stack, in the headline
    arithmetic (strict fp32: packed columns, layer 1 started on the early picks and merged by atomic max, the per-point
    layer-1 form at layer 2) and in the opt-in split-fp16 one (LDS-resident / shared-stream kernels): this is the shape at
    which the streamed first layer, the multi-pick FPS rounds, the point-major gathers and the fused tails are all active."""
    from oracle import cpu_stack
    from spsnet_amd import fused, pointnet2_modules as M, sa_stack, scenes
    layers = sa_stack.build_sa_layers(M, sa_stack.IASSD_KITTI, seed=9)
    xyz, feats = scenes.make_batch(dataset, scenes_n, 16384, seed0=123, dup_fraction=0.005)
    want = cpu_stack.sa_stack_cpu(cpu_stack.cpu_copy(layers), xyz, feats)
    layers = layers.to(dev)
    with torch.no_grad():
        got = sa_stack.run_sa_layers(layers, G.t(xyz), G.t(feats))
    assert not sa_stack.check_timeouts() and not fused.check_overflow()
    _check_stack_against_cpu_oracle(G, dev, layers, want, got, {})


@BOTH_PRECISIONS
def test_full_size_stability_stack_against_cpu_oracle(ext, G, dev, mlp_precision):
    """BASELINE configs[3] at full size (2 x 16 384): SPSNet's stability-score top-k ('sss_aware': sigmoid(max logits) *
    (1 - sigmoid(stds / 8 - 3)), pointnet2_modules.py:293-305) replacing the ctr-aware sampler of the last layer, the
    per-point `stds` thinned through the D-FPS layers in front of it -- against the CPU oracle stack, same bars."""
    from oracle import cpu_stack
    from spsnet_amd import fused, pointnet2_modules as M, sa_stack, scenes
    cfg = sa_stack.scaled_config(sample_methods=['D-FPS', 'D-FPS', 'sss_aware'])
    layers = sa_stack.build_sa_layers(M, cfg, seed=11)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 16384, seed0=321, dup_fraction=0.005)
    stds = np.random.default_rng(17).uniform(0.0, 48.0, (2, 16384)).astype(np.float32)
    want = cpu_stack.sa_stack_cpu(cpu_stack.cpu_copy(layers), xyz, feats, stds=stds)
    layers = layers.to(dev)
    with torch.no_grad():
        got = sa_stack.run_sa_layers(layers, G.t(xyz), G.t(feats), stds=G.t(stds))
    assert not sa_stack.check_timeouts() and not fused.check_overflow()
    # the stds the last layer's sampler sees on the oracle's side: thinned by the two D-FPS layers
    s1 = np.take_along_axis(np.take_along_axis(stds, want[0][3].astype(np.int64), 1), want[1][3].astype(np.int64), 1)
    _check_stack_against_cpu_oracle(G, dev, layers, want, got, dict(stds=G.t(np.ascontiguousarray(s1))))


# ------------------------------------------------------------------ pruned vs brute-force FPS kernels
@pytest.mark.parametrize("N,m,kind", [(6144, 512, "lattice"), (8192, 1024, "dup"), (7000, 700, "dup"), (16384, 4096, "kitti"),
                                      (16384, 600, "lattice"), (20480, 300, "dup"), (12345, 999, "uniform")])
def test_fps_pruned_equals_bruteforce_and_oracle(ext, G, oracle, N, m, kind):
    """Both FPS kernel families (spatially pruned / brute-force register-resident) against the oracle,
    indices AND final running distances bit-exact."""
    from spsnet_amd import _lib, scenes
    rng = np.random.default_rng(N + m)
    if kind == "lattice":
        xyz = cloud(rng, 2, N, lattice=True)
    elif kind == "kitti":
        xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, N, seed0=11, dup_fraction=0.02)
    elif kind == "uniform":
        xyz, _ = scenes.make_batch("uniform-v1", 2, N, seed0=12)
    else:
        xyz = cloud(rng, 2, N, dup=0.2)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    L = _lib.load()
    for mode in (0, 1):
        old = L.sps_set_fps_mode(mode)
        try:
            got, got_t = G.fps(ext, xyz, m)
        finally:
            L.sps_set_fps_mode(old)
        np.testing.assert_array_equal(got, want, err_msg=f"fps mode {mode}")
        np.testing.assert_array_equal(got_t, want_t, err_msg=f"fps mode {mode}")


def _adversarial_cloud(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "mirror4":      # 4-fold mirror symmetry about the first point: exact distance ties in different buckets
        q = rng.uniform(0.05, 30.0, size=(N // 4, 3)).astype(np.float32)
        q[:, 2] = rng.uniform(-1, 1, size=N // 4).astype(np.float32)
        xyz = np.concatenate([q * np.array(sg, np.float32) for sg in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))])
        xyz = xyz[rng.permutation(len(xyz))]
        xyz[0] = 0.0
    elif kind == "clusters":   # tight far-apart clumps: the hidden points of a wave are nearly as far as its best one
        c = rng.uniform(-40, 40, size=(24, 3)).astype(np.float32)
        xyz = (c[rng.integers(0, 24, N)] + rng.normal(0, 0.05, size=(N, 3))).astype(np.float32)
    elif kind == "stacked":    # 200 distinct locations, every point a duplicate: running distances tie exactly, many zeros
        c = rng.uniform(-20, 20, size=(200, 3)).astype(np.float32)
        xyz = c[rng.integers(0, 200, N)]
    elif kind == "sheet":      # integer grid on a plane: everything ties
        g = rng.integers(0, 96, size=(N, 2)).astype(np.float32)
        xyz = np.concatenate([g, np.zeros((N, 1), np.float32)], 1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(xyz[None].astype(np.float32))


@pytest.mark.parametrize("kind,N,m", [("mirror4", 16384, 4096), ("clusters", 16384, 2048), ("stacked", 8192, 1024),
                                      ("sheet", 12288, 3000), ("mirror4", 6144, 6144), ("clusters", 9000, 4500)])
def test_fps_multi_pick_rounds_adversarial(ext, G, oracle, kind, N, m):
    """The pruned kernel accepts several picks per round when it can prove sequential FPS would make them in that
    order.  Clouds built to stress that proof: exact ties across buckets, near-equal hidden points, duplicates."""
    xyz = np.concatenate([_adversarial_cloud(kind, N, s) for s in (1, 2)])
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    got, got_t = G.fps(ext, xyz, m)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)


def test_fps_pruned_degenerate_clouds(ext, G, oracle):
    """All points identical / collinear / containing NaN and Inf: the cell grid degenerates, results must not."""
    N, m = 8192, 300
    same = np.ones((1, N, 3), np.float32) * 2.5
    line = np.zeros((1, N, 3), np.float32)
    line[0, :, 0] = np.random.default_rng(0).permutation(N).astype(np.float32) * 0.01
    bad = cloud(np.random.default_rng(1), 1, N)
    bad[0, 17] = np.nan
    bad[0, 900, 2] = np.inf
    bad[0, 901, 0] = -np.inf
    for xyz in (same, line, bad):
        want, want_t = oracle.fps(xyz, m, return_temp=True)
        got, got_t = G.fps(ext, xyz, m)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("cluster", ["1", "8,4", "3,5"])
def test_fps_large_scene_degenerate_clouds(ext, G, oracle, cluster, monkeypatch):
    """The same degenerate inputs through the large-scene kernels (one workgroup, and spread over K workgroups: the split
    sort takes its box from a strided sample, which here is all-equal, collinear or holds NaN / Inf)."""
    monkeypatch.setenv("SPS_FPS_CLUSTER", cluster)
    N, m = 20000, 260
    same = np.ones((1, N, 3), np.float32) * 2.5
    line = np.zeros((1, N, 3), np.float32)
    line[0, :, 0] = np.random.default_rng(0).permutation(N).astype(np.float32) * 0.01
    bad = cloud(np.random.default_rng(1), 1, N)
    bad[0, 16] = np.nan            # (index 16 is in every K-strided sample)
    bad[0, 17] = np.nan
    bad[0, 960, 2] = np.inf
    bad[0, 1920, 0] = -np.inf
    for xyz in (same, line, bad):
        want, want_t = oracle.fps(xyz, m, return_temp=True)
        got, got_t = G.fps(ext, xyz, m)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("path", ["fused", "op_by_op", "fused_train"])
@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_golden_surface_feature(ext, G, dev, mode, path, monkeypatch):
    """FeatureExtraction / DenseEdgeConv (surface_feature.py:45-187) against the reference's output, including
    the dynamic-graph quirk where a d-channel feature tensor is read as packed xyz triples.  `fused` = the inference
    kernels (sps_linear_rows + sps_dense_edge_conv), `op_by_op` = the differentiable form (gradients enabled)."""
    from spsnet_amd import surface_feature as SF
    g = np.load(os.path.join(GOLD, "surface_feature.npz"))
    net = SF.FeatureExtraction(dynamic_graph=(mode == "dynamic"))
    pre = f"sd_{mode}."
    net.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}, strict=True)
    net = net.to(dev).eval()
    x = G.t(g["xyz"])
    if path == "fused":
        with torch.no_grad():
            assert all(c._fused(torch.empty(1, 1, 24, device=dev), x) for c in net.convs)
            out = net(x)
    elif path == "op_by_op":
        monkeypatch.setattr(SF, "FUSED_TRAINING", False)
        out = net(x)
        assert out.requires_grad
    else:   # fused_train: gradients wanted, fused forward + backward kernels
        out = net(x)
        assert out.requires_grad and type(out.grad_fn).__name__ == "DenseEdgeConvTrainBackward"
    ref = g["out_" + mode]
    assert out.shape == ref.shape
    assert float(np.abs(G.n(out.detach()) - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_surface_feature_fused_matches_op_by_op(ext, G, dev, mode, monkeypatch):
    """The fused DenseEdgeConv kernels against the op-by-op form on LiDAR-like scenes (B=2, N=8192: many full and many
    empty balls), random weights; 1e-4 relative to the largest feature."""
    from spsnet_amd import scenes, surface_feature as SF
    torch.manual_seed(5)
    net = SF.FeatureExtraction(dynamic_graph=(mode == "dynamic")).to(dev).eval()
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=77)
    x = G.t(xyz)
    with torch.no_grad():
        fused_out = net(x)
    monkeypatch.setattr(SF, "FUSED_TRAINING", False)
    plain = net(x)
    assert plain.requires_grad and not fused_out.requires_grad
    a, b = G.n(fused_out), G.n(plain.detach())
    assert a.shape == (2, 8192, 60)
    assert float(np.abs(a - b).max()) <= 1e-4 * max(1.0, float(np.abs(b).max()))


# ------------------------------------------------------------------ FPS of an FPS-ordered cloud (verified shortcut)
def test_fps_ordered_prefix_shortcut(ext, G, oracle):
    """D-FPS on the pick sequence of a previous D-FPS: confirmed scenes take the parallel check, everything is
    bit-identical to the plain kernel and the oracle (indices and final running distances)."""
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 4, 8192, seed0=21)
    i0 = oracle.fps(xyz, 2048)
    x1 = gather_xyz(xyz, i0)                      # FPS-ordered cloud (B, 2048, 3)
    x1[3] = x1[3][np.random.default_rng(0).permutation(2048)]   # scene 3: order destroyed -> must be recomputed
    want, want_t = oracle.fps(x1, 512, return_temp=True)
    idx, flags, temp = ext.fps_ordered_prefix(G.t(x1), 512, return_flags=True)
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)
    f = G.n(flags)
    assert f[:3].tolist() == [0, 0, 0] and f[3] == 1            # shortcut taken where it applies, refused where not
    assert (want[:3] == np.arange(512, dtype=np.int32)[None]).all()
    np.testing.assert_array_equal(G.fps(ext, x1, 512)[0], want)


def test_fps_ordered_prefix_many_centres(ext, G, oracle):
    """Config-5 sized prefix: 16 384 FPS-ordered points -> 4 096 (the centres are staged in dynamic LDS, up to 7 168 of
    them; more fall through to the ordinary kernel), confirmed and destroyed scenes, against the oracle."""
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, 40000, seed0=77)
    x1 = gather_xyz(xyz, oracle.fps(xyz, 16384))
    x1[1] = x1[1][np.random.default_rng(1).permutation(16384)]
    for m in (4096, 7168, 7169):
        want, want_t = oracle.fps(x1, m, return_temp=True)
        idx, flags, temp = ext.fps_ordered_prefix(G.t(x1), m, return_flags=True)
        np.testing.assert_array_equal(G.n(idx), want)
        np.testing.assert_array_equal(G.n(temp), want_t)
        if m <= 7168:
            assert G.n(flags).tolist() == [0, 1]


@pytest.mark.parametrize("N,m", [(600, 300), (4096, 1024), (4096, 4096), (5000, 100)])
def test_fps_ordered_prefix_with_ties(ext, G, oracle, N, m):
    """Lattice clouds: equal distances everywhere, the two runs' tie rules differ, so the guess often fails --
    the result must still equal the reference algorithm on that input."""
    rng = np.random.default_rng(N)
    base = cloud(rng, 2, 4 * N, lattice=True)
    x1 = gather_xyz(base, oracle.fps(base, N))
    want, want_t = oracle.fps(x1, m, return_temp=True)
    idx, flags, temp = ext.fps_ordered_prefix(G.t(x1), m, return_flags=True)
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)


@pytest.mark.parametrize("kind,N,m,cuts", [("lidar", 4096, 1024, (1024, 2048, 3584, 3840)), ("lidar", 2048, 512, (1000, 1990)),
                                           ("lattice", 4096, 1024, (2048, 3840)), ("lidar", 4096, 1024, ())])
def test_fps_ordered_prefix_second_pass_in_pieces(ext, G, oracle, kind, N, m, cuts):
    """OrderedPrefix as the streamed first layer drives it: begin(), then the second pass for the points that exist so far
    (check_upto after every chunk, cut points rounded down to 64), then finish() for the rest -- the same indices, final
    running distances and flags as the one-call form and the oracle; a destroyed scene and a lattice cloud (exact ties)
    are recomputed; force_redo recomputes everything."""
    from spsnet_amd import scenes
    if kind == "lattice":
        base = cloud(np.random.default_rng(N), 3, 4 * N, lattice=True)
    else:
        base, _ = scenes.make_batch("kitti-lidar-v1", 3, 4 * N, seed0=N + m)
    x1 = gather_xyz(base, oracle.fps(base, N))
    x1[2] = x1[2][np.random.default_rng(0).permutation(N)]
    want, want_t = oracle.fps(x1, m, return_temp=True)
    ref_idx, ref_flags, ref_temp = ext.fps_ordered_prefix(G.t(x1), m, return_flags=True)
    np.testing.assert_array_equal(G.n(ref_idx), want)
    for force in (None, 0, 1):
        op = ext.OrderedPrefix(G.t(x1), m)
        op.check_upto(cuts[0] if cuts else 64)          # before begin(): ignored
        assert op.checked == 0
        op.begin()
        for c in cuts:
            op.check_upto(c)
            assert op.checked == (min(c, N) & ~63)
        flag = None if force is None else torch.full((1,), force, dtype=torch.int32, device=op.flags.device)
        idx = op.finish(force_redo=flag)
        np.testing.assert_array_equal(G.n(idx), want)
        np.testing.assert_array_equal(G.n(op.temp), want_t)
        if force == 1:
            assert G.n(op.flags).tolist() == [1, 1, 1]
        else:
            np.testing.assert_array_equal(G.n(op.flags), G.n(ref_flags))
            assert G.n(op.flags)[2] == 1
            if kind == "lidar":
                assert G.n(op.flags)[:2].tolist() == [0, 0]


@pytest.mark.parametrize("N,M,ra,nsa,rb,nsb", [(16384, 4096, 0.2, 16, 0.8, 32), (4096, 1000, 0.8, 16, 1.6, 32),
                                                (1024, 512, 1.6, 16, 4.8, 32), (333, 70, 0.5, 4, 0.3, 64)])
def test_ball_query_dual_radius(ext, G, oracle, N, M, ra, nsa, rb, nsb):
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, N, seed0=N)
    rng = np.random.default_rng(M)
    new_xyz = xyz[:, rng.integers(0, N, M)].copy()
    new_xyz[:, -1] = 500.0
    for grouped, wave in ((True, False), (False, False), (False, True)):
        ia, ib = ext.ball_query_full2(ra, nsa, rb, nsb, G.t(xyz), G.t(new_xyz), spatial_groups=grouped,
                                      wave_per_centroid=wave)
        np.testing.assert_array_equal(G.n(ia), oracle.ball_query(ra, nsa, xyz, new_xyz))
        np.testing.assert_array_equal(G.n(ib), oracle.ball_query(rb, nsb, xyz, new_xyz))


def test_fenced_passes_in_flight_equal_sequential(ext, G, dev):
    """Two passes in flight on streams whose FPS producers are fenced onto compute units of their own (sa_stack.CuFence /
    pipelined_bench, hipExtStreamCreateWithCUMask): every output of the last pass bit-identical to a sequential,
    unstreamed pass; no wait timed out.  (The producers' sorting pre-pass must stay off the masked streams.)"""
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    layers = sa_stack.build_sa_layers(M, sa_stack.IASSD_KITTI, seed=4).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 4, 16384, seed0=51)
    x, f = G.t(xyz), G.t(feats)
    with torch.no_grad():
        want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
        res = sa_stack.pipelined_bench(lambda: sa_stack.run_sa_layers(layers, x, f), 6, torch.device(dev), in_flight=2, scenes=4)
    torch.cuda.synchronize()
    assert not sa_stack.check_timeouts()
    for a, b in zip(res["last_outputs"], want):
        for u, v in zip(a[:4], b[:4]):
            if u is not None:
                assert torch.equal(u, v)


@pytest.mark.parametrize("with_stds", [False, True])
def test_streamed_first_layer_equals_sequential(ext, G, dev, with_stds):
    """Layer 0 with its grouping/MLP consuming the FPS output while FPS runs (progress hand-off) against the plain
    sequential schedule: every output of every layer bit-identical, no wait timed out.  with_stds = BASELINE config 4
    (stability-score sampler at layer 2, stds thinned by every sampler on the way)."""
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    cfg = sa_stack.scaled_config(sample_methods=['D-FPS', 'D-FPS', 'sss_aware']) if with_stds else sa_stack.IASSD_KITTI
    layers = sa_stack.build_sa_layers(M, cfg, seed=2).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 4, 16384, seed0=31, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)
    sd = G.t(np.random.default_rng(5).uniform(0, 40, (4, 16384)).astype(np.float32)) if with_stds else None
    _run = sa_stack.run_sa_layers
    sa_stack_run = lambda *a, **k: _run(*a, stds=sd, **k)
    with torch.no_grad():
        b = sa_stack_run(layers, x, f, overlap=False)
        for rep in range(3):
            # poison the caching allocator's free blocks with in-bounds but wrong values: a consumer that ran ahead
            # of the producer (or read a stale cache line) would then compute visibly wrong results, not fault
            junk_i = torch.full((32 << 20,), 1 + rep, dtype=torch.int32, device=dev)
            junk_f = torch.full((32 << 20,), 0.5 + rep, dtype=torch.float32, device=dev)
            del junk_i, junk_f
            a = sa_stack_run(layers, x, f, stream_first_layer=True)
            torch.cuda.synchronize()
            assert not sa_stack.check_timeouts()
            for la, lb in zip(a, b):
                for ta, tb in zip(la, lb):
                    assert (ta is None and tb is None) or torch.equal(ta, tb), f"repetition {rep}"
    torch.cuda.synchronize()
    assert not sa_stack.check_timeouts()
    for la, lb in zip(a, b):
        for ta, tb in zip(la, lb):
            if ta is None:
                assert tb is None
            else:
                assert torch.equal(ta, tb)


@pytest.mark.parametrize("B,N,npts,ns", [(2, 40000, [4096, 1024, 256], None), (3, 70000, [8192, 2048, 512], [(64, 64)] * 3),
                                         (10, 20000, [2048, 512, 128], None)])
def test_streamed_large_scenes_equal_sequential(ext, G, dev, B, N, npts, ns):
    """Scenes beyond 16 384 points: layer 0 streamed behind the PUBLISHING clustered FPS (fps_pruned_cluster.hip, K = 8 / 4
    workgroups per scene by batch size; nsample 16 & 32 with the self-repairing last chunk, nsample 64 with the predicated
    re-issue) and the next layer's D-FPS as a verified identity prefix of up to 7168 centres -- against the sequential,
    unstreamed schedule: every output of every layer bit-identical, twice, allocator poisoned, no wait timed out."""
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    layers = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=npts, nsamples=ns), seed=9).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", B, N, seed0=41, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)
    with torch.no_grad():
        want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
        for rep in range(2):
            junk_i = torch.full((32 << 20,), 1 + rep, dtype=torch.int32, device=dev)
            junk_f = torch.full((32 << 20,), 0.5 + rep, dtype=torch.float32, device=dev)
            del junk_i, junk_f
            got = sa_stack.run_sa_layers(layers, x, f, stream_first_layer=True)
            torch.cuda.synchronize()
            assert not sa_stack.check_timeouts()
            for la, lb in zip(got, want):
                for ta, tb in zip(la, lb):
                    assert (ta is None and tb is None) or torch.equal(ta, tb), f"repetition {rep}"


@pytest.mark.parametrize("npts,ns,half", [(None, None, False), ([2048, 512, 128], [(64, 64)] * 3, False),
                                          ([2048, 512, 128], [(64, 64)] * 3, True)])
def test_streamed_first_layer_first_call_of_fresh_modules(G, dev, npts, ns, half):
    """The FIRST pass through freshly built modules takes the streamed schedule too: weight folding / packing happens
    inside that pass and must reach the consumer stream in time (it used to be enqueued behind the FPS kernel: all chunks
    but the last read unpacked weights).  Compared bit for bit with a sequential pass through a deep copy, allocator
    poisoned; nsample 16 & 32 at 16 384 points, nsample 64 (atomic-max units) with fp32 and with fp16 features."""
    import copy
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    N = 16384 if npts is None else 8192
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, N, seed0=31)
    x, f = G.t(xyz), G.t(feats.astype(np.float16) if half else feats)
    for trial in range(2):
        layers = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=npts, nsamples=ns), seed=2 + trial).to(dev)
        twin = copy.deepcopy(layers)
        junk_i = torch.full((32 << 20,), 3 + trial, dtype=torch.int32, device=dev)
        junk_f = torch.full((32 << 20,), 7.5 + trial, dtype=torch.float32, device=dev)
        del junk_i, junk_f
        torch.cuda.synchronize()
        with torch.no_grad():
            a = sa_stack.run_sa_layers(layers, x, f)
            torch.cuda.synchronize()
            b = sa_stack.run_sa_layers(twin, x, f, overlap=False, stream_first_layer=False)
        assert not sa_stack.check_timeouts()
        for k, (la, lb) in enumerate(zip(a, b)):
            for ta, tb in zip(la, lb):
                assert (ta is None and tb is None) or torch.equal(ta, tb), f"trial {trial}, layer {k}"


@pytest.mark.parametrize("c_feat,widths,ns,radius", FUSED_CASES[:7])
def test_fused_group_mlp_split_fp16(ext, G, dev, c_feat, widths, ns, radius):
    """The split-fp16 (hi+lo, 3 MFMAs) variant of the fused kernel against the unfused fp32 torch path: the 1e-4
    bar of BASELINE.json with a wide margin, and close to the fp32 MFMA kernel."""
    from spsnet_amd import fused, pointnet2_modules as M
    torch.manual_seed(c_feat * 100 + ns)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[radius], nsamples=[ns],
        mlps=[[c_feat] + list(widths)], use_xyz=True, dilated_group=False, aggregation_mlp=None, confidence_mlp=None,
        num_class=3).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    for m_ in mod.modules():
        if isinstance(m_, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m_.running_mean.copy_(torch.randn(m_.num_features, generator=gen) * 0.2)
                m_.running_var.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.weight.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.bias.copy_(torch.randn(m_.num_features, generator=gen) * 0.2)
    rng = np.random.default_rng(ns + c_feat)
    xyz = G.t(cloud(rng, 2, 3000, dup=0.02))
    feats = G.t((rng.normal(size=(2, c_feat, 3000)) * 3).astype(np.float32))
    with torch.no_grad():
        old32 = fused.set_precision("fp32")
        try:
            _, f32_out, _, _, _ = mod(xyz, feats)
        finally:
            fused.set_precision(old32)
        old = fused.set_precision("fp16x2")
        try:
            _, h_out, _, _, _ = mod(xyz, feats)
        finally:
            fused.set_precision(old)
        plan = mod._fused_plan
        mod._fused_plan = lambda *a, **k: None
        try:
            _, ref, _, _, _ = mod(xyz, feats)
        finally:
            mod._fused_plan = plan
    scale = max(1.0, float(ref.abs().max()))
    assert float((h_out - ref).abs().max()) <= 2e-5 * scale
    assert float((h_out - f32_out).abs().max()) <= 2e-5 * scale
    assert not fused.check_overflow()


def test_split_fp16_never_clamps_silently(ext, G, dev):
    """An operand beyond the exactly splittable range POISONS the centroids it reaches -- NaN rows, not clamped values --
    and is reported; centroids it does not reach equal the fp32 kernel's rows to the usual tolerance."""
    from spsnet_amd import fused, pointnet2_modules as M
    torch.manual_seed(0)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[1.0], nsamples=[32],
        mlps=[[5, 32, 32, 64]], use_xyz=True, dilated_group=False, aggregation_mlp=None, confidence_mlp=None,
        num_class=3).to(dev).eval()
    rng = np.random.default_rng(0)
    xyz = G.t(cloud(rng, 2, 2000))
    feats = G.t(rng.normal(size=(2, 5, 2000)).astype(np.float32))
    feats[0, 2, 100:140] = 3.0e5                       # forty out-of-range points in scene 0; scene 1 stays clean
    old = fused.set_precision("fp32")
    try:
        with torch.no_grad():
            _, ref, _, _, _ = mod(xyz, feats)
            fused.set_precision("fp16x2")
            fused.check_overflow()
            _, out, _, _, _ = mod(xyz, feats)
        assert fused.check_overflow()
        assert not fused.check_overflow()  # the flag resets
        bad = torch.isnan(out).any(dim=1)                # (B, M): poisoned centroids
        assert bad[0].any() and not bad[1].any() and torch.isfinite(ref).all()
        assert torch.isnan(out[0][:, bad[0]]).all()      # a poisoned centroid is NaN in every channel
        clean = ~bad
        scale = float(ref.abs().max())
        assert float((out.transpose(1, 2)[clean] - ref.transpose(1, 2)[clean]).abs().max()) <= 1e-4 * scale
    finally:
        fused.check_overflow()
        fused.set_precision(old)


@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
def test_nan_inputs_propagate_through_the_layer(ext, G, dev, precision):
    """torch's Conv / ReLU / max_pool2d / Conv1d chain propagates a NaN feature to every centroid whose ball holds the point;
    so does the fused path (integer-domain ReLU / pooling in the fp32 kernels, poisoned units in the split-fp16 ones), through
    the aggregation stack as well -- and nowhere else."""
    from spsnet_amd import fused, pointnet2_modules as M, pointnet2_utils as U
    torch.manual_seed(1)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.8, 1.6], nsamples=[16, 32],
        mlps=[[64, 64, 64, 128], [64, 64, 96, 128]], use_xyz=True, dilated_group=False, aggregation_mlp=[128], confidence_mlp=[],
        num_class=3).to(dev).eval()
    rng = np.random.default_rng(3)
    xyz = G.t(cloud(rng, 2, 2048))
    feats = G.t(rng.normal(size=(2, 64, 2048)).astype(np.float32))
    feats[1, 7, 300] = float("nan")
    old = fused.set_precision(precision)
    try:
        with torch.no_grad():
            fused.check_overflow()
            new_xyz, out, _, idx, _ = mod(xyz, feats)
            # which centroids hold point 300 of scene 1 in either ball?
            reach = torch.zeros(out.shape[0], out.shape[2], dtype=torch.bool, device=dev)
            for g in mod.groupers:
                rows = U.ball_query(g.radius, g.nsample, xyz, new_xyz)
                reach[1] |= (rows[1] == 300).any(dim=1)
        got = torch.isnan(out).any(dim=1)
        assert reach[1].any() and not (reach & ~got).any()      # every centroid the NaN reaches is NaN ...
        if precision == "fp32":
            assert torch.equal(got, reach)                       # ... and, in the exact kernels, no other
        else:                                                    # split-fp16 poisons whole kernel units: with 16 samples a
            partner = torch.zeros_like(reach)                    # unit of 32 columns holds centroids 2k and 2k + 1
            partner[:, 0::2], partner[:, 1::2] = reach[:, 1::2], reach[:, 0::2]
            assert not (got & ~(reach | partner)).any() and not got[0].any()
    finally:
        fused.check_overflow()
        fused.set_precision(old)


# ------------------------------------------------------------------ aggregation + confidence stacks as one kernel
@pytest.mark.parametrize("cin,cagg,conf,M", [(96, 64, None, 4096), (256, 128, 128, 1024), (512, 256, 256, 512),
                                             (48, 32, 48, 64), (1536, 512, None, 256)])
def test_pointwise_tail_matches_torch(ext, G, dev, cin, cagg, conf, M):
    """csrc/pw_mlp.hip (BatchNorm folded, fp32 MFMA) against the unfused torch modules it replaces
    (Conv1d+BN+ReLU; Conv1d+BN+ReLU+Conv1d) at the IA-SSD layer widths: 1e-4 of the output scale."""
    from spsnet_amd import fused, pointnet2_modules as M_
    torch.manual_seed(cin + cagg)
    mod = M_.PointnetSAModuleMSG_WithSampling(
        npoint_list=[M], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.5, 1.0], nsamples=[16, 16],
        mlps=[[4, 16, 16, cin // 2], [4, 16, 16, cin // 2]], use_xyz=True, dilated_group=False, aggregation_mlp=[cagg],
        confidence_mlp=[conf] if conf else None, num_class=3).to(dev).eval()
    gen = torch.Generator().manual_seed(3)
    for m_ in mod.modules():
        if isinstance(m_, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m_.running_mean.copy_(torch.randn(m_.num_features, generator=gen) * 0.1)
                m_.running_var.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.weight.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
                m_.bias.copy_(torch.randn(m_.num_features, generator=gen) * 0.1)
    pooled = torch.randn(3, cin, M, device=dev).relu()
    with torch.no_grad():
        got = fused.pointwise_tail(mod.aggregation_layer, mod.confidence_layers, pooled)
        assert got is not None, "fused tail did not apply"
        want_f = mod.aggregation_layer(pooled)
        want_c = mod.confidence_layers(want_f).transpose(1, 2) if conf else None
    assert got[0].shape == want_f.shape
    assert float((got[0] - want_f).abs().max()) <= 1e-4 * max(1.0, float(want_f.abs().max()))
    if conf:
        assert got[1].shape == want_c.shape and got[1].is_contiguous()
        assert float((got[1] - want_c).abs().max()) <= 1e-4 * max(1.0, float(want_c.abs().max()))
    else:
        assert got[1] is None
    # module-level switch: training mode keeps the reference's op sequence
    mod.train()
    assert fused.pointwise_tail(mod.aggregation_layer, mod.confidence_layers, pooled) is None


@pytest.mark.parametrize("N,M,j0,cnt,ra,nsa,rb,nsb", [(5000, 512, 128, 256, 0.4, 16, 1.5, 32), (16384, 4096, 3840, 256, 0.2, 16, 0.8, 32),
                                                       (4099, 300, 0, 300, 0.05, 8, 6.0, 64), (8192, 1024, 1000, 24, 1.0, 16, 1.0, 16)])
def test_ball_query_range_small_launch_kernels(ext, G, oracle, N, M, j0, cnt, ra, nsa, rb, nsb):
    """Centroid ranges small enough for the wave-per-centroid kernels (one wave, or four waves sharing a centroid):
    same rows as the oracle, rows outside the range untouched; includes empty balls and overfull balls."""
    from spsnet_amd import scenes
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, N, seed0=N + M)
    rng = np.random.default_rng(M)
    new_xyz = xyz[:, rng.integers(0, N, M)].copy()
    new_xyz[:, j0 + cnt - 1] = 500.0          # an empty ball inside the range
    ia = torch.full((2, M, nsa), -7, dtype=torch.int32, device="cuda")
    ib = torch.full((2, M, nsb), -7, dtype=torch.int32, device="cuda")
    ext.ball_query_full2_range(ra, rb, G.t(xyz), G.t(new_xyz), ia, ib, j0, cnt)
    wa, wb = oracle.ball_query(ra, nsa, xyz, new_xyz), oracle.ball_query(rb, nsb, xyz, new_xyz)
    np.testing.assert_array_equal(G.n(ia)[:, j0:j0 + cnt], wa[:, j0:j0 + cnt])
    np.testing.assert_array_equal(G.n(ib)[:, j0:j0 + cnt], wb[:, j0:j0 + cnt])
    assert (G.n(ia)[:, :j0] == -7).all() and (G.n(ia)[:, j0 + cnt:] == -7).all()
    assert (G.n(ib)[:, :j0] == -7).all() and (G.n(ib)[:, j0 + cnt:] == -7).all()


# ------------------------------------------------------------------ pruned FPS for scenes beyond one CU's registers
@pytest.mark.parametrize("cluster", ["1", "", "2,8", "4,5", "3,8", "8,1", "16,2", "12,2", "16,4", "8,8", "11,5"])
@pytest.mark.parametrize("N,m,kind", [(20000, 700, "lattice"), (40000, 2000, "dup"), (65536, 4096, "kitti"),
                                      (70001, 1500, "uniform"), (180000, 2500, "kitti"), (16385, 16385, "dup"),
                                      (30000, 900, "batch11")])
def test_fps_large_scene_kernel(ext, G, oracle, N, m, kind, cluster, monkeypatch):
    """fps_pruned_big.hip (points in a workspace, bucket metadata in registers, several picks per barrier) and
    fps_pruned_cluster.hip (the same scene spread over K workgroups that exchange their T best records per round)
    against the oracle and against the brute-force streaming kernel: indices AND final running distances bit-exact.
    Sizes cover the three metadata-row variants (<= 65 536, <= 131 072, <= 262 144 points), ragged last buckets and
    m = n; cluster = "K,T" forces a shape ("1": one workgroup, "": the launcher's choice), including odd K, a single
    published record per workgroup (everything else hidden behind its bound) and exact ties (lattice)."""
    from spsnet_amd import _lib, scenes
    if cluster:
        monkeypatch.setenv("SPS_FPS_CLUSTER", cluster)
    else:
        monkeypatch.delenv("SPS_FPS_CLUSTER", raising=False)
    rng = np.random.default_rng(N + m)
    if kind == "lattice":
        xyz = cloud(rng, 2, N, lattice=True)
    elif kind == "kitti":
        xyz, _ = scenes.make_batch("kitti-lidar-v1", 2 if N < 100000 else 1, N, seed0=21, dup_fraction=0.01)
    elif kind == "uniform":
        xyz, _ = scenes.make_batch("uniform-v1", 2, N, seed0=22)
    elif kind == "batch11":   # more than 8 scenes: the second block of 8 K workgroups, K halved by the residency rule
        xyz, _ = scenes.make_batch("kitti-lidar-v1", 11, N, seed0=23)
    else:
        xyz = cloud(rng, 2, N, dup=0.2)
    L = _lib.load()
    assert L.sps_fps_workspace_floats(N) > 0
    got, got_t = G.fps(ext, xyz, m)
    old = L.sps_set_fps_mode(1)
    try:
        brute, brute_t = G.fps(ext, xyz, m)
    finally:
        L.sps_set_fps_mode(old)
    np.testing.assert_array_equal(got, brute)
    np.testing.assert_array_equal(got_t, brute_t)
    if N * m <= 500_000_000:   # (the 180 000-point case included: one scene, ~2 s of oracle time)
        want, want_t = oracle.fps(xyz, m, return_temp=True)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_t, want_t)


@pytest.mark.parametrize("N,m,B", [(50000, 3000, 2), (16384, 512, 3)])
def test_fps_workgroup_exchanges_across_xcds(ext, G, oracle, N, m, B, monkeypatch):
    """SPS_FPS_CLUSTER_SPREAD=1 deals a scene's workgroups onto consecutive blocks = different XCDs (by default they share
    one): the record granules, the histogram exchange (write-through stores + sc1 loads) and the release / acquire hand-over
    of the sorted points then cross XCDs.  Clustered large-scene kernel and the sorting pre-pass, against the oracle."""
    from spsnet_amd import _lib, scenes
    monkeypatch.setenv("SPS_FPS_CLUSTER_SPREAD", "1")
    L = _lib.load()
    xyz, _ = scenes.make_batch("kitti-lidar-v1", B, N, seed0=61, dup_fraction=0.02)
    x = G.t(xyz)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=x.device)
    idx = torch.empty((B, m), dtype=torch.int32, device=x.device)
    work = torch.empty((B * int(L.sps_fps_workspace_floats(N)),), dtype=torch.float32, device=x.device)
    for rep in range(3):   # (the workspace is reused: stale tags and histograms of the previous launch are in it)
        temp.fill_(1e10)
        _lib.check(L.sps_fps_with_workspace(B, N, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr(), work.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "fps")
        want, want_t = oracle.fps(xyz, m, return_temp=True)
        np.testing.assert_array_equal(G.n(idx), want)
        np.testing.assert_array_equal(G.n(temp), want_t)


@pytest.mark.parametrize("N,m,B", [(16384, 1024, 3), (7000, 700, 2), (12000, 12000, 1), (16384, 300, 9)])
def test_fps_presorted_register_kernel(ext, G, oracle, N, m, B):
    """fps_presort.hip + the PRESORT instantiation of fps_pruned_kernel (the scenes sorted by a pre-pass of K workgroups per
    scene, K = 8 / 4 by batch size): sps_fps_with_workspace with a workspace at 6144 .. 16 384 points against the oracle --
    indices and final running distances bit-exact; duplicates and a lattice scene (exact ties) included."""
    from spsnet_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(N + m)
    xyz = cloud(rng, B, N, dup=0.1)
    xyz[0] = cloud(rng, 1, N, lattice=True)[0]
    x = G.t(xyz)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=x.device)
    idx = torch.empty((B, m), dtype=torch.int32, device=x.device)
    wf = int(L.sps_fps_workspace_floats(N))
    assert wf > 0
    work = torch.empty((B * wf,), dtype=torch.float32, device=x.device)
    _lib.check(L.sps_fps_with_workspace(B, N, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr(), work.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "fps")
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)


@pytest.mark.parametrize("N,m,B", [(16384, 1024, 3), (8192, 700, 2), (40000, 2048, 2), (70000, 1500, 1)])
def test_fps_exchange_give_up_is_redone(ext, G, oracle, N, m, B, monkeypatch):
    """Every cross-workgroup poll of the FPS kernels is FORCED to give up (sps_debug_set_exchange_spins(0xFFFFFFFF)): the
    K-way sorting pre-pass of the register kernel (<= 16 384 points) and the clustered large-scene kernel then raise their
    scenes' give-up words and leave -- no trap -- and the launcher's follow-up launch (self-sorting register kernel /
    one-workgroup large-scene kernel) samples those scenes: indices and final running distances bit-exact with the oracle.
    Then once more with the default bound (the follow-up launch is empty) for the same result."""
    from spsnet_amd import _lib
    L = _lib.load()
    monkeypatch.delenv("SPS_FPS_CLUSTER", raising=False)
    rng = np.random.default_rng(N + m)
    xyz = cloud(rng, B, N, dup=0.05)
    x = G.t(xyz)
    wf = int(L.sps_fps_workspace_floats(N))
    assert wf > 0
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    for bound in (0xFFFFFFFF, 0):
        old = L.sps_debug_set_exchange_spins(bound)
        try:
            temp = torch.full((B, N), 1e10, dtype=torch.float32, device=x.device)
            idx = torch.full((B, m), -7, dtype=torch.int32, device=x.device)
            work = torch.empty((B * wf,), dtype=torch.float32, device=x.device)
            _lib.check(L.sps_fps_with_workspace(B, N, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr(), work.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "fps")
            torch.cuda.synchronize()
        finally:
            L.sps_debug_set_exchange_spins(old)
        np.testing.assert_array_equal(G.n(idx), want)
        np.testing.assert_array_equal(G.n(temp), want_t)


@pytest.mark.parametrize("B,N,npts", [(2, 16384, None), (1, 40000, [4096, 1024, 256])])
def test_streamed_first_layer_survives_exchange_give_up(G, dev, B, N, npts):
    """The PUBLISHING producers behind a forced give-up of every cross-workgroup poll: the streamed first layer's consumers
    wait on the progress counter that the follow-up launch publishes (register kernel: as it samples; one-workgroup
    large-scene kernel: once at its end) -- every output of every layer bit-identical to the sequential pass."""
    from spsnet_amd import _lib, pointnet2_modules as M, sa_stack, scenes
    L = _lib.load()
    layers = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=npts), seed=12).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", B, N, seed0=63, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)
    with torch.no_grad():
        want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
        torch.cuda.synchronize()
        sa_stack.check_timeouts()
        old = L.sps_debug_set_exchange_spins(0xFFFFFFFF)
        try:
            got = sa_stack.run_sa_layers(layers, x, f)
            torch.cuda.synchronize()
        finally:
            L.sps_debug_set_exchange_spins(old)
        sa_stack.check_timeouts()     # (a consumer's bounded wait may or may not have run out behind the slower producer)
        for k, (la, lb) in enumerate(zip(got, want)):
            for ta, tb in zip(la, lb):
                assert (ta is None and tb is None) or torch.equal(ta, tb), f"layer {k}"


def test_fps_presorted_degenerate_clouds(ext, G, oracle):
    """All-equal, collinear and NaN / Inf clouds through the sorting pre-pass (its box comes from a strided sample)."""
    from spsnet_amd import _lib
    L = _lib.load()
    N, m = 8192, 300
    same = np.ones((1, N, 3), np.float32) * 2.5
    line = np.zeros((1, N, 3), np.float32)
    line[0, :, 0] = np.random.default_rng(0).permutation(N).astype(np.float32) * 0.01
    bad = cloud(np.random.default_rng(1), 1, N)
    bad[0, 16] = np.nan
    bad[0, 17] = np.nan
    bad[0, 904, 2] = np.inf
    bad[0, 1000, 0] = -np.inf
    work = torch.empty((int(L.sps_fps_workspace_floats(N)),), dtype=torch.float32, device="cuda")
    for xyz in (same, line, bad):
        x = G.t(xyz)
        temp = torch.full((1, N), 1e10, dtype=torch.float32, device=x.device)
        idx = torch.empty((1, m), dtype=torch.int32, device=x.device)
        _lib.check(L.sps_fps_with_workspace(1, N, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr(), work.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "fps")
        want, want_t = oracle.fps(xyz, m, return_temp=True)
        np.testing.assert_array_equal(G.n(idx), want)
        np.testing.assert_array_equal(G.n(temp), want_t)


# ------------------------------------------------------------------ deterministic gradients
@pytest.mark.parametrize("B,C,N,M,ns", [(2, 5, 700, 96, 16), (3, 67, 4096, 1024, 32), (1, 16, 300, 300, 1), (2, 8, 64, 512, 8)])
def test_deterministic_group_and_gather_grads(ext, G, oracle, B, C, N, M, ns):
    """sps_index_add_deterministic: the gradient of group_points / gather_points summed in ascending column order --
    bit-identical to the oracle's sequential loop, identical from run to run, and within fp32 rounding of the atomic
    kernels.  Includes heavily repeated targets (M*ns >> N)."""
    from spsnet_amd import pointnet2_utils as U
    rng = np.random.default_rng(B * 1000 + N)
    if ns == 1:
        idx = rng.integers(0, N, size=(B, M)).astype(np.int32)
        go = rng.standard_normal((B, C, M)).astype(np.float32)
        want = oracle.gather_points_grad(go, idx, N)
    else:
        idx = rng.integers(0, max(1, N // 4), size=(B, M, ns)).astype(np.int32)   # few targets, many hits each
        go = rng.standard_normal((B, C, M, ns)).astype(np.float32)
        want = oracle.group_points_grad(go, idx, N)
    outs = []
    for _ in range(2):
        gp = torch.zeros((B, C, N), device="cuda")
        ext.index_add_deterministic(G.t(go), G.t(idx), gp)
        outs.append(G.n(gp))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], want)
    # through autograd, switched by the module flag
    feats = torch.randn(B, C, N, device="cuda", requires_grad=True)
    old = U.DETERMINISTIC_BACKWARD
    try:
        grads = []
        for flag in (True, False):
            U.DETERMINISTIC_BACKWARD = flag
            feats.grad = None
            out = U.gather_operation(feats, G.t(idx)) if ns == 1 else U.grouping_operation(feats, G.t(idx))
            out.backward(G.t(go))
            grads.append(G.n(feats.grad))
    finally:
        U.DETERMINISTIC_BACKWARD = old
    np.testing.assert_array_equal(grads[0], want)
    np.testing.assert_allclose(grads[1], want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ whole backbones (IASSD_backbone.py / PAGNet_backbone.py)
@BOTH_PRECISIONS
@pytest.mark.parametrize("tag", ["iassd", "pagnet"])
@pytest.mark.parametrize("schedule", ["overlapped", "layer_by_layer"])
def test_golden_backbone(ext, G, dev, tag, schedule, mlp_precision):
    """IASSD_Backbone / PAGNet_Backbone.forward on 2 x 4096 points at the shipped widths against the reference's own
    forward (run over the C oracle, oracle/gen_golden.py:backbones): sampled centres bit-exact at every level, features,
    votes and class scores to 1e-4.  `overlapped` = the inference schedule (streamed layer 0, early FPS, surface features
    on a side stream), `layer_by_layer` = the reference's order (gradients enabled).  Both grouped-MLP arithmetics: in
    strict fp32 (the default) layer 5's 256 / 512 / 1024-wide scales run on the point-major fp32 MFMA kernel."""
    from spsnet_amd import backbones as BB, scenes
    g = np.load(os.path.join(GOLD, f"backbone_{tag}.npz"))
    base = BB.IASSD_KITTI_CFG if tag == "iassd" else BB.SPSNET_KITTI_CFG
    cls = BB.IASSD_Backbone if tag == "iassd" else BB.PAGNet_Backbone
    net = cls(BB.scaled_cfg(base, [int(v) for v in g["npoints"]]), num_class=3, input_channels=4)
    scenes.fill_parameters(net, int(g["seed"]))
    net = net.to(dev).eval()
    batch = dict(batch_size=2, points=G.t(g["points"]))
    if tag == "pagnet":
        batch["stds"] = G.t(g["stds"])
    if schedule == "overlapped":
        with torch.no_grad():
            out = net(batch)
    else:
        out = net(batch)
        assert out["centers_features"].requires_grad

    def close(a, ref, what):
        a = G.n(a)
        assert a.shape == ref.shape, what
        if ref.size == 0:   # the voting layer's (B, M, 0) "features"
            return
        tol = 1e-4 * max(1.0, float(np.abs(ref).max()))
        assert float(np.abs(a - ref).max()) <= tol, what

    for k in range(len(out["encoder_xyz"])):
        want = g[f"encoder_xyz_{k}"]
        if k >= 5:         # votes (centre + clamped regression output) and the last layer, which is centred on them
            close(out["encoder_xyz"][k], want, f"encoder_xyz[{k}]")
        else:              # sampled subsets of the input cloud: exact
            np.testing.assert_array_equal(G.n(out["encoder_xyz"][k]), want, err_msg=f"encoder_xyz[{k}]")
    for k, t in enumerate(out["encoder_features"]):
        key = f"encoder_features_{k}"
        if key in g.files:
            close(t, g[key], key)
    for k, t in enumerate(out["sa_ins_preds"]):
        key = f"sa_ins_preds_{k}"
        assert (key in g.files) == isinstance(t, torch.Tensor)
        if key in g.files:
            close(t, g[key], key)
    for key in ("ctr_offsets", "centers", "centers_origin", "centers_features"):
        close(out[key], g[key], key)
    np.testing.assert_array_equal(G.n(out["ctr_batch_idx"]), g["ctr_batch_idx"])
    assert len(out["encoder_coords"]) == int(g["n_encoder_coords"])


# ------------------------------------------------------------------ stability generator (stability_generate/model.py, eval path)
def test_stability_generator_stds(ext, G, dev):
    """Generate_center.forward in eval mode (stability_generate/model.py:545-588) at the shipped configuration on
    2 x 8192 points: the SA layer with every point a centroid (two-radius grid ball query + fused MLPs + aggregation)
    against the CPU oracle stack, and stds = sum exp(logvar / 2) against float64 numpy.  The PointnetSampling layer
    itself is pinned by the reference fixture generator_layer.npz; the head is three torch ops."""
    import copy
    from oracle import cpu_stack
    from spsnet_amd import scenes, stability_generator as SG
    cfg = copy.deepcopy(SG.SF_UNC_CFG)
    cfg['SA_CONFIG']['NPOINT_LIST'] = [[8192]]
    net = scenes.fill_parameters(SG.Generate_center(cfg), 21).eval()
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=31, dup_fraction=0.01)
    layer_cpu = cpu_stack.cpu_copy(net.feature_extract.SA_modules[0])
    want_xyz, want_feat, _, want_idx, _ = cpu_stack.sa_layer_cpu(layer_cpu, xyz, feats)
    w2 = net.feature_encoder.fc2.weight.detach().double().numpy()
    b2 = net.feature_encoder.fc2.bias.detach().double().numpy()
    logvar = want_feat.transpose(0, 2, 1).astype(np.float64) @ w2.T + b2
    want_stds = np.exp(0.5 * logvar).sum(-1)

    net = net.to(dev)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 8192)[:, None]
    points = np.concatenate([bidx, xyz.reshape(-1, 3), feats.transpose(0, 2, 1).reshape(-1, 1)], 1).astype(np.float32)
    with torch.no_grad():
        out = net(dict(batch_size=2, points=G.t(points)))
    np.testing.assert_array_equal(G.n(out['encoder_xyz'][1]), want_xyz)
    soc = G.n(out['soc_feature'])
    ref = want_feat.transpose(0, 2, 1)
    assert float(np.abs(soc - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    stds = G.n(out['stds'])
    assert stds.shape == (2, 8192)
    assert float(np.abs(stds - want_stds).max()) <= 1e-4 * max(1.0, float(np.abs(want_stds).max()))
    with pytest.raises(NotImplementedError):
        net.train()(dict(batch_size=2, points=G.t(points)))


# ------------------------------------------------------------------ training mode: forward, BatchNorm statistics, gradients
def _sa_layer_train_reference(mod_cpu, xyz, feats, oracle):
    """Pure-PyTorch fp32 restatement of PointnetSAModuleMSG_WithSampling.forward in train() mode on the CPU
    (pointnet2_modules.py:399-460): FPS / ball-query indices from the C oracle, grouping by advanced indexing so that
    autograd supplies the scatter-add the reference implements in group_points_grad_kernel."""
    B, N, _ = xyz.shape
    idx = torch.from_numpy(oracle.fps(xyz.numpy(), mod_cpu.npoint_list[0]).astype(np.int64))          # (B, M)
    new_xyz = torch.gather(xyz, 1, idx[..., None].expand(-1, -1, 3))
    bsel = torch.arange(B)[:, None, None]
    pooled = []
    for grouper, mlp in zip(mod_cpu.groupers, mod_cpu.mlps):
        bq = torch.from_numpy(oracle.ball_query(grouper.radius, grouper.nsample, xyz.numpy(), new_xyz.numpy()).astype(np.int64))
        rel = xyz[bsel, bq] - new_xyz[:, :, None, :]                       # (B, M, ns, 3)
        grouped = torch.cat([rel.permute(0, 3, 1, 2), feats.permute(0, 2, 1)[bsel, bq].permute(0, 3, 1, 2)], dim=1)
        y = mlp(grouped)
        pooled.append(torch.nn.functional.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1))
    nf = mod_cpu.aggregation_layer(torch.cat(pooled, dim=1))
    cls = mod_cpu.confidence_layers(nf).transpose(1, 2)
    return new_xyz, nf, cls, idx


def test_training_mode_matches_torch_reference(ext, G, dev, oracle):
    """An SA layer in train() mode (BatchNorm on batch statistics): outputs, updated running statistics and the
    gradients w.r.t. the input features and every parameter against the CPU restatement above.  Distinct coordinates
    (no exact ties in the max-pool) and a loss that reaches both heads."""
    import copy
    from spsnet_amd import pointnet2_modules as M, scenes
    torch.manual_seed(1)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.6, 1.2], nsamples=[8, 16],
        mlps=[[4, 8, 16], [4, 16, 24]], use_xyz=True, dilated_group=False, aggregation_mlp=[32], confidence_mlp=[16],
        num_class=3)
    scenes.fill_parameters(mod, 8)
    ref = copy.deepcopy(mod).train()
    mod = mod.to(dev).train()
    rng = np.random.default_rng(4)
    xyz = torch.from_numpy(rng.uniform(-3, 3, (2, 2048, 3)).astype(np.float32))
    feats0 = torch.from_numpy(rng.normal(size=(2, 4, 2048)).astype(np.float32))
    wn = torch.from_numpy(rng.normal(size=(2, 32, 256)).astype(np.float32))
    wc = torch.from_numpy(rng.normal(size=(2, 256, 3)).astype(np.float32))

    f_ref = feats0.clone().requires_grad_(True)
    _, nf_r, cls_r, idx_r = _sa_layer_train_reference(ref, xyz, f_ref, oracle)
    ((nf_r * wn).sum() + (cls_r * wc).sum()).backward()

    f_gpu = feats0.clone().to(dev).requires_grad_(True)
    new_xyz, nf, cls, idx, _ = mod(xyz.to(dev), f_gpu)
    ((nf * wn.to(dev)).sum() + (cls * wc.to(dev)).sum()).backward()

    np.testing.assert_array_equal(G.n(idx), idx_r.numpy().astype(np.int32))

    def close(a, b, what, tol=2e-4):
        a, b = G.n(a), b.detach().numpy()
        assert a.shape == b.shape, what
        assert float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max())), what

    close(nf, nf_r, "new_features")
    close(cls, cls_r, "cls")
    close(f_gpu.grad, f_ref.grad, "d/d features")
    gpu_sd, ref_sd = dict(mod.named_parameters()), dict(ref.named_parameters())
    for name, p in ref_sd.items():
        close(gpu_sd[name].grad, p.grad, "d/d " + name)
    for (name, bg), (_, br) in zip(mod.named_buffers(), ref.named_buffers()):
        if bg.dtype.is_floating_point:
            close(bg, br, "buffer " + name)


@pytest.mark.parametrize("input_grad", [False, True])
@pytest.mark.parametrize("fused_train", [True, False])
def test_eval_after_frozen_weight_training_forwards_sees_new_running_stats(dev, fused_train, input_grad, monkeypatch):
    """eval -> train-mode forwards with FROZEN weights (BatchNorm recalibration, swa_utils.update_bn, lr = 0) -> eval: the
    kernels write running_mean / running_var through raw pointers, and the folded inference caches are keyed on those
    tensors' versions -- the second eval must use the NEW statistics.  Checked against a twin module run through torch's own
    Conv / BatchNorm on the same inputs (grouping replayed from this module's indices is not needed: the layer is run on
    identical data by both, and only the statistics differ between the two eval passes).  input_grad: the train-mode forwards
    run with autograd on and an input that wants gradients, i.e. through this library's own train-mode kernels
    (mlp_train.hip / bn_relu_train.hip, which write the statistics through raw pointers); without it they run under
    no_grad through torch's batch_norm -- which does not move the statistics' version counters either."""
    import copy
    from spsnet_amd import pointnet2_modules as M, scenes
    monkeypatch.setattr(M, "FUSED_MLP_TRAINING", fused_train)
    torch.manual_seed(3)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[256], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.6, 1.2], nsamples=[16, 32],
        mlps=[[4, 16, 16, 32], [4, 32, 32, 64]], use_xyz=True, dilated_group=False, aggregation_mlp=[64], confidence_mlp=[32],
        num_class=3)
    scenes.fill_parameters(mod, 5)
    mod = mod.to(dev)
    for p in mod.parameters():
        p.requires_grad_(False)
    rng = np.random.default_rng(8)
    xyz = torch.from_numpy(rng.uniform(-3, 3, (2, 2048, 3)).astype(np.float32)).to(dev)
    feats = torch.from_numpy((3.0 * rng.normal(size=(2, 4, 2048)) + 1.5).astype(np.float32)).to(dev)
    with torch.no_grad():
        mod.eval()
        first = mod(xyz, feats)[1].clone()
        before = {k: v.clone() for k, v in mod.named_buffers() if v.dtype.is_floating_point}
        mod.train()
        for _ in range(3):
            if input_grad:
                with torch.enable_grad():
                    mod(xyz, feats.clone().requires_grad_(True))
            else:
                mod(xyz, feats)
        mod.eval()
        second = mod(xyz, feats)[1].clone()
        moved = max(float((v - before[k]).abs().max()) for k, v in mod.named_buffers() if v.dtype.is_floating_point)
        assert moved > 1e-3, "the train-mode forwards were supposed to move the running statistics"
        # a twin built from the CURRENT state (fresh caches by construction) is the expected result of the second eval
        twin = copy.deepcopy(mod).eval()
        for m_ in twin.modules():
            for attr in [a for a in vars(m_) if a.startswith("_sps")]:
                delattr(m_, attr)
        want = twin(xyz, feats)[1]
    assert float((second - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert float((second - first).abs().max()) > 1e-4, "the second eval pass still uses the statistics of the first"


# ------------------------------------------------------------------ pointnet2_stack: ragged batches (parity unpinned by the reference)
def _ragged(rng, sizes, dup=0.03):
    parts = []
    for n in sizes:
        p = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        k = int(n * dup)
        if k:
            p[rng.choice(n, k, replace=False)] = p[rng.integers(0, n, k)]
        parts.append(p)
    return np.concatenate(parts, 0), np.asarray(sizes, np.int32)


@pytest.mark.parametrize("sizes,qsizes,r,ns", [([1000, 37, 2500], [200, 5, 300], 0.5, 16), ([1], [1], 1.0, 4),
                                               ([5000, 5000], [1024, 1000], 0.2, 32), ([300, 300, 300, 300], [64, 1, 64, 7], 9.0, 8)])
def test_stack_ball_query_and_group(dev, G, oracle, sizes, qsizes, r, ns):
    """sps_ball_query_kernel_launcher_stack / sps_group_points(_grad)_kernel_launcher_stack through the extension mirror and
    the autograd layer (pointnet2_stack/pointnet2_utils.py), against the oracle's restatement of the CUDA kernels."""
    from spsnet_amd.pointnet2_stack import pointnet2_stack_cuda as SC, pointnet2_utils as SU
    rng = np.random.default_rng(sum(sizes))
    xyz, cnt = _ragged(rng, sizes)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    q = np.concatenate([np.concatenate([xyz[s + rng.integers(0, n, (m + 1) // 2)], rng.uniform(-3, 3, (m // 2, 3)).astype(np.float32)])
                        for s, n, m in zip(starts, sizes, qsizes)]).astype(np.float32)
    q[-1] = 100.0                                        # an empty ball
    qc = np.asarray(qsizes, np.int32)
    raw = torch.zeros((len(q), ns), dtype=torch.int32, device=dev)
    SC.ball_query_wrapper(len(sizes), len(q), r, ns, G.t(q), G.t(qc), G.t(xyz), G.t(cnt), raw)
    want_raw = oracle.stack_ball_query(r, ns, xyz, cnt, q, qc)
    np.testing.assert_array_equal(G.n(raw), want_raw)
    idx, empty = SU.ball_query(r, ns, G.t(xyz), G.t(cnt), G.t(q), G.t(qc))
    want_idx = want_raw.copy(); want_idx[want_raw[:, 0] == -1] = 0
    np.testing.assert_array_equal(G.n(idx), want_idx)
    np.testing.assert_array_equal(G.n(empty), want_raw[:, 0] == -1)
    feats = rng.normal(size=(len(xyz), 7)).astype(np.float32)
    f = G.t(feats).requires_grad_(True)
    out = SU.grouping_operation(f, G.t(cnt), idx, G.t(qc))
    np.testing.assert_array_equal(G.n(out), oracle.stack_group_points(feats, cnt, want_idx, qc))
    go = rng.normal(size=out.shape).astype(np.float32)
    out.backward(G.t(go))
    np.testing.assert_allclose(G.n(f.grad), oracle.stack_group_points_grad(go, want_idx, qc, cnt, len(xyz)), rtol=1e-4, atol=1e-5)
    nf, idx2 = SU.QueryAndGroup(r, ns, use_xyz=True)(G.t(xyz), G.t(cnt), G.t(q), G.t(qc), G.t(feats))
    assert nf.shape == (len(q), 3 + 7, ns) and torch.equal(idx2, idx)
    assert float(nf[empty].abs().max()) == 0.0 if bool(empty.any()) else True


@pytest.mark.parametrize("sizes,npoints", [([1000, 37, 2500], [100, 37, 512]), ([4096, 4096], [1024, 1]), ([9000], [2000])])
def test_stack_fps(dev, G, oracle, sizes, npoints):
    """stack_farthest_point_sampling (1024-thread tie rule, global indices) incl. lattice clouds with masses of equal
    distances, and the batch-form FPS of the stack module."""
    from spsnet_amd.pointnet2_stack import pointnet2_utils as SU
    rng = np.random.default_rng(sum(sizes))
    for lattice in (False, True):
        if lattice:
            xyz = np.concatenate([rng.integers(-4, 5, (n, 3)).astype(np.float32) * 0.25 for n in sizes])
        else:
            xyz, _ = _ragged(rng, sizes)
        cnt = np.asarray(sizes, np.int32)
        got = SU.stack_farthest_point_sample(G.t(xyz), G.t(cnt), list(npoints))
        np.testing.assert_array_equal(G.n(got), oracle.stack_fps(xyz, cnt, np.asarray(npoints, np.int32)))
    dense = rng.uniform(-3, 3, (2, 3000, 3)).astype(np.float32)
    np.testing.assert_array_equal(G.n(SU.farthest_point_sample(G.t(dense), 300)), oracle.fps(dense, 300))


def test_stack_three_nn_interpolate_and_voxel_query(dev, G, oracle):
    from spsnet_amd.pointnet2_stack import pointnet2_utils as SU, voxel_query_utils as VU
    rng = np.random.default_rng(17)
    known, kc = _ragged(rng, [700, 2, 1500])
    unknown, uc = _ragged(rng, [300, 50, 999], dup=0.0)
    unknown[:40] = known[:40]                            # exact matches -> zero distances and ties
    dist, idx = SU.three_nn(G.t(unknown), G.t(uc), G.t(known), G.t(kc))
    d2, widx = oracle.stack_three_nn(unknown, uc, known, kc)
    np.testing.assert_array_equal(G.n(idx), widx)
    np.testing.assert_array_equal(G.n(dist), np.sqrt(d2))
    feats = rng.normal(size=(len(known), 9)).astype(np.float32)
    w = rng.uniform(0, 1, (len(unknown), 3)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    f = G.t(feats).requires_grad_(True)
    out = SU.three_interpolate(f, idx, G.t(w))
    np.testing.assert_array_equal(G.n(out), oracle.stack_three_interpolate(feats, widx, w))
    go = rng.normal(size=out.shape).astype(np.float32)
    out.backward(G.t(go))
    np.testing.assert_allclose(G.n(f.grad), oracle.stack_three_interpolate_grad(go, widx, w, len(known)), rtol=1e-4, atol=1e-5)

    # voxel query: two scenes of 2000 points in a 0.5 m grid; the table keeps the last point written to a voxel
    B, n, vs = 2, 2000, 0.5
    xyz = rng.uniform(0, 8, (B * n, 3)).astype(np.float32)
    xyz[:, 2] *= 0.25
    grid = (4, 16, 16)                                   # Z, Y, X
    coords = np.floor(xyz / vs).astype(np.int32)[:, ::-1]  # z, y, x
    pi = -np.ones((B,) + grid, np.int32)
    for i in range(B * n):
        pi[i // n, coords[i, 0], coords[i, 1], coords[i, 2]] = i
    sel = np.concatenate([rng.choice(n, 300, replace=False) + b * n for b in range(B)])
    new_xyz = (xyz[sel] + rng.normal(scale=0.05, size=(len(sel), 3))).astype(np.float32)
    new_coords = np.concatenate([(sel // n)[:, None].astype(np.int32), coords[sel]], 1).astype(np.int32)
    idx, empty = VU.voxel_query((1, 2, 2), 0.8, 16, G.t(xyz), G.t(new_xyz), G.t(new_coords), G.t(pi))
    want = oracle.stack_voxel_query((1, 2, 2), 0.8, 16, xyz, new_xyz, new_coords, pi)
    wempty = want[:, 0] == -1
    want[wempty] = 0
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(empty), wempty)
    cnt = np.full((B,), n, np.int32)
    gf, gx, em = VU.VoxelQueryAndGrouping((1, 2, 2), 0.8, 16)(
        G.t(new_coords), G.t(xyz), G.t(cnt), G.t(new_xyz), G.t(np.full((B,), 300, np.int32)), G.t(xyz.copy()), G.t(pi))
    assert gf.shape == (600, 3, 16) and torch.equal(gf, gx)


def test_stack_modules_against_torch_reference(dev, G, oracle):
    """StackSAModuleMSG / StackPointnetFPModule (pointnet2_stack/pointnet2_modules.py:30-157) on ragged scenes, train mode,
    forward and the gradient w.r.t. the features, against a CPU restatement with oracle indices and torch indexing."""
    import copy
    from spsnet_amd import scenes
    from spsnet_amd.pointnet2_stack import pointnet2_modules as SM
    rng = np.random.default_rng(23)
    xyz, cnt = _ragged(rng, [900, 40, 1500], dup=0.0)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    qs = [128, 16, 200]
    q = np.concatenate([xyz[s + rng.choice(n, m, replace=False)] for s, n, m in zip(starts, cnt, qs)]).astype(np.float32)
    qc = np.asarray(qs, np.int32)
    feats = rng.normal(size=(len(xyz), 5)).astype(np.float32)
    mod = scenes.fill_parameters(SM.StackSAModuleMSG(radii=[0.5, 1.0], nsamples=[8, 16], mlps=[[5, 8, 16], [5, 8, 24]]), 3)
    ref = copy.deepcopy(mod).train()
    mod = mod.to(dev).train()
    f_gpu = G.t(feats).requires_grad_(True)
    _, out = mod(G.t(xyz), G.t(cnt), G.t(q), G.t(qc), f_gpu)
    # CPU restatement
    f_ref = torch.from_numpy(feats).requires_grad_(True)
    xt, qt = torch.from_numpy(xyz), torch.from_numpy(q)
    scene_start = torch.from_numpy(np.repeat(starts, qs).astype(np.int64))
    pooled = []
    for grouper, mlp in zip(ref.groupers, ref.mlps):
        raw = oracle.stack_ball_query(grouper.radius, grouper.nsample, xyz, cnt, q, qc)
        empty = torch.from_numpy(raw[:, 0] == -1)
        raw[raw[:, 0] == -1] = 0
        gi = torch.from_numpy(raw.astype(np.int64)) + scene_start[:, None]            # global rows (M, ns)
        gx = (xt[gi] - qt[:, None, :]).permute(0, 2, 1)                                # (M, 3, ns)
        gf = f_ref[gi].permute(0, 2, 1)
        grouped = torch.cat([gx, gf], dim=1)
        grouped = torch.where(empty[:, None, None], torch.zeros_like(grouped), grouped)
        y = mlp(grouped.permute(1, 0, 2).unsqueeze(0))
        pooled.append(torch.nn.functional.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1).squeeze(0).permute(1, 0))
    want = torch.cat(pooled, dim=1)
    wsum = torch.from_numpy(rng.normal(size=tuple(want.shape)).astype(np.float32))
    (want * wsum).sum().backward()
    (out * wsum.to(dev)).sum().backward()
    tol = lambda b: 2e-4 * max(1.0, float(np.abs(b).max()))
    assert float(np.abs(G.n(out) - want.detach().numpy()).max()) <= tol(want.detach().numpy())
    assert float(np.abs(G.n(f_gpu.grad) - f_ref.grad.numpy()).max()) <= tol(f_ref.grad.numpy())

    fp = scenes.fill_parameters(SM.StackPointnetFPModule(mlp=[16 + 5, 12]), 4)
    fp_ref = copy.deepcopy(fp).eval()
    fp = fp.to(dev).eval()
    kf = rng.normal(size=(len(q), 16)).astype(np.float32)
    with torch.no_grad():
        got = fp(G.t(xyz), G.t(cnt), G.t(q), G.t(qc), G.t(feats), G.t(kf))
        d2, idx = oracle.stack_three_nn(xyz, cnt, q, qc)
        rec = 1.0 / (torch.from_numpy(np.sqrt(d2)) + 1e-8)
        w = rec / rec.sum(-1, keepdim=True)
        interp = torch.from_numpy(oracle.stack_three_interpolate(kf, idx, w.numpy()))
        x = torch.cat([interp, torch.from_numpy(feats)], dim=1)
        want = fp_ref.mlp(x.permute(1, 0)[None, :, :, None]).squeeze(0).squeeze(-1).permute(1, 0).numpy()
    assert float(np.abs(G.n(got) - want).max()) <= tol(want)


def test_pool_max_matches_torch_max_pool2d(ext, dev):
    """sps_pool_max_fwd / _bwd against F.max_pool2d(x, [1, ns]) forward and backward, with ties (repeated first hits, ReLU
    zeros) and NaNs: same values, same gradient routing."""
    from spsnet_amd import pointnet2_modules as M
    g = torch.Generator(device=dev).manual_seed(2)
    for shape in ((2, 5, 33, 16), (1, 3, 7, 1), (2, 4, 20, 32), (1, 2, 9, 7), (1, 2, 5, 64), (3, 64, 700, 16)):
        x = torch.randn(shape, generator=g, device=dev)
        x = torch.relu(x)                                  # masses of equal zeros
        x[..., shape[-1] // 2:] = x[..., :1]               # repeated first hit
        if shape[-1] > 2:
            x[0, 0, 0, 1] = float("nan")
            x[-1, -1, -1, shape[-1] - 1] = float("nan")    # a NaN in the last lane's share
            x[-1, -1, -2, shape[-1] // 3] = float("nan")   # two NaNs in one row: the first one is the arg-max
            x[-1, -1, -2, shape[-1] - 2] = float("nan")
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        ya = M._pool_over_samples(a, 'max_pool')
        yb = torch.nn.functional.max_pool2d(b, kernel_size=[1, shape[-1]]).squeeze(-1)
        assert torch.equal(torch.nan_to_num(ya, nan=-7.0), torch.nan_to_num(yb, nan=-7.0))
        go = torch.randn(ya.shape, generator=g, device=dev)
        ya.backward(go); yb.backward(go)
        assert torch.equal(a.grad, b.grad)


def test_bn_relu_train_matches_torch(ext, dev):
    """sps_bn_relu_train_fwd / _bwd against nn.BatchNorm2d (train mode) + ReLU: output, running statistics,
    num_batches_tracked and the gradients w.r.t. input, weight and bias."""
    import copy
    from spsnet_amd import pointnet2_modules as M
    g = torch.Generator(device=dev).manual_seed(6)
    for shape in ((2, 5, 33, 16), (3, 16, 300, 32), (1, 1, 1, 2), (2, 7, 600, 16)):
        conv = torch.nn.Conv2d(shape[1], shape[1], 1, bias=False)
        bn = torch.nn.BatchNorm2d(shape[1])
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3); bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
        seq = torch.nn.Sequential(conv, bn, torch.nn.ReLU()).to(dev).train()
        ref = copy.deepcopy(seq)
        x = torch.randn(shape, generator=g, device=dev) * 3 + 1
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        ya = M._shared_mlp(seq, a)
        yb = ref(b)
        go = torch.randn(shape, generator=g, device=dev)
        ya.backward(go); yb.backward(go)
        close = lambda p, q, tol=1e-4: float((p.detach() - q.detach()).abs().max()) <= tol * max(1.0, float(q.detach().abs().max()))
        assert close(ya, yb) and close(a.grad, b.grad)
        assert close(seq[1].running_mean, ref[1].running_mean, 1e-5) and close(seq[1].running_var, ref[1].running_var, 1e-5)
        assert int(seq[1].num_batches_tracked) == int(ref[1].num_batches_tracked) == 1
        assert close(seq[1].weight.grad, ref[1].weight.grad) and close(seq[1].bias.grad, ref[1].bias.grad)
        assert close(seq[0].weight.grad, ref[0].weight.grad)


@pytest.mark.parametrize("neighbor_type,nsample", [(0, -1), (1, -1), (0, 12)])
def test_stack_vector_pool_family(dev, G, oracle, neighbor_type, nsample):
    """The four vector-pool functions (vector_pool_gpu.cu) against the oracle's restatement: local neighbour lists (per
    centre, whatever position the atomic counter gave them), three-NN of the grid centres inside them, pooled features /
    local xyz / counts for both pooling types, the set of grouped triples, the retry protocol and the gradient."""
    from spsnet_amd.pointnet2_stack import pointnet2_stack_cuda as SC, pointnet2_utils as SU
    rng = np.random.default_rng(31 + neighbor_type)
    xyz, cnt = _ragged(rng, [900, 30, 1400], dup=0.02)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    qs = [40, 3, 60]
    q = np.concatenate([xyz[s + rng.choice(n, m, replace=False)] + rng.normal(scale=0.05, size=(m, 3))
                        for s, n, m in zip(starts, cnt, qs)]).astype(np.float32)
    q[-1] = 50.0                                         # a centre without neighbours
    qc = np.asarray(qs, np.int32)
    M, dist = len(q), 0.9
    # --- local neighbour lists + three-NN of grid centres
    want_lists, want_lens = oracle.vp_local_neighbors(xyz, cnt, q, qc, dist * 2.0, nsample, neighbor_type)
    grid = (2, 2, 2)
    from spsnet_amd.pointnet2_stack.pointnet2_modules import VectorPoolAggregationModule as VPA
    centres = G.n(VPA.get_dense_voxels_by_center(G.t(q), dist, grid)).astype(np.float32)
    d, idx, avg = SU.three_nn_for_vector_pool_by_two_step(G.t(xyz), G.t(cnt), G.t(q), G.t(centres), G.t(qc), dist, nsample,
                                                          neighbor_type, 5, 8, 2.0)   # avg length 5: forces a retry
    wd2, widx = oracle.vp_three_nn_local(xyz, centres, want_lists, want_lens)
    np.testing.assert_array_equal(G.n(idx), widx)
    np.testing.assert_array_equal(G.n(d), np.sqrt(wd2))
    assert int(avg) == -(-int(want_lens.sum()) // M)
    assert (widx[-1] == -1).all()
    # --- pooling, both types
    feats = rng.normal(size=(len(xyz), 6)).astype(np.float32)
    for pooling_type in (0, 1):
        f = G.t(feats).requires_grad_(True)
        nf, nl, mean_pts, cg = SU.vector_pool_with_voxel_query_op(G.t(xyz), G.t(cnt), f, G.t(q), G.t(qc), 2, 2, 2, dist, 3, 1,
                                                                 2, nsample, neighbor_type, pooling_type)   # 2 per centre: retry
        cum, wnf, wnl, wcg, wgrouped = oracle.vp_pool(xyz, cnt, feats, q, qc, grid, dist, 3, 1, 10 ** 6, nsample,
                                                      neighbor_type, pooling_type)
        np.testing.assert_array_equal(G.n(cg), wcg)
        norm = np.maximum(wcg[:, :, None].astype(np.float32), 1e-6)
        np.testing.assert_array_equal(G.n(nf), (wnf.reshape(M, 8, 3) / norm).reshape(M, -1))
        np.testing.assert_array_equal(G.n(nl), (wnl.reshape(M, 8, 3) / norm).reshape(M, -1))
        assert int(mean_pts) == -(-cum // M)
        go = rng.normal(size=tuple(nf.shape)).astype(np.float32)
        nf.backward(G.t(go))
        want_grad = oracle.vp_pool_grad(go, wcg, wgrouped, len(xyz), 6)
        np.testing.assert_allclose(G.n(f.grad), want_grad, rtol=1e-4, atol=1e-5)
    # --- raw kernel: rows of grouped_idxs as a set, counter beyond the buffer
    nfb = torch.zeros((M, 24), device=dev); nlb = torch.zeros((M, 24), device=dev)
    cgb = torch.zeros((M, 8), dtype=torch.int32, device=dev); gi = torch.zeros((cum + 5, 3), dtype=torch.int32, device=dev)
    got = SC.vector_pool_wrapper(G.t(xyz), G.t(cnt), G.t(feats), G.t(q), G.t(qc), nfb, nlb, cgb, gi, 2, 2, 2, dist, 1, cum + 5,
                                 nsample, neighbor_type, 1)
    assert got == cum
    assert sorted(map(tuple, G.n(gi)[:cum].tolist())) == sorted(map(tuple, wgrouped.tolist()))


def test_stack_vector_pool_modules_run(dev, G):
    """VectorPoolAggregationModule (all three aggregation types) and the MSG wrapper: forward + backward, finite, shapes."""
    from spsnet_amd.pointnet2_stack import pointnet2_modules as SM
    rng = np.random.default_rng(5)
    xyz, cnt = _ragged(rng, [800, 1200], dup=0.0)
    q = np.concatenate([xyz[:50], xyz[800:870]]).astype(np.float32)
    qc = np.asarray([50, 70], np.int32)
    feats = G.t(rng.normal(size=(len(xyz), 32)).astype(np.float32)).requires_grad_(True)
    for kind in ("local_interpolation", "voxel_avg_pool", "voxel_random_choice"):
        mod = SM.VectorPoolAggregationModule(32, (2, 2, 2), kind, 16, 8, (24,), 0.8, -1, 0).to(dev).train()
        _, out = mod(xyz=G.t(xyz), xyz_batch_cnt=G.t(cnt), new_xyz=G.t(q), new_xyz_batch_cnt=G.t(qc), features=feats)
        assert out.shape == (120, 24) and torch.isfinite(out).all()
        feats.grad = None
        out.square().mean().backward()
        assert feats.grad is not None and torch.isfinite(feats.grad).all() and float(feats.grad.abs().sum()) > 0

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    group = Cfg(NUM_LOCAL_VOXEL=(2, 2, 2), POST_MLPS=(16,), MAX_NEIGHBOR_DISTANCE=0.8, NEIGHBOR_NSAMPLE=-1)
    cfg = Cfg(NUM_GROUPS=2, GROUP_CFG_0=group, GROUP_CFG_1=Cfg(group, MAX_NEIGHBOR_DISTANCE=1.6),
              LOCAL_AGGREGATION_TYPE='voxel_avg_pool', NUM_REDUCED_CHANNELS=16, NUM_CHANNELS_OF_LOCAL_AGGREGATION=8,
              MSG_POST_MLPS=(20,))
    msg = SM.VectorPoolAggregationModuleMSG(32, cfg).to(dev).train()
    _, out = msg(xyz=G.t(xyz), xyz_batch_cnt=G.t(cnt), new_xyz=G.t(q), new_xyz_batch_cnt=G.t(qc), features=feats)
    assert out.shape == (120, 20) and torch.isfinite(out).all()


@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_surface_feature_training_gradients(ext, G, dev, mode, monkeypatch):
    """FeatureExtraction with gradients through the fused kernels (sps_dense_edge_conv + sps_dense_edge_conv_bwd) against
    autograd over the op-by-op form: output, the gradient w.r.t. the input cloud and every parameter.  2 x 2048 dense points
    (full and padded balls); the loss reaches all 60 output channels."""
    from spsnet_amd import scenes, surface_feature as SF
    torch.manual_seed(9)
    net = SF.FeatureExtraction(dynamic_graph=(mode == "dynamic")).to(dev).train()
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, 2048, seed0=13)
    xyz = ((xyz - xyz.mean(1, keepdims=True)) * 0.15).astype(np.float32)
    wsum = torch.randn((2, 2048, 60), generator=torch.Generator().manual_seed(1)).to(dev)

    def run(fused_training):
        monkeypatch.setattr(SF, "FUSED_TRAINING", fused_training)
        for p in net.parameters():
            p.grad = None
        x = G.t(xyz).requires_grad_(True)
        out = net(x)
        (out * wsum).sum().backward()
        return out.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    out_a, dx_a, gp_a = run(True)
    out_b, dx_b, gp_b = run(False)

    def close(a, b, what, tol=2e-4):
        a, b = G.n(a), G.n(b)
        assert float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max())), what

    if mode == "static":
        close(out_a, out_b, "output")
        # the subgradient of max is discontinuous: where two neighbours' values agree to the last bits, the two forward
        # implementations may pick different ones -- a handful of points, visible in d/d xyz only
        off = ((dx_a - dx_b).abs().amax(-1) > 2e-4 * float(dx_b.abs().max())).float().mean()
        assert float(off) < 5e-3
        for k in gp_b:   # one flipped argmax moves a bias gradient by one point's share: a few 1e-3 of the largest entry
            close(gp_a[k], gp_b[k], "d/d " + k, tol=5e-3)
    else:
        # dynamic graph: a neighbour can flip with the last bit of the previous convolution's output, so
        # compare where the outputs agree: all but a handful of points, and gradients in aggregate
        rows = (out_a - out_b).abs().amax(-1) <= 1e-4 * float(out_b.abs().max())
        assert float(rows.float().mean()) > 0.999
        for k in gp_b:
            rel = float((gp_a[k] - gp_b[k]).abs().max()) / max(1.0, float(gp_b[k].abs().max()))
            assert rel <= 2e-2, k


@pytest.mark.parametrize("relative", [True, False])
def test_dense_edge_conv_backward_kernel(ext, G, dev, relative, monkeypatch):
    """One DenseEdgeConv in isolation (same input for both paths, so the argmax choices agree): output and every gradient
    of sps_dense_edge_conv_bwd against autograd over the op-by-op form, 1e-5 relative."""
    from spsnet_amd import scenes, surface_feature as SF
    torch.manual_seed(4)
    xyz, _ = scenes.make_batch("kitti-lidar-v1", 2, 2048, seed0=13)
    pos = G.t(((xyz - xyz.mean(1, keepdims=True)) * 0.15).astype(np.float32))
    conv = SF.DenseEdgeConv(24, 3, 12, knn=16, relative_feat_only=relative).to(dev).train()
    x0 = torch.randn(2, 2048, 24, device=dev)
    w = torch.randn(2, 2048, 60, device=dev)
    res = {}
    for fused_training in (True, False):
        monkeypatch.setattr(SF, "FUSED_TRAINING", fused_training)
        for p in conv.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        out = conv(x, pos)
        (out * w).sum().backward()
        res[fused_training] = [out.detach(), x.grad.detach()] + [p.grad.detach().clone() for p in conv.parameters()]
    for a, b in zip(res[True], res[False]):
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("cin,relu", [(3, False), (60, True), (17, True)])
def test_linear_rows_training(ext, dev, cin, relu):
    """sps_linear_rows + sps_linear_rows_bwd (fused.LinearRowsTrain) against nn.Linear (+ ReLU) autograd."""
    from spsnet_amd import fused
    g = torch.Generator(device=dev).manual_seed(cin)
    lin = torch.nn.Linear(cin, 24).to(dev)
    x0 = torch.randn((3, 1000, cin), generator=g, device=dev)
    go = torch.randn((3, 1000, 24), generator=g, device=dev)
    a = x0.clone().requires_grad_(True)
    ya = fused.LinearRowsTrain.apply(a, lin.weight, lin.bias, relu)
    ya.backward(go)
    got = (ya.detach(), a.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone())
    lin.weight.grad = None; lin.bias.grad = None
    b = x0.clone().requires_grad_(True)
    yb = lin(b)
    yb = torch.relu(yb) if relu else yb
    yb.backward(go)
    for p, q in zip(got, (yb.detach(), b.grad, lin.weight.grad, lin.bias.grad)):
        assert float((p - q).abs().max()) <= 1e-4 * max(1.0, float(q.abs().max()))


@pytest.mark.parametrize("tag", ["iassd", "pagnet"])
@BOTH_TRAIN_PRECISIONS
def test_backbone_training_step_runs(ext, G, dev, tag, train_precision):
    """tools/train.py-style use of the backbone mirrors: train() mode, forward + backward through the fused training
    kernels (BatchNorm+ReLU, max-pool, LDS scatter, DenseEdgeConv / FCLayer backward); finite gradients on every parameter
    that takes part, running statistics updated."""
    from spsnet_amd import backbones as BB, scenes
    base = BB.IASSD_KITTI_CFG if tag == "iassd" else BB.SPSNET_KITTI_CFG
    cls = BB.IASSD_Backbone if tag == "iassd" else BB.PAGNet_Backbone
    net = scenes.fill_parameters(cls(BB.scaled_cfg(base, [1024, 256, 128, 64, -1, 64]), num_class=3, input_channels=4), 2)
    net = net.to(dev).train()
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 4096, seed0=77)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 4096)[:, None]
    points = np.concatenate([bidx, xyz.reshape(-1, 3), feats.transpose(0, 2, 1).reshape(-1, 1)], 1).astype(np.float32)
    batch = dict(batch_size=2, points=G.t(points))
    if tag == "pagnet":
        batch["stds"] = G.t(np.random.default_rng(1).uniform(0, 40, (2, 4096)).astype(np.float32))
    before = {k: v.clone() for k, v in net.state_dict().items() if k.endswith("running_mean")}
    # Every convolution and BatchNorm of the step -- the grouped MLPs up to layer 5's 256 / 512 / 1024-wide scales, the
    # aggregation / confidence / vote stacks up to 1536 -> 512, the class-score and offset heads -- runs on this library's
    # kernels IN BOTH training arithmetics: asserted on what the GPU ran (the profiler's kernel records of one whole step),
    # not on which Python function was called.
    from spsnet_amd import pointnet2_modules as PM
    fused_calls = []
    orig_fused = PM._GroupedMLPPoolTrain.apply
    PM._GroupedMLPPoolTrain.apply = lambda *a, **k: fused_calls.append(tuple(a[2].shape)) or orig_fused(*a, **k)

    def step():
        out = net(dict(batch))
        loss = out["centers_features"].square().mean() + out["ctr_offsets"][:, 1:].square().mean()
        for t in out["sa_ins_preds"]:
            if isinstance(t, torch.Tensor):
                loss = loss + t[..., 1:].square().mean()
        for p in net.parameters():
            p.grad = None
        loss.backward()

    try:
        names = G.kernel_names(step)
    finally:
        del PM._GroupedMLPPoolTrain.apply                 # (back to the inherited autograd.Function.apply)
    assert sum(names.values()) > 100 and any("tconv_kernel" in k for k in names), "the profiler recorded no kernels of the step"
    assert not G.library_kernels(names), G.library_kernels(names)
    f32 = train_precision == "fp32"
    # (the last template argument of tconv_kernel / twgrad_kernel is the arithmetic: true = exact fp32 MFMA)
    assert all((", true>(" in k) == f32 for k in names if "tconv_kernel<" in k or "twgrad_kernel<" in k), \
        sorted(k for k in names if "tconv_kernel<" in k)[:4]
    assert any(shape[1] == 259 for shape in fused_calls), fused_calls      # layer 5: 256 feature channels + xyz
    grads = [(k, p.grad) for k, p in net.named_parameters() if p.grad is not None]
    assert len(grads) > 40 and all(torch.isfinite(g).all() for _, g in grads)
    assert any(float(g.abs().sum()) > 0 for _, g in grads)
    if tag == "pagnet":
        assert any(k.startswith("SF_extract") and float(g.abs().sum()) > 0 for k, g in grads)
    after = net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("B,ci,co,M,ns", [(2, 4, 16, 128, 16), (2, 67, 64, 96, 32), (1, 131, 256, 48, 16), (3, 96, 128, 20, 16),
                                          (2, 256, 256, 64, 32), (2, 19, 22, 10, 8)])
def test_conv1x1_training_kernels(ext, dev, B, ci, co, M, ns):
    """sps_conv1x1_apply / sps_conv1x1_wgrad (pointnet2_modules._Conv1x1Train) against nn.Conv2d(kernel 1, no bias)
    autograd: output, input gradient, weight gradient; channel counts that are not multiples of 4 / 16 / 64 included."""
    from spsnet_amd import pointnet2_modules as M_
    g = torch.Generator(device=dev).manual_seed(ci * 1000 + co)
    conv = torch.nn.Conv2d(ci, co, 1, bias=False).to(dev)
    x0 = torch.randn((B, ci, M, ns), generator=g, device=dev)
    go = torch.randn((B, co, M, ns), generator=g, device=dev)
    a = x0.clone().requires_grad_(True)
    ya = M_._Conv1x1Train.apply(a, conv.weight)
    ya.backward(go)
    got = (ya.detach(), a.grad.clone(), conv.weight.grad.clone())
    conv.weight.grad = None
    b = x0.clone().requires_grad_(True)
    yb = conv(b)
    yb.backward(go)
    for p, q, tol in zip(got, (yb.detach(), b.grad, conv.weight.grad), (1e-4, 1e-4, 2e-4)):
        assert p.shape == q.shape
        assert float((p - q).abs().max()) <= tol * max(1.0, float(q.abs().max()))


def test_stack_ops_agree_with_pinned_batch_ops(ext, dev, G):
    """Indirect pin for the stacked ops (whose oracle restatement has no reference fixture to check against): on scenes
    of EQUAL size the stacked ball query, grouping, FPS, three_nn and three_interpolate are the same functions as the
    batch-form ops, and those are pinned by the reference-generated goldens.  Bit-exact indices, equal features."""
    from spsnet_amd import pointnet2_utils as BU
    from spsnet_amd.pointnet2_stack import pointnet2_utils as SU
    g = torch.Generator(device=dev).manual_seed(41)
    B, N, M, C, ns, r = 3, 1500, 200, 7, 16, 0.45
    xyz = torch.rand((B, N, 3), generator=g, device=dev) * 4.0
    feats = torch.randn((B, C, N), generator=g, device=dev)
    ncnt = torch.full((B,), N, dtype=torch.int32, device=dev)
    mcnt = torch.full((B,), M, dtype=torch.int32, device=dev)
    # farthest point sampling: global rows of the stacked form vs per-scene indices of the batch form
    fb = BU.furthest_point_sample(xyz, M)
    fs = SU.stack_farthest_point_sample(xyz.view(-1, 3), ncnt, M)
    off = (torch.arange(B, device=dev, dtype=torch.int32) * N)[:, None]
    assert torch.equal(fs.view(B, M), fb + off)
    new_xyz = torch.gather(xyz, 1, fb.long()[..., None].expand(-1, -1, 3)).contiguous()
    new_xyz[:, -3:] += 50.0                                      # a few empty balls
    # ball query (+ the empty-ball convention: all-zero rows on both sides)
    ib = BU.ball_query(r, ns, xyz, new_xyz)
    is_, empty = SU.ball_query(r, ns, xyz.view(-1, 3), ncnt, new_xyz.view(-1, 3), mcnt)
    assert torch.equal(is_.view(B, M, ns), ib)
    assert bool(empty.view(B, M)[:, -3:].all()) and not bool(empty.view(B, M)[:, :-3].any())
    # grouping: (M_total, C, ns) stacked vs (B, C, M, ns) batch; empty balls read point 0 of their scene on both sides
    gb = BU.grouping_operation(feats, ib)
    gs = SU.grouping_operation(feats.permute(0, 2, 1).reshape(-1, C).contiguous(), ncnt, is_, mcnt)
    assert torch.equal(gs.view(B, M, C, ns).permute(0, 2, 1, 3), gb)
    # three_nn / three_interpolate: unknown = all points, known = the sampled ones
    known = torch.gather(xyz, 1, fb.long()[..., None].expand(-1, -1, 3)).contiguous()
    db, tb = BU.three_nn(xyz, known)
    ds, ts = SU.three_nn(xyz.view(-1, 3), ncnt, known.view(-1, 3), mcnt)
    assert torch.equal(ts.view(B, N, 3), tb + (torch.arange(B, device=dev, dtype=torch.int32) * M)[:, None, None])
    assert torch.equal(ds.view(B, N, 3), db)
    w = 1.0 / (db + 1e-8)
    w = w / w.sum(dim=2, keepdim=True)
    kf = torch.randn((B, C, M), generator=g, device=dev)
    yb = BU.three_interpolate(kf, tb, w)                          # (B, C, N)
    ys = SU.three_interpolate(kf.permute(0, 2, 1).reshape(-1, C).contiguous(), ts, w.view(-1, 3).contiguous())
    np.testing.assert_allclose(ys.view(B, N, C).permute(0, 2, 1).cpu().numpy(), yb.cpu().numpy(), rtol=0, atol=1e-6)


def test_backbone_rejects_scenes_of_unequal_size(ext, dev):
    """The deferred equal-counts verdict (backbones.equal_counts_check) raises on the GPU path as the reference's
    assert does, and passes silently for well-formed batches (covered by the golden tests)."""
    from spsnet_amd import backbones, scenes
    net = backbones.IASSD_Backbone(backbones.scaled_cfg(backbones.IASSD_KITTI_CFG, [1024, 256, 128, 64, -1, 64]), num_class=3, input_channels=4)
    scenes.fill_parameters(net, 3)
    net = net.to(dev).eval()
    B, N = 2, 2048
    g = torch.Generator(device=dev).manual_seed(1)
    pts = torch.rand((B * N, 4), generator=g, device=dev) * 10.0
    bidx = torch.arange(B, device=dev).repeat_interleave(N).float()
    bidx[N - 1] = 1.0                                             # scene 0 has N-1 points, scene 1 has N+1
    with torch.no_grad(), pytest.raises(AssertionError):
        net({'batch_size': B, 'points': torch.cat([bidx[:, None], pts], dim=1)})
    torch.cuda.synchronize()


def test_conv1x1_train_wide_layers_match_conv2d(ext, dev):
    """_Conv1x1Train on both of its routes (conv1x1_train.hip below pointnet2_modules._BLAS_MIN channels, batched library
    GEMM from there up) against nn.functional.conv2d: output, input gradient, weight gradient."""
    from spsnet_amd import pointnet2_modules as M
    g = torch.Generator(device=dev).manual_seed(12)
    for (B, ci, co, m, ns) in ((2, 131, 128, 40, 16), (3, 64, 96, 24, 32), (2, 40, 200, 16, 16), (1, 256, 64, 8, 16)):
        x = torch.randn((B, ci, m, ns), generator=g, device=dev)
        w = torch.randn((co, ci, 1, 1), generator=g, device=dev) / ci ** 0.5
        go = torch.randn((B, co, m, ns), generator=g, device=dev)
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ya = M._Conv1x1Train.apply(xa, wa)
        yb = torch.nn.functional.conv2d(xb.double(), wb.double())
        ya.backward(go); yb.backward(go.double())
        for got, ref in ((ya, yb), (xa.grad, xb.grad), (wa.grad, wb.grad)):
            scale = float(ref.abs().max())
            assert float((got.double() - ref).abs().max()) <= 2e-6 * scale + 1e-6


# ------------------------------------------------------------------ pointnet2_stack modules vs reference-generated fixtures
def test_stack_modules_match_reference_fixtures(dev):
    """tests/golden/stackmod_*.npz (the REFERENCE's pointnet2_stack Python run over the C oracle, oracle/gen_golden_stack.py)
    replayed through the build's stack modules on the HIP extension: indices / groupings bit-exact, module outputs and
    input gradients 1e-5, state_dict names by strict load.  Pins everything above the extension boundary; the kernels'
    arithmetic stays pinned by the oracle only."""
    from tests import stack_replay as R
    R.replay_sa_fp(dev)
    R.replay_vector_pool(dev)
    R.replay_voxel_sa(dev)


# ------------------------------------------------------------------ fp16 feature tensors (BASELINE configs[4])
# Tolerance of the fp16-feature path against the fp32 CPU stack run on the same (fp16-rounded) input features: the stored
# features are halves (relative spacing 2^-11 = 4.9e-4) and every MFMA operand is rounded to fp16 once; measured on MI355X
# (tools/fp16_err.py): max 4.5e-4, mean 2.7e-5 of a layer's largest feature at every layer of every shape below.
FP16_MAX, FP16_MEAN, FP16_CLS = 2e-3, 1e-4, 5e-4


def _fp16_stack_check(G, dev, B, N, npts, ns, seed0, exact_layers=(0, 1)):
    from oracle import cpu_stack
    from spsnet_amd import fused, pointnet2_modules as M, sa_stack, scenes
    cfg = sa_stack.scaled_config(npoints=npts, nsamples=ns)
    layers = sa_stack.build_sa_layers(M, cfg, seed=2)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", B, N, seed0=seed0)
    feats_h = feats.astype(np.float16)
    want = cpu_stack.sa_stack_cpu(cpu_stack.cpu_copy(layers), xyz, feats_h.astype(np.float32))
    layers = layers.to(dev)
    with torch.no_grad():
        got = sa_stack.run_sa_layers(layers, G.t(xyz), G.t(feats_h))
    assert not sa_stack.check_timeouts() and not fused.check_overflow()

    def feature_check(gf, wf):
        scale = float(np.abs(wf).max())
        err = np.abs(gf - wf)
        assert float(err.max()) <= FP16_MAX * scale and float(err.mean()) <= FP16_MEAN * scale, (err.max(), err.mean(), scale)

    for k, ((gx, gf, gc, gi), (wx, wf, wc, wi)) in enumerate(zip(got, want)):
        assert gf.dtype == torch.float16 and gx.dtype == torch.float32
        if k in exact_layers:   # D-FPS layers: sampled indices and centroids bit-exact, whatever the feature dtype
            np.testing.assert_array_equal(G.n(gi), wi)
            np.testing.assert_array_equal(G.n(gx), wx)
            feature_check(G.n(gf.float()), wf)
            if wc is not None:
                assert float(np.abs(G.n(gc) - wc).max()) <= FP16_CLS
        else:                   # score-sampled layer: picks agree up to near-ties of scores computed from fp16 features
            gi_n, shared = G.n(gi), []
            for b in range(B):
                common, gp, wp = np.intersect1d(gi_n[b], wi[b], return_indices=True)
                shared.append(len(common) / wi.shape[1])
                np.testing.assert_array_equal(G.n(gx)[b][gp], wx[b][wp])
                feature_check(G.n(gf.float())[b][:, gp], wf[b][:, wp])
            assert np.mean(shared) >= 0.97
    return xyz, got, want


@pytest.mark.parametrize("B,N,npts,ns", [(2, 4096, [1024, 256, 128], None), (2, 8192, [2048, 512, 128], [(64, 64)] * 3)])
def test_fp16_feature_stack_small(G, dev, B, N, npts, ns):
    """fp16 feature tensors in HBM feeding the MFMA kernels directly (mode 3 of sps_sa_group_mlp_ex, fp16 outputs of the
    aggregation kernel): nsample 16 & 32 and nsample 64, against the fp32 CPU oracle stack."""
    _fp16_stack_check(G, dev, B, N, npts, ns, seed0=31)


def test_config5_shape_end_to_end(ext, G, oracle, dev):
    """BASELINE configs[4], one GPU's share, at FULL size: 1 scene x 180 000 points -> 16 384 / 4 096 / 1 024 centroids,
    nsample 64 at both radii, fp16 features (shapes scaled from tools/cfgs/waymo_models/IA-SSD.yaml:45-60).  Against the
    ORACLE: the large-scene FPS (fps_pruned_big.hip) and both D-FPS layers bit-exact, the layer-0 ball-query rows
    (16 384 x 180 000 pairs per radius) bit-exact, features at the stated fp16 tolerance.  ~20 s of CPU oracle work."""
    xyz, got, want = _fp16_stack_check(G, dev, 1, 180000, [16384, 4096, 1024], [(64, 64)] * 3, seed0=7)
    # the kernels below the stack, each against the oracle at this size
    idx, temp = G.fps(ext, xyz, 16384)
    want_idx, want_temp = oracle.fps(xyz, 16384, return_temp=True)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(temp, want_temp)
    new_xyz = want[0][0]
    for radius in (0.2, 0.8):
        np.testing.assert_array_equal(G.ball_query(ext, radius, 64, xyz, new_xyz), oracle.ball_query(radius, 64, xyz, new_xyz))


# ------------------------------------------------------------------ packed columns (only a ball's distinct neighbours are computed)
def _padded_rows(rng, B, M, ns, N):
    """Ball-query-shaped rows: cnt sorted distinct indices, then repeats of the first (ball_query_gpu.cu:35-42); counts
    cover every slot class, full rows and single-hit rows (= empty balls, which keep the caller's zeros)."""
    idx = np.zeros((B, M, ns), np.int32)
    for b in range(B):
        for j in range(M):
            cnt = int(rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64])) if rng.random() < 0.7 else int(rng.integers(1, ns + 1))
            cnt = min(cnt, ns)
            row = np.sort(rng.choice(N, cnt, replace=False))
            idx[b, j, :cnt] = row
            idx[b, j, cnt:] = row[0]
    return idx


@pytest.mark.parametrize("B,M,ns,j0,jcount", [(2, 200, 16, 0, 200), (3, 130, 32, 0, 130), (1, 77, 64, 0, 77), (2, 256, 32, 64, 100),
                                             (2, 64, 8, 0, 64)])
def test_pack_columns_stream(dev, G, B, M, ns, j0, jcount):
    """sps_pack_columns: every centroid of the range appears exactly once, in a slot of 2^ceil(log2 cnt) columns aligned to
    its size that holds exactly its distinct neighbours (+ repeats of the first); tiles come in multiples of four; unused
    lanes are marked."""
    from spsnet_amd import fused
    rng = np.random.default_rng(B * 1000 + M + ns)
    idx = _padded_rows(rng, B, M, ns, 5000)
    pc = fused.pack_columns(G.t(idx), j0, jcount)
    ntiles = int(pc.ntiles.item())
    assert ntiles % 4 == 0 and 0 < ntiles <= pc.cap
    cols = G.n(pc.cols)[:ntiles * 16]
    meta = G.n(pc.meta)[:ntiles * 16].view(np.uint32)
    j, scene, lg, unused = meta & 0xFFFFF, (meta >> 20) & 0xFF, (meta >> 28) & 7, meta >> 31
    seen = set()
    e = 0
    while e < ntiles * 16:
        if unused[e]:
            e += 1
            continue
        size = 1 << int(lg[e])
        assert e % size == 0, "slot not aligned to its size"
        assert (j[e:e + size] == j[e]).all() and (scene[e:e + size] == scene[e]).all() and not unused[e:e + size].any()
        key = (int(scene[e]), int(j[e]))
        assert key not in seen and j0 <= key[1] < j0 + jcount
        seen.add(key)
        row = idx[key[0], key[1]]
        cnt = len(np.unique(row))
        assert size == 1 << int(np.ceil(np.log2(cnt))) if cnt > 1 else size == 1
        np.testing.assert_array_equal(np.unique(cols[e:e + size]), np.unique(row))
        assert cols[e] == row[0]
        e += size
    assert len(seen) == B * jcount


@pytest.mark.parametrize("mode", ["fp32", "fp16x2", "half"])
@pytest.mark.parametrize("c_feat,widths,ns", [(1, [16, 16, 32], 16), (1, [32, 32, 64], 32), (64, [64, 64, 128], 16),
                                              (64, [64, 96, 128], 32), (128, [128, 128, 256], 16), (128, [128, 256, 256], 32),
                                              (64, [64, 96, 128], 64), (1, [32, 32, 64], 64)])
def test_packed_group_mlp_is_bit_identical(G, dev, mode, c_feat, widths, ns):
    """The grouped MLP over packed columns against the same kernel over all nsample columns: pooled features identical bit
    for bit (a repeated column reproduces the first column's activations, max is idempotent), in both output layouts, for
    the fp32, split-fp16 (per-wave kernel) and fp16-feature arithmetic."""
    from spsnet_amd import fused, pointnet2_modules as M
    if mode == "fp32" and widths[0] >= 128 and ns == 64:
        pytest.skip("no fp32 variant")
    rng = np.random.default_rng(ns * 7 + c_feat)
    B, N, Mc = 2, 3000, 192
    old, old_share = fused.set_precision("fp32" if mode == "fp32" else "fp16x2"), fused.SHARE_WEIGHTS
    fused.SHARE_WEIGHTS = False      # the per-wave split-fp16 kernel (the shared-stream kernel keeps the padded form)
    try:
        torch.manual_seed(ns + c_feat)
        mlp = M._conv_bn_relu_stack([c_feat + 3] + list(widths), torch.nn.Conv2d, torch.nn.BatchNorm2d).to(dev).eval()
        gen = torch.Generator().manual_seed(3)
        for m_ in mlp.modules():
            if isinstance(m_, torch.nn.BatchNorm2d):
                with torch.no_grad():
                    m_.running_mean.copy_(torch.randn(m_.num_features, generator=gen) * 0.2)
                    m_.running_var.copy_(torch.rand(m_.num_features, generator=gen) + 0.5)
        xyz = G.t(cloud(rng, B, N))
        new_xyz = xyz[:, :Mc].contiguous()
        feats = G.t(rng.normal(size=(B, c_feat, N)).astype(np.float32))
        if mode == "half":
            feats = feats.half()
        idx = G.t(_padded_rows(rng, B, Mc, ns, N))
        packed = fused.pack_scale(mlp, ns, half=mode == "half")
        assert packed is not None and packed.split == {"fp32": 0, "fp16x2": (1 if widths[0] >= 32 else 0), "half": 3}[mode]
        alloc = torch.zeros if ns > 32 else torch.empty
        c3 = widths[-1]
        ref = alloc((B, c3, Mc), dtype=torch.float32, device=dev)
        fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, ref, 0)
        columns = fused.pack_columns(idx)
        got = alloc((B, c3, Mc), dtype=torch.float32, device=dev)
        fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, got, 0, columns=columns)
        got_pm = alloc((B, Mc, c3), dtype=torch.float32, device=dev)
        fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, got_pm, 0, columns=columns, out_point_major=True)
        torch.cuda.synchronize()
        assert float(ref.abs().max()) > 0
        assert torch.equal(got, ref)
        assert torch.equal(got_pm.transpose(1, 2), ref)     # (the padded per-wave kernels keep the reference layout only)
        with pytest.raises(Exception):
            fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, got_pm, 0, out_point_major=True)
        assert int(columns.ntiles.item()) * 16 < B * Mc * ns      # and fewer columns were computed
    finally:
        fused.set_precision(old)
        fused.SHARE_WEIGHTS = old_share


def test_shared_stream_kernel_point_major_output(G, dev):
    """sa_mlp_f16_lds.hip with a point-major `out` (lanes <-> rows: contiguous stores) against its channel-major form."""
    from spsnet_amd import fused, pointnet2_modules as M
    rng = np.random.default_rng(5)
    B, N, Mc, ns, c_feat, widths = 2, 2048, 256, 32, 128, [128, 256, 256]
    old = fused.set_precision("fp16x2")
    try:
        torch.manual_seed(1)
        mlp = M._conv_bn_relu_stack([c_feat + 3] + widths, torch.nn.Conv2d, torch.nn.BatchNorm2d).to(dev).eval()
        xyz = G.t(cloud(rng, B, N))
        new_xyz = xyz[:, :Mc].contiguous()
        feats = G.t(rng.normal(size=(B, c_feat, N)).astype(np.float32))
        idx = G.t(_padded_rows(rng, B, Mc, ns, N))
        packed = fused.pack_scale(mlp, ns)
        assert packed.split == 2
        ref = torch.empty((B, widths[-1], Mc), dtype=torch.float32, device=dev)
        fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, ref, 0)
        pm = torch.empty((B, Mc, widths[-1]), dtype=torch.float32, device=dev)
        fused.group_mlp_pool(xyz, new_xyz, feats, idx, packed, pm, 0, out_point_major=True)
        assert torch.equal(pm.transpose(1, 2), ref)
    finally:
        fused.set_precision(old)


@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
def test_stack_with_and_without_packed_columns(G, dev, precision):
    """The whole SA stack with PACK_COLUMNS on and off: every output of every layer bit-identical."""
    from spsnet_amd import fused, pointnet2_modules as M, sa_stack, scenes
    layers = sa_stack.build_sa_layers(M, sa_stack.IASSD_KITTI, seed=4).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 16384, seed0=91, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)
    old, old_pack = fused.set_precision(precision), fused.PACK_COLUMNS
    try:
        with torch.no_grad():
            fused.PACK_COLUMNS = False
            a = sa_stack.run_sa_layers(layers, x, f)
            fused.PACK_COLUMNS = "always"
            b = sa_stack.run_sa_layers(layers, x, f)
            c = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
        for la, lb, lc in zip(a, b, c):
            for ta, tb, tc in zip(la, lb, lc):
                assert (ta is None and tb is None) or (torch.equal(ta, tb) and torch.equal(ta, tc))
    finally:
        fused.set_precision(old)
        fused.PACK_COLUMNS = old_pack


# ------------------------------------------------------------------ streamed layer: a wait that gives up is repaired, never returned
@pytest.mark.parametrize("npts,ns,half", [(None, None, False), ([2048, 512, 128], [(64, 64)] * 3, True)])
def test_streamed_first_layer_repairs_timed_out_waits(G, dev, npts, ns, half):
    """Every bounded progress wait is FORCED to give up at once (sps_debug_set_wait_spins): the chunk consumers then run on
    samples the FPS kernel has not written yet, and the predicated redo behind the producer must repair the layer -- every
    output of every layer bit-identical to the plain sequential pass, with the waits reported as timed out."""
    from spsnet_amd import _lib, pointnet2_modules as M, sa_stack, scenes
    L = _lib.load()
    N = 16384 if npts is None else 8192
    layers = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=npts, nsamples=ns), seed=6).to(dev)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, N, seed0=55, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats.astype(np.float16) if half else feats)
    with torch.no_grad():
        want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
        torch.cuda.synchronize()
        sa_stack.check_timeouts()
        old = L.sps_debug_set_wait_spins(0xFFFFFFFF)   # give up without looking: independent of the host's pace
        try:
            for rep in range(2):
                junk = torch.full((16 << 20,), 5 + rep, dtype=torch.int32, device=dev)   # stale memory = wrong but in-range values
                del junk
                got = sa_stack.run_sa_layers(layers, x, f)
                torch.cuda.synchronize()
                assert sa_stack.check_timeouts(), "the waits were supposed to give up"
                for k, (la, lb) in enumerate(zip(got, want)):
                    for ta, tb in zip(la, lb):
                        assert (ta is None and tb is None) or torch.equal(ta, tb), f"repetition {rep}, layer {k}"
        finally:
            L.sps_debug_set_wait_spins(old)
        got = sa_stack.run_sa_layers(layers, x, f)
        torch.cuda.synchronize()
        assert not sa_stack.check_timeouts()
        for la, lb in zip(got, want):
            for ta, tb in zip(la, lb):
                assert (ta is None and tb is None) or torch.equal(ta, tb)


# ------------------------------------------------------------------ staged grouping: rows over point ranges, staged packing, merged pooling
@pytest.mark.parametrize("B,N,M,k0,kc", [(2, 4096, 1024, 0, 2048), (2, 4096, 1024, 3072, 1024), (3, 1000, 256, 320, 37),
                                          (1, 8192, 512, 8000, 192), (2, 4096, 1024, 1024, 0)])
def test_ball_query_over_a_point_range(ext, G, oracle, B, N, M, k0, kc):
    """sps_ball_query_full2_points: both radii for all centroids over the points [k0, k0 + kc) only == the oracle's ball query
    of the sliced cloud (indices shifted back), -1 in every slot of a row without a hit; with the repair flag(s) up: the rows of
    the whole cloud (zeros for an empty ball, as always)."""
    rng = np.random.default_rng(B * N + k0)
    xyz = cloud(rng, B, N, dup=0.05)
    ctr = xyz[:, rng.permutation(N)[:M]].copy()
    ra, nsa, rb, nsb = 0.35, 16, 0.7, 32
    x, c = G.t(xyz), G.t(ctr)
    ia, ib = ext.ball_query_full2_points(ra, nsa, rb, nsb, x, c, k0, kc)
    for got, r, ns in ((ia, ra, nsa), (ib, rb, nsb)):
        want = np.full((B, M, ns), -1, np.int32)
        if kc > 0:
            sub = oracle.ball_query(r, ns, np.ascontiguousarray(xyz[:, k0:k0 + kc]), ctr)
            # the oracle leaves zeros for an empty ball, like the kernel; a non-empty row is shifted by k0
            empty = (sub == 0).all(-1) & ~_first_point_hit(xyz[:, k0:k0 + kc], ctr, r)
            want = np.where(empty[..., None], -1, sub + k0).astype(np.int32)
        np.testing.assert_array_equal(G.n(got), want)
    one = torch.ones((1,), dtype=torch.int32, device=x.device)
    flags = torch.zeros((B,), dtype=torch.int32, device=x.device)
    flags[B - 1] = 1
    for kw in (dict(full_if=one), dict(full_if_any=flags)):
        fa, fb = ext.ball_query_full2_points(ra, nsa, rb, nsb, x, c, k0, kc, **kw)
        np.testing.assert_array_equal(G.n(fa), oracle.ball_query(ra, nsa, xyz, ctr))
        np.testing.assert_array_equal(G.n(fb), oracle.ball_query(rb, nsb, xyz, ctr))


def _first_point_hit(pts, ctr, r):
    """(B, M) bool: is point 0 of `pts` inside the ball (fp32, the kernels' arithmetic is irrelevant at this margin)?"""
    d = pts[:, None, 0, :].astype(np.float64) - ctr.astype(np.float64)
    return (d ** 2).sum(-1) < float(np.float32(r) * np.float32(r)) * (1 - 1e-5)


@pytest.mark.parametrize("stages", [(1024,), (512, 1536), (256, 1024, 2048, 3072), (4095,)])
def test_staged_grouped_mlp_equals_one_launch(ext, G, dev, stages):
    """The grouped MLP of a layer computed in STAGES over growing point ranges -- rows over [k_i, k_i+1) from
    sps_ball_query_full2_points, sps_pack_columns2_late with the running per-centroid counts, pooled rows merged by atomic
    max -- against ONE launch over the complete rows: bit-identical pooled features for both scales; and with the repair
    flag up in the last stage (complete rows, plain stores) the same again, whatever the earlier stages left in `out`."""
    from spsnet_amd import fused, pointnet2_modules as M
    rng = np.random.default_rng(len(stages) * 100 + stages[0])
    B, N, Mc, cf = 2, 4096, 512, 64
    xyz = cloud(rng, B, N, dup=0.02)
    x = G.t(xyz)
    new_xyz = x[:, :Mc].contiguous()             # centroids are points of the cloud (every first-stage row holds itself)
    feats = fused.attach_point_major_twin(torch.randn(B, cf, N, device=dev))
    old = fused.set_precision("fp32")
    try:
        mod = M.PointnetSAModuleMSG_WithSampling(
            npoint_list=[Mc], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.4, 0.8], nsamples=[16, 32],
            mlps=[[cf, 64, 64, 128], [cf, 64, 96, 128]], use_xyz=True, dilated_group=False, aggregation_mlp=None,
            confidence_mlp=None, num_class=3).to(dev).eval()
        with torch.no_grad():
            plan = mod._fused_plan(x, new_xyz, feats)
            assert plan and all(p.split == 0 and p.point_major for p in plan)
            ga, gb = mod.groupers
            width = sum(p.c3_real for p in plan)
            ia, ib = ext.ball_query_full2(ga.radius, ga.nsample, gb.radius, gb.nsample, x, new_xyz)
            ca, cb = fused.pack_columns2(ia, ib)
            want = torch.empty((B, Mc, width), device=dev)
            mod._run_scales(x, new_xyz, feats, (ia, ib), plan, want, [ca, cb], True)
            for repair in (False, True):
                out = torch.zeros((B, Mc, width), device=dev) if not repair else torch.full((B, Mc, width), 7.25, device=dev)
                flag = torch.full((1,), int(repair), dtype=torch.int32, device=dev)
                prev, k0 = None, 0
                for i, k1 in enumerate(tuple(stages) + (N,)):
                    last = k1 == N
                    kw = dict(full_if=flag) if last else {}
                    sa, sb = ext.ball_query_full2_points(ga.radius, ga.nsample, gb.radius, gb.nsample, x, new_xyz, k0, k1 - k0, **kw)
                    pa, pb, prev = fused.pack_columns2_staged(sa, sb, last, prev=prev, **kw)
                    mkw = {} if i == 0 else (dict(merge=True, full_range_if=flag) if last else dict(merge=True))
                    mod._run_scales(x, new_xyz, feats, (sa, sb), plan, out, [pa, pb], True, **mkw)
                    k0 = k1
                torch.cuda.synchronize()
                assert torch.equal(out, want), f"repair={repair}"
    finally:
        fused.set_precision(old)


# ------------------------------------------------------------------ exact fp32: the next layer starts on the early picks
@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
@pytest.mark.parametrize("case", ["plain", "waits-give-up", "prefix-guess-fails"])
def test_streamed_first_layer_early_pool(G, dev, case, precision, monkeypatch):
    """Both arithmetics (strict fp32: the point-major kernel; split-fp16: the per-wave kernel with its weights in LDS): behind the chunks that end at 6/16, 9/16 and 12/16 of layer 0's picks, layer 1 queries the centroids that
    exist and runs the grouped MLP of the columns they give (begin_early_pool, three stages); behind the last pick it adds the
    last quarter's columns by an atomic max.  Against the plain sequential pass: every output of every layer bit-identical, twice, allocator poisoned --
    also when every bounded wait is forced to give up (the late launches then redo layer 1 from scratch on the repaired
    layer 0) and on a lattice cloud whose exact distance ties break the identity-prefix guess of layer 1's D-FPS (flagged
    scenes: the same redo, on the centroids the real D-FPS picks)."""
    from spsnet_amd import _lib, fused, pointnet2_modules as M, sa_stack, scenes
    L = _lib.load()
    layers = sa_stack.build_sa_layers(M, sa_stack.IASSD_KITTI, seed=21).to(dev)
    if case == "prefix-guess-fails":
        rng = np.random.default_rng(77)
        xyz = cloud(rng, 2, 16384, lattice=True) * 4.0 + rng.integers(0, 2, (2, 16384, 3)).astype(np.float32) * 0.5
        feats = rng.uniform(0, 1, (2, 1, 16384)).astype(np.float32)
    else:
        xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 16384, seed0=71, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)
    monkeypatch.setattr(fused, "PACK_PM32_MIN_COLUMNS", 1024)     # (two scenes: below the size where packing pays)
    began = []
    orig = M.PointnetSAModuleMSG_WithSampling.begin_early_pool
    monkeypatch.setattr(M.PointnetSAModuleMSG_WithSampling, "begin_early_pool",
                        lambda self, *a, **k: began.append(orig(self, *a, **k)) or began[-1])
    old = fused.set_precision(precision)
    old_spins = L.sps_debug_set_wait_spins(0xFFFFFFFF) if case == "waits-give-up" else None
    try:
        with torch.no_grad():
            if old_spins is not None:
                L.sps_debug_set_wait_spins(old_spins)
            want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
            torch.cuda.synchronize()
            sa_stack.check_timeouts()
            if case == "waits-give-up":
                L.sps_debug_set_wait_spins(0xFFFFFFFF)
            for rep in range(2):
                junk_i = torch.full((32 << 20,), 3 + rep, dtype=torch.int32, device=dev)
                junk_f = torch.full((32 << 20,), 1.5 + rep, dtype=torch.float32, device=dev)
                del junk_i, junk_f
                got = sa_stack.run_sa_layers(layers, x, f)
                torch.cuda.synchronize()
                assert sa_stack.check_timeouts() == (case == "waits-give-up")
                for k, (la, lb) in enumerate(zip(got, want)):
                    for ta, tb in zip(la, lb):
                        assert (ta is None and tb is None) or torch.equal(ta, tb), f"repetition {rep}, layer {k}"
    finally:
        fused.set_precision(old)
        if case == "waits-give-up":
            L.sps_debug_set_wait_spins(old_spins)
    assert len(began) == 2 * len(sa_stack.EARLY_POOL_AT_16) and all(began), "layer 1 was supposed to start on the early picks"
    if case == "prefix-guess-fails":
        idx1 = got[1][3]
        assert not torch.equal(idx1, torch.arange(idx1.shape[1], device=dev, dtype=idx1.dtype).expand_as(idx1)), \
            "the lattice cloud was supposed to break the identity-prefix guess"


# ------------------------------------------------------------------ training: layer 0's ball queries beside its FPS
@pytest.mark.parametrize("force_timeouts", [False, True])
def test_training_streamed_queries_equal_unstreamed(G, dev, force_timeouts, monkeypatch):
    """A TRAINING pass (BatchNorm on batch statistics, gradients) with layer 0's ball queries consuming the publishing FPS
    chunk by chunk (sa_stack._streamed_first_layer_queries) against the same pass with every query behind the FPS: every
    output and every running statistic bit-identical, every parameter gradient within 1e-5 -- also when each bounded progress
    wait is forced to give up (the last chunk's query then repairs the whole layer)."""
    import copy
    from spsnet_amd import _lib, pointnet2_modules as M, sa_stack, scenes
    L = _lib.load()
    base = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=[1024, 256, 128]), seed=9).to(dev).train()
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=77, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)

    def run(layers, streamed):
        monkeypatch.setattr(sa_stack, "STREAM_TRAINING_QUERIES", streamed)
        outs = sa_stack.run_sa_layers(layers, x, f)
        loss = sum(o[1].square().mean() for o in outs) + sum(o[2].square().mean() for o in outs if o[2] is not None)
        loss.backward()
        torch.cuda.synchronize()
        return outs

    ref_layers, got_layers = copy.deepcopy(base), copy.deepcopy(base)
    want = run(ref_layers, False)
    sa_stack.check_timeouts()
    old = L.sps_debug_set_wait_spins(0xFFFFFFFF) if force_timeouts else None
    try:
        calls = []
        orig = sa_stack._streamed_first_layer_queries
        monkeypatch.setattr(sa_stack, "_streamed_first_layer_queries", lambda *a: calls.append(orig(*a)) or calls[-1])
        got = run(got_layers, True)
        assert calls == [True], "layer 0 was supposed to qualify for the streamed queries"
        assert bool(sa_stack.check_timeouts()) == force_timeouts
    finally:
        if old is not None:
            L.sps_debug_set_wait_spins(old)
    for k, (la, lb) in enumerate(zip(got, want)):
        for ta, tb in zip(la, lb):
            assert (ta is None and tb is None) or torch.equal(ta, tb), f"layer {k}"
    # (gradients: the grouping backward adds with LDS atomics, whose order is not fixed from run to run)
    for (name, pa), (_, pb) in zip(got_layers.named_parameters(), ref_layers.named_parameters()):
        if pa.grad is None and pb.grad is None:
            continue
        err = float((pa.grad - pb.grad).abs().max())
        assert err <= 1e-5 * max(1.0, float(pb.grad.abs().max())), (name, err)
    for (name, ba), (_, bb) in zip(got_layers.named_buffers(), ref_layers.named_buffers()):
        assert torch.equal(ba, bb), name


@pytest.mark.parametrize("C,use_xyz", [(0, True), (5, True), (20, False)])
def test_group_concat_matches_query_and_group(ext, G, C, use_xyz):
    """sps_group_concat on the rows of a ball query == the fused sps_query_and_group (which is pinned to the oracle)."""
    rng = np.random.default_rng(C)
    xyz = rng.uniform(-2, 2, (2, 3000, 3)).astype(np.float32)
    new_xyz = xyz[:, rng.integers(0, 3000, 200)].copy()
    feats = rng.normal(size=(2, C, 3000)).astype(np.float32) if C else None
    want, idx = ext.query_and_group(0.7, 16, G.t(xyz), G.t(new_xyz), None if feats is None else G.t(feats), use_xyz)
    got = ext.group_concat(G.t(xyz), G.t(new_xyz), None if feats is None else G.t(feats), idx, use_xyz)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ the fused train-mode grouped MLP (csrc/mlp_train.hip)
@pytest.mark.parametrize("B,M,ns,widths", [(2, 128, 16, [7, 24, 40, 72]), (2, 64, 32, [131, 128, 256, 256]),
                                           (3, 40, 8, [4, 16, 32]), (1, 16, 4, [19]), (2, 32, 64, [67, 64, 96, 128]),
                                           (2, 48, 16, [259, 256, 200]), (2, 24, 8, [20, 48, 40]), (1, 8, 8, [5, 16, 16, 16]),
                                           # IA-SSD layer 5 (IA-SSD.yaml:35-55): K slabs in the convolutions, 256 x 256 blocks of dW
                                           (2, 32, 16, [259, 256, 256, 512]), (2, 16, 32, [259, 256, 512, 1024]),
                                           (1, 8, 8, [300, 520, 70]), (1, 8, 8, [2100, 16])])
@pytest.mark.parametrize("one_call", [True, False], ids=["one-c-call", "launch-by-launch"])
@BOTH_TRAIN_PRECISIONS
def test_fused_train_mode_mlp_matches_torch(dev, B, M, ns, widths, one_call, train_precision, monkeypatch):
    """_GroupedMLPPoolTrain (conv + batch statistics in the epilogue, BatchNorm / ReLU / pool routing / BatchNorm backward
    in the operand loads, split-fp16 MFMA) against the plain torch op sequence of the reference (pointnet2_modules.py:432-444)
    in float64 on the CPU: pooled output, running statistics, and the gradients w.r.t. the grouped input and every
    parameter, at 2e-4 of the largest reference magnitude (the op-by-op GPU path is held to the same bar).  Shapes cover
    channel counts that are not multiples of 16 / 32, more than 128 output rows (two row chunks), one to three layers,
    every supported nsample, column counts that are odd multiples of 64 (the narrower weight-gradient stage) or a single
    64-column block, widths of 257 .. 1024 on either side of a layer (K slabs of 256 input rows in sps_tconv, every slab behind
    the first accumulating into the output; 256 x 256 blocks of the weight gradient in sps_twgrad; channel counts that are
    no multiple of the slab), and a width beyond 2048 (declined: falls back to the op-by-op path)."""
    import copy
    from spsnet_amd import fused, pointnet2_modules as PM
    torch.manual_seed(B * 1000 + M + ns)
    c0 = widths[0] if len(widths) > 1 else 5
    chain = widths if len(widths) > 1 else [5] + widths
    mlp = PM._conv_bn_relu_stack(list(chain), torch.nn.Conv2d, torch.nn.BatchNorm2d)
    for mod in mlp:
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5).mul_(torch.where(torch.rand_like(mod.weight) < 0.2, -1.0, 1.0))
            mod.bias.data.normal_(0, 0.3)
            mod.running_mean.normal_()
            mod.running_var.uniform_(0.5, 2.0)
    ref = copy.deepcopy(mlp).double().train()
    mlp = mlp.to(dev).train()
    x0 = torch.randn(B, c0, M, ns)
    wout = torch.randn(B, chain[-1], M)

    xr = x0.double().requires_grad_(True)
    out_r = ref(xr).max(dim=3)[0]
    (out_r * wout.double()).sum().backward()

    xg = x0.to(dev).requires_grad_(True)
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    # both host forms of the same kernels: one C call per stack (sps_mlp_train_forward / _backward, the default) and the
    # launch-by-launch form SyncBatchNorm and SPS_ONE_CALL_TRAINING=0 use
    monkeypatch.setattr(PM, "ONE_CALL_TRAINING", one_call)
    got = PM._fused_mlp_pool_train(mlp, xg, 'max_pool')
    if max(chain) > 2048:
        assert got is None
        return
    assert got is not None, "the stack was supposed to qualify"
    (got * wout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert not fused.check_overflow()

    def close(a, b, what, tol=2e-4):
        a, b = a.detach().cpu().double(), b.detach()
        assert a.shape == b.shape, what
        err = float((a - b).abs().max())
        assert err <= tol * max(1.0, float(b.abs().max())), (what, err, float(b.abs().max()))

    close(got, out_r, "pooled")
    close(xg.grad, xr.grad, "d/d input")
    for (name, pg), (_, pr) in zip(mlp.named_parameters(), ref.named_parameters()):
        close(pg.grad, pr.grad, "d/d " + name)
    for (name, bg), (_, br) in zip(mlp.named_buffers(), ref.named_buffers()):
        if bg.dtype.is_floating_point:
            close(bg, br, "buffer " + name)
        else:
            assert int(bg) == int(br), name


@SPLIT_FP16_TRAINING
def test_fused_train_mode_mlp_poisons_unrepresentable_operands(dev, train_precision, monkeypatch):
    """An operand beyond the split-fp16 range is never clamped silently: the outputs that depend on it are NaN and the overflow
    flag is raised.  (Exact fp32, the default, has no such range: test_fused_train_mode_mlp_large_operands_in_fp32.)"""
    from spsnet_amd import fused, pointnet2_modules as PM
    torch.manual_seed(0)
    mlp = PM._conv_bn_relu_stack([4, 16, 32], torch.nn.Conv2d, torch.nn.BatchNorm2d).to(dev).train()
    x = torch.randn(2, 4, 32, 16, device=dev)
    x[1, 2, 5, 3] = 1e6
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    fused.check_overflow()
    out = PM._fused_mlp_pool_train(mlp, x.requires_grad_(True), 'max_pool')
    torch.cuda.synchronize()
    assert out is not None and bool(torch.isnan(out).any())
    assert fused.check_overflow()


def test_fused_train_mode_mlp_large_operands_in_fp32(dev, monkeypatch):
    """Exact fp32 (the default training arithmetic): an operand of 1e6 -- beyond what the split form can carry -- is just a
    number: finite outputs within 2e-4 of float64 torch, no overflow flag."""
    import copy
    from spsnet_amd import fused, pointnet2_modules as PM
    assert fused.TRAIN_PRECISION == "fp32", "the library default is the reference's arithmetic"
    torch.manual_seed(0)
    mlp = PM._conv_bn_relu_stack([4, 16, 32], torch.nn.Conv2d, torch.nn.BatchNorm2d)
    ref = copy.deepcopy(mlp).double().train()
    mlp = mlp.to(dev).train()
    x = torch.randn(2, 4, 32, 16)
    x[1, 2, 5, 3] = 1e6
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    fused.check_overflow()
    out = PM._fused_mlp_pool_train(mlp, x.to(dev).requires_grad_(True), 'max_pool')
    want = ref(x.double()).max(dim=3)[0]
    torch.cuda.synchronize()
    assert out is not None and bool(torch.isfinite(out).all()) and not fused.check_overflow()
    assert float((out.cpu().double() - want).abs().max()) <= 2e-4 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("B,M,widths,tailconv", [(2, 256, [96, 64], False), (3, 128, [256, 128, 128], True), (2, 64, [40, 24], True),
                                                 (2, 64, [1536, 512], False)])     # (IA-SSD layer 5's aggregation stack)
@pytest.mark.parametrize("one_call", [True, False], ids=["one-c-call", "launch-by-launch"])
@BOTH_TRAIN_PRECISIONS
def test_fused_train_mode_pointwise_stack_matches_torch(dev, B, M, widths, tailconv, one_call, train_precision, monkeypatch):
    """The aggregation / confidence stacks ([Conv1d, BatchNorm1d, ReLU] x n, optionally a class-score Conv1d with bias behind
    them) in train() mode through _pointwise_stack (fused kernels, no pool) against float64 torch: output, running statistics
    and every gradient."""
    import copy
    from spsnet_amd import fused, pointnet2_modules as PM
    torch.manual_seed(M + len(widths))
    mods = list(PM._conv_bn_relu_stack(list(widths), torch.nn.Conv1d, torch.nn.BatchNorm1d))
    if tailconv:
        mods.append(torch.nn.Conv1d(widths[-1], 3, kernel_size=1, bias=True))
    stack = torch.nn.Sequential(*mods)
    for mod in stack:
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    ref = copy.deepcopy(stack).double().train()
    stack = stack.to(dev).train()
    x0 = torch.randn(B, widths[0], M).abs() * 2 + 0.1          # post-ReLU-like inputs
    cout = 3 if tailconv else widths[-1]
    wout = torch.randn(B, cout, M) * 1e-4                       # small gradients, as a mean-reduced loss produces them
    xr = x0.double().requires_grad_(True)
    out_r = ref(xr)
    (out_r * wout.double()).sum().backward()
    xg = x0.to(dev).requires_grad_(True)
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    monkeypatch.setattr(PM, "ONE_CALL_TRAINING", one_call)
    monkeypatch.setattr(PM, "FUSED_POINTWISE_TRAINING", True)
    calls = []
    orig = PM._fused_stack_train
    monkeypatch.setattr(PM, "_fused_stack_train", lambda *a: calls.append(orig(*a)) or calls[-1])
    got = PM._pointwise_stack(stack, xg)
    assert len(calls) == 1 and calls[0] is not None, "the stack was supposed to take the fused kernels"
    (got * wout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert not fused.check_overflow()

    def close(a, b, what, tol=2e-5):
        a, b = a.detach().cpu().double(), b.detach()
        assert a.shape == b.shape, what
        err = float((a - b).abs().max())
        assert err <= tol * max(1e-30, float(b.abs().max())), (what, err, float(b.abs().max()))

    close(got, out_r, "output")
    close(xg.grad, xr.grad, "d/d input")
    for (name, pg), (_, pr) in zip(stack.named_parameters(), ref.named_parameters()):
        close(pg.grad, pr.grad, "d/d " + name)
    for (name, bg), (_, br) in zip(stack.named_buffers(), ref.named_buffers()):
        if bg.dtype.is_floating_point:
            close(bg, br, "buffer " + name)
        else:
            assert int(bg) == int(br), name


@pytest.mark.parametrize("B,N,M,ns,C,use_xyz,new_grad", [(2, 3000, 256, 16, 24, True, False), (3, 1024, 100, 32, 7, True, True),
                                                         (1, 20000, 64, 8, 40, False, False), (2, 500, 33, 5, 3, True, True)])
def test_group_concat_with_gradients_matches_op_sequence(G, dev, B, N, M, ns, C, use_xyz, new_grad, monkeypatch):
    """group_with_index when gradients are wanted (_GroupConcat: one launch forward, the feature gradient scattered straight
    from the wide gradient tensor by sps_group_points_grad_strided) against the differentiable op sequence it replaces
    (grouping_operation x 2, subtract, cat: pointnet2_utils.py:312-320 of the reference): values bit-identical, gradients
    of the features and of new_xyz within fp32 summation order; covers the LDS and the global-atomic scatter kernels."""
    from spsnet_amd import pointnet2_utils as U
    gen = torch.Generator().manual_seed(N + M)
    xyz = (torch.rand(B, N, 3, generator=gen) * 10).to(dev)
    idx = torch.randint(0, N, (B, M, ns), generator=gen, dtype=torch.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]                      # padded balls repeat their first hit
    idx = idx.to(dev)
    feats0 = torch.randn(B, C, N, generator=gen)
    new0 = torch.rand(B, M, 3, generator=gen) * 10
    wout = torch.randn(B, C + (3 if use_xyz else 0), M, ns, generator=gen).to(dev)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(U, "GROUP_CONCAT_TRAINING", flag)
        f = feats0.to(dev).requires_grad_(True)
        q = new0.to(dev).requires_grad_(new_grad)
        out = U.group_with_index(xyz, q, f, idx, use_xyz)
        assert (type(out.grad_fn).__name__ == "_GroupConcatBackward") == flag
        (out * wout).sum().backward()
        res[flag] = (out.detach(), f.grad, q.grad)
    assert torch.equal(res[True][0], res[False][0])
    for a, b, what in ((res[True][1], res[False][1], "features"), (res[True][2], res[False][2], "new_xyz")):
        if b is None:
            assert a is None, what
            continue
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), what
    # deterministic mode and a cloud that wants gradients itself keep the op sequence
    monkeypatch.setattr(U, "GROUP_CONCAT_TRAINING", True)
    monkeypatch.setattr(U, "DETERMINISTIC_BACKWARD", True)
    out = U.group_with_index(xyz, new0.to(dev), feats0.to(dev).requires_grad_(True), idx, use_xyz)
    assert type(out.grad_fn).__name__ != "_GroupConcatBackward"
    monkeypatch.setattr(U, "DETERMINISTIC_BACKWARD", False)
    out = U.group_with_index(xyz.clone().requires_grad_(True), new0.to(dev), feats0.to(dev), idx, use_xyz)
    assert type(out.grad_fn).__name__ != "_GroupConcatBackward"


def test_training_prefetched_first_layer_equals_plain(G, dev):
    """sa_stack.prefetch_first_layer: layer 0's FPS and ball queries of the NEXT batch started before the current step's
    backward (on a side stream, beside it) -- every output and running statistic of the next forward bit-identical to a
    forward that samples by itself, gradients within 1e-5; the prefetch is consumed exactly once and a forward over a
    DIFFERENT tensor ignores it."""
    import copy
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    base = sa_stack.build_sa_layers(M, sa_stack.scaled_config(npoints=[1024, 256, 128]), seed=11).to(dev).train()
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=5, dup_fraction=0.01)
    x, f = G.t(xyz), G.t(feats)

    def loss_of(outs):
        return sum(o[1].square().mean() for o in outs) + sum(o[2].square().mean() for o in outs if o[2] is not None)

    ref, got = copy.deepcopy(base), copy.deepcopy(base)
    for _ in range(2):                                   # two plain steps
        want = sa_stack.run_sa_layers(ref, x, f)
        loss_of(want).backward()
    outs = sa_stack.run_sa_layers(got, x, f)             # step 1, with the next batch (the same tensor) prefetched
    loss = loss_of(outs)
    assert sa_stack.prefetch_first_layer(got, x)
    loss.backward()
    calls = []
    orig = sa_stack._streamed_first_layer_queries
    sa_stack._streamed_first_layer_queries = lambda *a: calls.append(1) or orig(*a)
    try:
        outs = sa_stack.run_sa_layers(got, x, f)         # step 2 picks the prefetch up
        assert calls == [], "the prefetched sampling was supposed to be used"
        loss_of(outs).backward()
        torch.cuda.synchronize()
        for k, (la, lb) in enumerate(zip(outs, want)):
            for ta, tb in zip(la, lb):
                assert (ta is None and tb is None) or torch.equal(ta, tb), f"layer {k}"
        for (name, pa), (_, pb) in zip(got.named_parameters(), ref.named_parameters()):
            if pa.grad is not None:
                err = float((pa.grad - pb.grad).abs().max())
                assert err <= 1e-5 * max(1.0, float(pb.grad.abs().max())), (name, err)
        for (name, ba), (_, bb) in zip(got.named_buffers(), ref.named_buffers()):
            assert torch.equal(ba, bb), name
        # a prefetch for one tensor, a forward over another: ignored (and the layer samples by itself)
        assert sa_stack.prefetch_first_layer(got, x)
        x2 = x.clone()
        sa_stack.run_sa_layers(got, x2, f)
        assert calls == [1, 1], "one call by the prefetch, one by the forward over the other tensor"
        torch.cuda.synchronize()
        assert not sa_stack.check_timeouts()
    finally:
        sa_stack._streamed_first_layer_queries = orig


def test_backbone_prefetch_sampling_equals_plain(G, dev):
    """IASSD_Backbone.prefetch_sampling(next batch) + forward over the same `points` tensor == a plain training forward
    (the picked-up FPS / ball queries are the same kernels' results): every tensor of the output dict bit-identical."""
    import copy
    from spsnet_amd import backbones as BB, scenes
    net = scenes.fill_parameters(BB.IASSD_Backbone(BB.scaled_cfg(BB.IASSD_KITTI_CFG, [1024, 256, 128, 64, -1, 64]), num_class=3,
                                                   input_channels=4), 3).to(dev).train()
    twin = copy.deepcopy(net)
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=9)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 8192)[:, None]
    points = G.t(np.concatenate([bidx, xyz.reshape(-1, 3), feats.transpose(0, 2, 1).reshape(-1, 1)], 1).astype(np.float32))
    want = twin(dict(batch_size=2, points=points))
    assert net.prefetch_sampling(dict(batch_size=2, points=points))
    got = net(dict(batch_size=2, points=points))
    torch.cuda.synchronize()
    assert net.SA_modules[0]._presampled is None, "the prefetch was supposed to be consumed"
    for key, w in want.items():
        g = got[key]
        if isinstance(w, torch.Tensor):
            assert torch.equal(g, w), key
        elif isinstance(w, (list, tuple)):
            for a, b in zip(g, w):
                if isinstance(b, torch.Tensor):
                    assert torch.equal(a, b), key


@pytest.mark.parametrize("gscale", [1e-12, 1e-4, 1e4])
@BOTH_TRAIN_PRECISIONS
def test_fused_train_mode_mlp_gradient_scale_invariance(dev, gscale, train_precision, monkeypatch):
    """The fp16 halves of the gradient operands carry an exact power-of-two scale (csrc/mlp_train.hip), so the accuracy of the
    backward must not depend on the magnitude of the incoming gradient: 1e-12 .. 1e4 against float64 torch, every gradient
    within 2e-5 of its own largest entry.  (Unscaled, gradients below ~1e-3 lose their low halves to fp16 denormals.)
    Also: a frozen convolution weight gets no gradient, an input that does not require one neither, a zero BatchNorm weight
    yields finite gradients."""
    import copy
    from spsnet_amd import fused, pointnet2_modules as PM
    torch.manual_seed(3)
    mlp = PM._conv_bn_relu_stack([19, 48, 64, 96], torch.nn.Conv2d, torch.nn.BatchNorm2d)
    mlp[4].weight.data[5] = 0.0                          # a dead channel of the second BatchNorm
    mlp[3].weight.requires_grad_(False)                  # a frozen convolution
    ref = copy.deepcopy(mlp).double().train()
    mlp = mlp.to(dev).train()
    x0 = torch.randn(2, 19, 64, 16).abs() + 0.2
    wout = torch.randn(2, 96, 64) * gscale
    xr = x0.double().requires_grad_(True)
    (ref(xr).max(dim=3)[0] * wout.double()).sum().backward()
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    for needs_dx in (True, False):
        for p in mlp.parameters():
            p.grad = None
        xg = x0.to(dev).requires_grad_(needs_dx)
        out = PM._fused_mlp_pool_train(mlp, xg, 'max_pool')
        assert out is not None
        (out * wout.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert not fused.check_overflow()
        assert mlp[3].weight.grad is None and (xg.grad is not None) == needs_dx
        pairs = [(p.grad, q.grad, n) for (n, p), (_, q) in zip(mlp.named_parameters(), ref.named_parameters()) if q.grad is not None]
        if needs_dx:
            pairs.append((xg.grad, xr.grad, "input"))
        for g, w, name in pairs:
            assert torch.isfinite(g).all(), name
            err = float((g.cpu().double() - w).abs().max())
            assert err <= 2e-5 * float(w.abs().max()) + 1e-300, (name, err, float(w.abs().max()))


@BOTH_TRAIN_PRECISIONS
def test_fused_train_mode_mlp_nan_input_propagates(dev, train_precision, monkeypatch):
    """A NaN in the grouped input reaches the pooled outputs that depend on it (as through torch's Conv / BatchNorm / ReLU /
    max_pool2d, where it reaches all of them via the batch statistics); nothing is clamped.  The split form also raises its
    overflow flag; exact fp32 has no flag to raise -- the NaN is the report."""
    from spsnet_amd import fused, pointnet2_modules as PM
    torch.manual_seed(0)
    mlp = PM._conv_bn_relu_stack([4, 16, 32], torch.nn.Conv2d, torch.nn.BatchNorm2d).to(dev).train()
    x = torch.randn(2, 4, 32, 16, device=dev)
    x[0, 1, 7, 2] = float("nan")
    monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
    fused.check_overflow()
    out = PM._fused_mlp_pool_train(mlp, x.requires_grad_(True), 'max_pool')
    torch.cuda.synchronize()
    assert out is not None and bool(torch.isnan(out).any())
    assert fused.check_overflow() == (train_precision == "fp16x2")


@pytest.mark.parametrize("mode", ["inference", "gradients", "train"])
def test_golden_pointnet2msg_backbone(G, dev, mode):
    """PointNet2MSG (PointRCNN's backbone: four MSG SA layers + four feature-propagation layers,
    pointnet2_backbone.py:9-100) on 2 x 4096 points at the shipped widths against the reference's own forward run over the
    C oracle (oracle/gen_golden.py:pointnet2msg): per-point features to 1e-4, point coordinates exact.  `inference` = the
    fused kernels with the next layer's D-FPS started early as a verified identity prefix, `gradients` = the reference's
    op order with autograd (eval-mode BatchNorm); `train` only checks that a training step runs and yields finite
    gradients (batch statistics: no golden)."""
    import copy
    from spsnet_amd import backbones as BB, scenes
    g = np.load(os.path.join(GOLD, "backbone_pointnet2msg.npz"))
    cfg = copy.deepcopy(BB.POINTRCNN_KITTI_CFG)
    cfg['SA_CONFIG']['NPOINTS'] = [int(v) for v in g["npoints"]]
    net = BB.PointNet2MSG(cfg, input_channels=4)
    assert net.num_point_features == int(g["num_point_features"]) and len(net.state_dict()) == int(g["n_state"])
    scenes.fill_parameters(net, int(g["seed"]))
    net = net.to(dev)
    batch = dict(batch_size=2, points=G.t(g["points"]))
    if mode == "train":
        out = net.train()(batch)
        out["point_features"].square().mean().backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        assert len(grads) > 60 and all(torch.isfinite(x).all() for x in grads)
        return
    net.eval()
    if mode == "inference":
        with torch.no_grad():
            out = net(batch)
    else:
        out = net(batch)
        assert out["point_features"].requires_grad
    want = g["point_features"]
    got = G.n(out["point_features"])
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= 1e-4 * max(1.0, float(np.abs(want).max()))
    np.testing.assert_array_equal(G.n(out["point_coords"]), g["point_coords"])


def test_pointnet2msg_streamed_first_layer_equals_sequential(G, dev, monkeypatch):
    """PointNet2MSG inference with layer 0 streamed against its own FPS (and layer 1's D-FPS taken from the verified identity
    prefix) == the same forward layer by layer: per-point features bit-identical, no bounded wait gave up."""
    import copy
    from spsnet_amd import backbones as BB, sa_stack, scenes
    cfg = copy.deepcopy(BB.POINTRCNN_KITTI_CFG)
    cfg['SA_CONFIG']['NPOINTS'] = [1024, 256, 64, 16]
    net = scenes.fill_parameters(BB.PointNet2MSG(cfg, input_channels=4), 4).to(dev).eval()
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 8192, seed0=13, dup_fraction=0.01)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 8192)[:, None]
    points = G.t(np.concatenate([bidx, xyz.reshape(-1, 3), feats.transpose(0, 2, 1).reshape(-1, 1)], 1).astype(np.float32))
    calls = []
    orig = sa_stack._streamed_first_layer
    monkeypatch.setattr(sa_stack, "_streamed_first_layer", lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1])
    with torch.no_grad():
        monkeypatch.setattr(BB, "STREAM_FIRST_LAYER", False)
        want = net(dict(batch_size=2, points=points))["point_features"].clone()
        assert calls == []
        monkeypatch.setattr(BB, "STREAM_FIRST_LAYER", True)
        got = net(dict(batch_size=2, points=points))["point_features"]
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0] is not None, "layer 0 was supposed to be streamed"
    assert not sa_stack.check_timeouts()
    assert torch.equal(got, want)


@pytest.mark.parametrize("n,m,c_known,c_skip,widths", [(64, 16, 32, 16, [48, 32]), (256, 77, 20, 0, [64]), (1024, 256, 256, 1, [128, 128]),
                                                       (48, 9, 100, 37, [16, 512]), (32, 5, 512, 512, [256, 256]), (1000, 300, 64, 3, [32, 32]),
                                                       (7, 4, 16, 0, [16])])
def test_fp_module_fused_kernel_matches_op_sequence(dev, n, m, c_known, c_skip, widths):
    """PointnetFPModule in inference: the one-kernel form (three_interpolate + cat + [Conv2d + BatchNorm2d + ReLU] x (1 | 2),
    csrc/pw_mlp.hip fp_mlp_kernel) against the module's own op sequence with gradients enabled (the unfused kernels, pinned
    by the reference-generated fp_module golden): 1e-4.  No skip features, one layer, channel counts that are not multiples
    of 16 and 1024 input channels included."""
    from spsnet_amd import fused, pointnet2_modules as M, scenes
    torch.manual_seed(n + c_known)
    fp = scenes.fill_parameters(M.PointnetFPModule(mlp=[c_known + c_skip] + widths), 3).to(dev).eval()
    unknown = torch.rand(2, n, 3, device=dev) * 4
    known = torch.rand(2, m, 3, device=dev) * 4
    kf = torch.randn(2, c_known, m, device=dev)
    uf = torch.randn(2, c_skip, n, device=dev) if c_skip else None
    calls = []
    orig = fused.fp_module_mlp
    fused.fp_module_mlp = lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1]
    try:
        with torch.no_grad():
            got = fp(unknown, known, uf, kf)
            rows = fp(unknown, known, uf, kf, point_major_ok=True)
        assert len(calls) == 2 and calls[0] is not None and calls[1] is not None, "the fused kernel was supposed to serve this shape"
        want = fp(unknown, known, uf, kf.clone().requires_grad_(True), point_major_ok=True)      # gradients wanted: the op sequence
        assert len(calls) == 3 and calls[2] is None and not getattr(want, "_sps_point_major", False)
    finally:
        fused.fp_module_mlp = orig
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    # per-point rows straight from the kernel: the same numbers, transposed
    assert getattr(rows, "_sps_point_major", False) and rows.shape == (2, n, widths[-1]) and rows.is_contiguous()
    assert torch.equal(rows.transpose(1, 2), got)
    # the weights formed inside the kernel from three_nn's distances against the module's three torch ops
    from spsnet_amd import pointnet2_utils as U
    with torch.no_grad():
        dist, idx = U.three_nn(unknown, known)
        inv = 1.0 / (dist + 1e-8)
        weight = inv / torch.sum(inv, dim=2, keepdim=True)
        given = fused.fp_module_mlp(fp.mlp, kf, uf, idx, weight)
    assert float((given - got).abs().max()) <= 2e-6 * max(1.0, float(got.abs().max()))


@BOTH_TRAIN_PRECISIONS
def test_fp_module_training_on_fused_kernels_matches_torch(dev, train_precision, monkeypatch):
    """PointnetFPModule in train() mode with its [Conv2d 1x1, BatchNorm2d, ReLU] stack on the fused train-mode kernels
    (no pool) against the module's plain torch op sequence: output, running statistics and every gradient (incl. the
    gradient that flows back through the interpolation into the coarse features)."""
    import copy
    from spsnet_amd import pointnet2_modules as M, scenes
    torch.manual_seed(5)
    fp = scenes.fill_parameters(M.PointnetFPModule(mlp=[40 + 9, 64, 32]), 2).to(dev).train()
    ref = copy.deepcopy(fp)
    unknown = torch.rand(2, 2048, 3, device=dev) * 4
    known = torch.rand(2, 256, 3, device=dev) * 4
    kf0 = torch.randn(2, 40, 256, device=dev)
    uf0 = torch.randn(2, 9, 2048, device=dev)
    wout = torch.randn(2, 32, 2048, device=dev) * 1e-3
    res = []
    for mod, fused_on in ((fp, True), (ref, False)):
        monkeypatch.setattr(M, "FUSED_FP_TRAINING_MIN", 0 if fused_on else 1 << 62)
        calls = []
        orig = M._fused_stack_train
        monkeypatch.setattr(M, "_fused_stack_train", lambda *a: calls.append(orig(*a)) or calls[-1])
        kf, uf = kf0.clone().requires_grad_(True), uf0.clone().requires_grad_(True)
        out = mod(unknown, known, uf, kf)
        (out * wout).sum().backward()
        monkeypatch.setattr(M, "_fused_stack_train", orig)
        assert (len(calls) == 1 and calls[0] is not None) == fused_on
        res.append([out.detach(), kf.grad, uf.grad] + [p.grad for p in mod.parameters()] + [b.detach().float() for b in mod.buffers()])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        err = float((a - b).abs().max())
        assert err <= 2e-5 * max(1e-30, float(b.abs().max())) + 1e-12, (err, float(b.abs().max()))


@pytest.mark.parametrize("B,M,ns,widths", [(2, 64, 16, [259, 128, 196, 256]), (2, 128, 32, [20, 40, 24]), (1, 32, 8, [7, 100]),
                                           (2, 32, 32, [288, 272, 384]), (2, 64, 16, [515, 256, 256, 512]), (2, 64, 32, [515, 256, 384, 512])])
@BOTH_PRECISIONS
def test_generic_eval_mlp_pool_matches_torch(dev, B, M, ns, widths, mlp_precision):
    """fused.generic_mlp_pool (inference at widths outside the specialised kernels' table: the streaming convolution kernels
    with the running-statistics BatchNorm applied in the operand loads and the pool; in strict fp32 every layer on the
    exact-fp32 MFMA convolution kernel -- never a library GEMM) against torch's eval-mode op sequence: 1e-4."""
    from spsnet_amd import fused, pointnet2_modules as PM, scenes
    torch.manual_seed(M + ns)
    mlp = scenes.fill_parameters(PM._conv_bn_relu_stack(list(widths), torch.nn.Conv2d, torch.nn.BatchNorm2d), 6).to(dev).eval()
    x = torch.randn(B, widths[0], M, ns, device=dev)
    with torch.no_grad():
        got = fused.generic_mlp_pool(mlp, x)
        want = mlp(x).max(dim=3)[0]
    assert got is not None and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert not fused.check_overflow()
    assert fused.generic_mlp_pool(mlp, x.clone().requires_grad_(True)) is None      # gradients wanted: declined


@BOTH_TRAIN_PRECISIONS
def test_fused_train_mode_mlp_under_sync_batchnorm(dev, train_precision, monkeypatch):
    """tools/train.py --sync_bn converts every BatchNorm to nn.SyncBatchNorm: the fused train-mode stack then all-reduces its
    statistics (forward) and its BatchNorm-backward sums, and returns LOCAL weight / bias gradients, as torch's SyncBatchNorm
    does.  In a one-process group the synchronised path must reproduce the plain one (output, running statistics,
    gradients), and both must agree with torch's own SyncBatchNorm op sequence."""
    import copy
    import torch.distributed as dist
    from spsnet_amd import pointnet2_modules as PM
    created = False
    if not dist.is_initialized():
        import socket
        with socket.socket() as sock:            # a free port of this host
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        created = True
    try:
        torch.manual_seed(8)
        plain = PM._conv_bn_relu_stack([12, 32, 48], torch.nn.Conv2d, torch.nn.BatchNorm2d).to(dev).train()
        synced = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(plain)).to(dev).train()
        torch_ref = copy.deepcopy(synced)
        x0 = torch.randn(2, 12, 64, 16, device=dev)
        wout = torch.randn(2, 48, 64, device=dev) * 1e-3
        monkeypatch.setattr(PM, "FUSED_MLP_TRAINING", True)
        monkeypatch.setattr(PM, "_SYNC_ALWAYS", True)
        res = []
        for mlp, fused_on in ((plain, True), (synced, True), (torch_ref, False)):
            x = x0.clone().requires_grad_(True)
            out = PM._fused_mlp_pool_train(mlp, x, 'max_pool') if fused_on else mlp(x).max(dim=3)[0]
            assert out is not None
            (out * wout).sum().backward()
            res.append([out.detach(), x.grad] + [p.grad for p in mlp.parameters()] + [b.detach().float() for b in mlp.buffers()])
        torch.cuda.synchronize()
        for other, tol in ((res[1], 1e-6), (res[2], 2e-5)):
            for a, b in zip(res[0], other):
                err = float((a - b).abs().max())
                assert err <= tol * max(1e-30, float(b.abs().max())) + 1e-12, (err, float(b.abs().max()))
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.gpu
def test_helper_streams_really_run_beside_the_pass(dev):
    """HIP maps streams onto a few hardware queues and serialises the ones that share a queue; streams.helper() only hands out
    streams that passed the device-side probe against the pass's stream and its FPS producer."""
    from spsnet_amd import streams
    main = torch.cuda.current_stream(dev)
    assert not streams.run_concurrently(main, main)                      # one stream: the setter cannot start
    producer = streams.helper(dev, main, "producer", exclusive=True)
    scale = streams.helper(dev, main, "scale0")
    assert streams.helper(dev, main, "producer") is producer             # one per (device, main stream, tag)
    assert streams.run_concurrently(main, producer) and streams.run_concurrently(producer, main)
    assert streams.run_concurrently(producer, scale) and streams.run_concurrently(main, scale)
    # every role this long-lived process has asked for on the default stream -- scales, chunks, side, check, surface, ...,
    # whatever the tests before this one needed, in whatever order -- was placed: the producer's queue is reserved FIRST
    assert streams.overlap_verified(dev, main) and streams.unplaced(dev, main) == []
    x = torch.ones(1 << 20, device=dev)
    with torch.cuda.stream(producer):                                    # the probe leaves the streams usable
        y = x * 2
    producer.synchronize()
    assert float(y.sum()) == 2.0 * (1 << 20)


def test_warm_pass_replays_from_a_graph_with_one_host_call(G, dev):
    """spsnet_amd.graphs: the streamed SA stack and an IASSD_Backbone forward captured WARM (after eager passes: weights packed,
    helper streams placed) into a HIP graph and replayed -- on the captured batch and on a second one copied into the static
    inputs: every output bit-identical to the eager pass on the same batch."""
    from spsnet_amd import backbones as BB, graphs, pointnet2_modules as M, sa_stack, scenes
    layers = sa_stack.build_sa_layers(M, sa_stack.IASSD_KITTI, seed=3).to(dev)
    batches = [scenes.make_batch("kitti-lidar-v1", 2, 16384, seed0=s) for s in (5, 50)]
    x0, f0 = G.t(batches[0][0]), G.t(batches[0][1])
    g = graphs.graphed_sa_stack(layers, x0, f0)
    with torch.no_grad():
        for xa, fa in batches + batches[:1]:
            x, f = G.t(xa), G.t(fa)
            got = [tuple(None if t is None else t.clone() for t in o) for o in g(x, f)]
            want = sa_stack.run_sa_layers(layers, x, f, overlap=False, stream_first_layer=False)
            torch.cuda.synchronize()
            assert not sa_stack.check_timeouts()
            for a, b in zip(got, want):
                for p, q in zip(a, b):
                    assert (p is None and q is None) or torch.equal(p, q)
    net = scenes.fill_parameters(BB.IASSD_Backbone(BB.IASSD_KITTI_CFG, input_channels=4, num_class=3), 5).to(dev).eval()

    def points_of(xa, fa):
        bidx = np.repeat(np.arange(2, dtype=np.float32), 16384)[:, None]
        return G.t(np.concatenate([bidx, xa.reshape(-1, 3), fa.transpose(0, 2, 1).reshape(-1, 1)], 1).astype(np.float32))
    pts = [points_of(*b) for b in batches]
    gb = graphs.graphed_backbone(net, 2, pts[0])
    with torch.no_grad():
        for p in pts + pts[:1]:
            out = gb(p)
            got = {k: out[k].clone() for k in ("centers", "centers_features", "ctr_offsets", "encoder_features") if isinstance(out[k], torch.Tensor)}
            assert bool(out["scene_sizes_equal"])          # (the reference's assert, kept on the device under replay)
            want = net(dict(batch_size=2, points=p))
            torch.cuda.synchronize()
            for k, v in got.items():
                assert torch.equal(v, want[k]), k


@pytest.mark.parametrize("mode", ["streamed", "seq"])
def test_first_pass_of_a_fresh_process_captures_into_a_graph(dev, mode):
    """include/spsnet_sa.h promises launchers that neither allocate nor synchronise (legal under stream capture); the one
    call that does both is sps_init().  A FRESH process (tools/graph_try.py as a subprocess: nothing of the library has run
    in it) calls spsnet_amd.init(), captures its very first SA-stack pass -- the streamed schedule with its helper streams,
    bounded waits, packed columns and early stages, or the sequential one -- into a HIP graph and replays it on the captured
    batch and on a second batch copied into the static inputs: every output bit-identical to an eager sequential pass (stale
    per-launch state -- progress counters, zero pools, the pre-pass's flag epochs -- would show on the second batch)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GRAPH_TRY_B="2")
    done = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_try.py"), mode, "fp32"], cwd=root, env=env,
                          capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and "GRAPH_TRY_OK" in done.stdout, (done.stdout[-2000:], done.stderr[-3000:])
    assert done.stdout.count("identical to an eager sequential pass: True; timeouts False") == 2, done.stdout[-2000:]


def test_sps_init_is_idempotent_and_launchers_never_allocate(ext, G, oracle, dev):
    """sps_init / sps_is_initialized (include/spsnet_sa.h): idempotent; the publishing FPS under stream capture declines the
    sorting pre-pass (its flags carry a per-launch epoch a replay could not renew) and still samples exactly."""
    import ctypes
    import spsnet_amd
    from spsnet_amd import _lib
    L = _lib.load()
    assert spsnet_amd.init(dev) and L.sps_is_initialized(dev.index or 0) == 1
    assert L.sps_init(dev.index or 0, ctypes.c_void_p(_lib.raw_stream(dev))) == 0          # again: a no-op
    assert L.sps_init(99, None) != 0 and b"no device" in L.sps_last_error()
    xyz = cloud(np.random.default_rng(3), 2, 8192, dup=0.05)
    x = G.t(xyz)
    want = oracle.fps(xyz, 512)
    idx = torch.zeros((2, 512), dtype=torch.int32, device=dev)
    progress = torch.zeros((2,), dtype=torch.int32, device=dev)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        progress.zero_()
        work = ext.fps_publish(x, None, idx, progress)
    for _ in range(2):
        idx.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(G.n(idx), want)
        assert G.n(progress).tolist() == [512, 512]
    del work


def test_helper_streams_of_a_second_pass_and_forget(dev):
    """A pass issued from a stream of its own gets its own helpers (placed by the same rules); forget() drops them -- the
    registry, the helper -> root links and the callers' caches -- and the next request places a fresh set."""
    from spsnet_amd import sa_stack, streams
    own = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(own):
        side = sa_stack._helper_stream(dev, "side")
        producer = sa_stack._helper_stream(dev, "producer")
        assert streams.helper(dev, own, "producer") is producer and streams.helper(dev, side, "side") is side
        assert streams.overlap_verified(dev, own)
        assert streams.run_concurrently(own, producer) and streams.run_concurrently(producer, side)
        n_cached = len(sa_stack._SIDE_STREAMS)
        streams.forget(dev, own)
        assert len(sa_stack._SIDE_STREAMS) == n_cached - 2
        assert not streams.overlap_verified(dev, own)                    # nothing registered: nothing verified
        again = sa_stack._helper_stream(dev, "producer")
        assert streams.helper(dev, own, "producer") is again and streams.overlap_verified(dev, own)
        streams.forget(dev, own)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ exact fp32: layer 1's feature product once per point
@pytest.mark.parametrize("cf,widths", [(64, ([64, 64, 128], [64, 96, 128])), (128, ([128, 128, 256], [128, 256, 256]))])
def test_layer1_per_point_form_matches_the_grouped_one(ext, G, dev, cf, widths):
    """sps_sa_layer1_per_point + mode bit 32 of the exact-fp32 point-major kernel: b1 + W1f . features once per POINT, the
    coordinate k-step per grouped point.  Against the kernel that multiplies the features per grouped point: the same pooled
    features up to summation order (<= 2e-6 of the layer's scale), with packed and unpacked columns, and both within 1e-4 of a
    float64 restatement of group -> SharedMLP -> max-pool (pointnet2_modules.py:114-122, eval-mode BatchNorm folded)."""
    from spsnet_amd import fused, pointnet2_modules as M
    rng = np.random.default_rng(cf)
    B, N, Mc = 2, 1024, 512
    x = G.t(cloud(rng, B, N, dup=0.02))
    new_xyz = x[:, :Mc].contiguous()
    feats = fused.attach_point_major_twin(torch.randn(B, cf, N, device=dev))
    old, old_hoist = fused.set_precision("fp32"), fused.HOIST_LAYER1
    fused.HOIST_LAYER1 = True      # (the default; SPS_HOIST_LAYER1=0 turns it off)
    try:
        mod = M.PointnetSAModuleMSG_WithSampling(
            npoint_list=[Mc], sample_range_list=[-1], sample_type_list=['ctr_aware'], radii=[0.8, 1.6], nsamples=[16, 32],
            mlps=[[cf] + widths[0], [cf] + widths[1]], use_xyz=True, dilated_group=False, aggregation_mlp=None,
            confidence_mlp=None, num_class=3).to(dev).eval()
        for mlp in mod.mlps:                       # non-trivial BatchNorm statistics
            for layer in mlp:
                if isinstance(layer, torch.nn.BatchNorm2d):
                    layer.running_mean.uniform_(-0.2, 0.2)
                    layer.running_var.uniform_(0.5, 1.5)
                    layer.weight.data.uniform_(0.5, 1.5)
                    layer.bias.data.uniform_(-0.2, 0.2)
        with torch.no_grad():
            plan = mod._fused_plan(x, new_xyz, feats)
            assert plan and all(p.split == 0 and p.point_major for p in plan)
            assert all(fused.can_hoist_layer1(p, B, N, Mc, g.nsample) for p, g in zip(plan, mod.groupers))
            ga, gb = mod.groupers
            width = sum(p.c3_real for p in plan)
            idxs = ext.ball_query_full2(ga.radius, ga.nsample, gb.radius, gb.nsample, x, new_xyz)
            packs = fused.pack_columns2(*idxs)
            hoist = mod._layer1_per_point(x, new_xyz, feats, plan)
            assert hoist is not None
            outs = {}
            for name, cols, h in (("plain", [None, None], None), ("plain-packed", list(packs), None),
                                  ("per-point", [None, None], hoist), ("per-point-packed", list(packs), hoist)):
                pm = cols[0] is not None
                out = torch.empty((B, Mc, width) if pm else (B, width, Mc), device=dev)
                mod._run_scales(x, new_xyz, feats, idxs, plan, out, cols, pm, hoist=h)
                torch.cuda.synchronize()
                outs[name] = out.transpose(1, 2) if pm else out
            # float64 restatement
            want = []
            for g, mlp, idx in zip(mod.groupers, mod.mlps, idxs):
                grouped = torch.cat([(x.transpose(1, 2).double()[:, :, None, :].expand(B, 3, Mc, N).gather(
                                        3, idx.long()[:, None].expand(B, 3, Mc, g.nsample)) - new_xyz.transpose(1, 2).double()[..., None]),
                                     feats.double()[:, :, None, :].expand(B, cf, Mc, N).gather(
                                        3, idx.long()[:, None].expand(B, cf, Mc, g.nsample))], dim=1)
                want.append(mlp.double()(grouped).amax(dim=3))
                mlp.float()
            want = torch.cat(want, dim=1)
        scale = float(want.abs().max())
        assert torch.equal(outs["plain"], outs["plain-packed"]) and torch.equal(outs["per-point"], outs["per-point-packed"])
        assert float((outs["per-point"] - outs["plain"]).abs().max()) <= 2e-6 * scale
        for name in ("plain", "per-point"):
            assert float((outs[name].double() - want).abs().max()) <= 1e-4 * max(scale, 1.0), name
    finally:
        fused.set_precision(old)
        fused.HOIST_LAYER1 = old_hoist


@pytest.mark.parametrize("B", [1, 8])
def test_layer1_form_gating_changes_only_last_bits(ext, G, dev, B):
    """The exact-fp32 MLP contract is tolerance-based (1e-4), the INDEX contract ends at the layer's sampler: which form of layer
    1 runs (the grouped one, or its feature product once per point) depends on shape gating -- a point-major twin, M ns >= 4 N,
    `early_pool_plan` (B M <= 8192, enough columns to pack), whether the layer is a plain D-FPS layer.  Here a plain D-FPS layer
    at IA-SSD layer 1's widths, at a batch size where `early_pool_plan` is None (B = 1: too few columns) and at the bench's
    (B = 8: the plan exists, the layer keeps the grouped form): sampled indices identical to the form-forced runs, features
    within 2e-6 of the layer's scale of each other whatever the gate picked."""
    from spsnet_amd import fused, pointnet2_modules as M, scenes
    torch.manual_seed(7)
    mod = M.PointnetSAModuleMSG_WithSampling(
        npoint_list=[1024], sample_range_list=[-1], sample_type_list=['D-FPS'], radii=[0.8, 1.6], nsamples=[16, 32],
        mlps=[[64, 64, 64, 128], [64, 64, 96, 128]], use_xyz=True, dilated_group=False, aggregation_mlp=[128], confidence_mlp=[128],
        num_class=3)
    scenes.fill_parameters(mod, 5)
    mod = mod.to(dev).eval()
    xyz_np, _ = scenes.make_batch("kitti-lidar-v1", B, 4096, seed0=31)
    x = G.t(xyz_np)
    feats = fused.attach_point_major_twin(torch.randn(B, 64, 4096, device=dev))
    old, old_hoist = fused.set_precision("fp32"), fused.HOIST_LAYER1
    try:
        outs = {}
        with torch.no_grad():
            plan_exists = mod.early_pool_plan(x, x[:, :1024].contiguous(), feats) is not None
            assert plan_exists == (B == 8)
            for name, hoist in (("default", True), ("grouped", False)):
                fused.HOIST_LAYER1 = hoist
                nx, nf, cls, idx, _ = mod(x, feats)
                outs[name] = (idx.clone(), nf.clone(), cls.clone())
        assert torch.equal(outs["default"][0], outs["grouped"][0])
        scale = float(outs["grouped"][1].abs().max())
        assert float((outs["default"][1] - outs["grouped"][1]).abs().max()) <= 2e-6 * max(scale, 1.0)
        assert float((outs["default"][2] - outs["grouped"][2]).abs().max()) <= 1e-5 * max(1.0, float(outs["grouped"][2].abs().max()))
        if plan_exists:      # a layer sa_stack may start on a partly written cloud keeps the grouped form in both schedules
            assert torch.equal(outs["default"][1], outs["grouped"][1])
    finally:
        fused.set_precision(old)
        fused.HOIST_LAYER1 = old_hoist
