"""The register-resident pruned FPS kernel (fps_pruned.hip) against the oracle, indices AND final running distances
bit-exact, through all four launch forms: plain, PRESORT (sorting pre-pass), PUBLISH (progress words checked) and RESOLVE
(behind the ordered-prefix check of fps_verify.hip).  The clouds stress the multi-pick round: many exact ties inside one
wave, dense clumps where every record of a round lowers the next, the smallest N the kernel takes, N not a multiple of 64,
m close to N, NaN / Inf points."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext(dev):
    import spsnet_amd.pointnet2_batch_cuda as e
    return e


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    return gpu_util


def _cloud(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":         # few distinct coordinates per axis: many records of one wave tie exactly
        return (rng.integers(0, 6, (N, 3)) * 0.5).astype(np.float32)
    if kind == "clusters":     # dense clumps: every record of a round lowers the next
        c = rng.uniform(-40, 40, (16, 3)).astype(np.float32)
        return (c[rng.integers(0, 16, N)] + rng.normal(0, 0.02, (N, 3))).astype(np.float32)
    if kind == "kitti":
        from spsnet_amd import scenes
        return scenes.make_batch("kitti-lidar-v1", 1, N, seed0=seed, dup_fraction=0.02)[0][0]
    if kind == "bad":          # NaN and Inf coordinates
        x = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
        x[17] = np.nan
        x[900, 2] = np.inf
        x[901, 0] = -np.inf
        x[N - 1, 1] = np.nan
        return x
    return rng.uniform(-3, 3, (N, 3)).astype(np.float32)


def _batch(kinds, N, seed):
    return np.ascontiguousarray(np.stack([_cloud(k, N, seed + i) for i, k in enumerate(kinds)]))


CASES = [(["ties", "clusters"], 16384, 4096), (["ties", "kitti"], 6144, 2048), (["clusters", "uniform"], 7001, 1500),
         (["uniform", "ties"], 6144, 6144), (["kitti", "clusters"], 9000, 8990), (["bad", "uniform"], 8192, 700)]


@pytest.mark.parametrize("kinds,N,m", CASES)
def test_point_records_plain_and_presorted(ext, G, oracle, kinds, N, m):
    from spsnet_amd import _lib
    L = _lib.load()
    xyz = _batch(kinds, N, N + m)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    got, got_t = G.fps(ext, xyz, m)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)
    B = len(xyz)
    x = G.t(xyz)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=x.device)
    idx = torch.empty((B, m), dtype=torch.int32, device=x.device)
    work = torch.empty((B * int(L.sps_fps_workspace_floats(N)),), dtype=torch.float32, device=x.device)
    _lib.check(L.sps_fps_with_workspace(B, N, m, x.data_ptr(), temp.data_ptr(), idx.data_ptr(), work.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "fps")
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)


@pytest.mark.parametrize("presort", [True, False])
@pytest.mark.parametrize("kinds,N,m", [CASES[0], CASES[2], CASES[4]])
def test_point_records_publish(ext, G, oracle, kinds, N, m, presort):
    xyz = _batch(kinds, N, N + 3 * m)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    x = G.t(xyz)
    B = len(xyz)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=x.device)
    idx = torch.zeros((B, m), dtype=torch.int32, device=x.device)
    progress = torch.zeros((B,), dtype=torch.int32, device=x.device)
    work = ext.fps_publish(x, temp, idx, progress, presort=presort)
    torch.cuda.synchronize()
    del work
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)
    assert G.n(progress).tolist() == [m] * B


def test_point_records_resolve(ext, G, oracle):
    """RESOLVE: the ordered-prefix check confirms scene 0 and refuses the shuffled scene 1, which the RESOLVE launch redoes."""
    from spsnet_amd import scenes
    base, _ = scenes.make_batch("kitti-lidar-v1", 2, 24000, seed0=5)
    i0 = oracle.fps(base, 8192)
    x1 = np.ascontiguousarray(np.take_along_axis(base, i0[..., None].astype(np.int64).repeat(3, axis=2), axis=1))
    x1[1] = x1[1][np.random.default_rng(2).permutation(8192)]
    want, want_t = oracle.fps(x1, 2048, return_temp=True)
    idx, flags, temp = ext.fps_ordered_prefix(G.t(x1), 2048, return_flags=True)
    np.testing.assert_array_equal(G.n(idx), want)
    np.testing.assert_array_equal(G.n(temp), want_t)
    assert G.n(flags).tolist() == [0, 1]
