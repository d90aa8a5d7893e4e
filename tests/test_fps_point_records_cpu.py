"""The point-record round modelled for the register-resident pruned FPS kernel, proven on the CPU: every wave publishes its
four best points and the exact distance of its fifth, every wave re-ranks the published records by sequential FPS with
the exact update arithmetic, and stops at the first record that does not beat the running bound (own distances of the
picks, bounds of exposed waves).  tools/fps_records_model.py is that round in numpy; it must reproduce the C oracle's
sequential FPS -- indices and final running distances -- exactly."""
import numpy as np
import pytest

from tools import fps_records_model as F


def _cloud(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "kitti":
        from spsnet_amd import scenes
        return scenes.make_batch("kitti-lidar-v1", 1, N, seed0=seed, dup_fraction=0.02)[0]
    if kind == "uniform":
        return rng.uniform(-3, 3, (1, N, 3)).astype(np.float32)
    if kind == "lattice":      # integer lattice: exact ties everywhere
        return (rng.integers(-4, 5, (1, N, 3)) * 0.25).astype(np.float32)
    if kind == "duplicates":   # 200 locations, every point a duplicate
        c = rng.uniform(-20, 20, (200, 3)).astype(np.float32)
        return c[rng.integers(0, 200, N)][None]
    if kind == "mirror4":      # 4-fold mirror symmetry: exact ties across waves
        q = rng.uniform(0.05, 30.0, (N // 4, 3)).astype(np.float32)
        x = np.concatenate([q * np.array(s, np.float32) for s in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))])
        return x[rng.permutation(len(x))][None]
    if kind == "collinear":
        x = np.zeros((1, N, 3), np.float32)
        x[0, :, 0] = rng.permutation(N).astype(np.float32) * 0.01
        return x
    if kind == "clusters":     # tight far-apart clumps: every record of a round lowers the next
        c = rng.uniform(-40, 40, (24, 3)).astype(np.float32)
        return (c[rng.integers(0, 24, N)] + rng.normal(0, 0.05, (N, 3))).astype(np.float32)[None]
    raise ValueError(kind)


@pytest.mark.parametrize("kind,N,m", [("kitti", 8192, 2048), ("uniform", 6144, 1536), ("lattice", 4096, 600),
                                      ("duplicates", 4096, 1024), ("mirror4", 4096, 1024), ("collinear", 4096, 800),
                                      ("clusters", 4096, 1024), ("uniform", 1000, 1000)])
def test_point_record_rounds_reproduce_sequential_fps(oracle, kind, N, m):
    xyz = _cloud(kind, N, 7)
    want, want_t = oracle.fps(xyz, m, return_temp=True)
    got, got_t, stats = F.scene_fps(xyz, m, oracle.opt_n_threads(N))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_t, want_t)
    assert sum(s["picks"] for s in stats[0]) == m - 1


def test_point_records_take_several_picks_per_round(oracle):
    """On a KITTI-shaped cloud the rule accepts far more than the one pick a round must make."""
    xyz = _cloud("kitti", 8192, 3)
    _, _, stats = F.scene_fps(xyz, 2048, oracle.opt_n_threads(8192))
    assert 2047 / len(stats[0]) > 8
