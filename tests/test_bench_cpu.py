"""bench.py's host-side logic that needs no GPU: the oracle verdict attached to `validated` (the timed batch against the CPU
oracle's pass over the same scenes and weights)."""
import copy
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("sps_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_oracle_verdict_accepts_the_oracle_and_names_what_differs(oracle):
    from oracle import cpu_stack
    from spsnet_amd import pointnet2_modules as M, sa_stack, scenes
    bench = _bench()
    cfg = sa_stack.scaled_config(npoints=[256, 64, 32])
    layers = cpu_stack.cpu_copy(sa_stack.build_sa_layers(M, cfg, seed=2))
    xyz, feats = scenes.make_batch("kitti-lidar-v1", 2, 1024, seed0=5)
    want = cpu_stack.sa_stack_cpu(layers, xyz, feats)
    samplers = [m[0] for m in cfg["sample_method_list"]]
    rec, bad = bench.oracle_verdict(copy.deepcopy(want), want, samplers, 1e-4)
    assert not bad and rec["ok"] and rec["idx_exact"] and rec["new_xyz_exact"] and rec["max_abs_err_features"] == 0.0
    assert [r["sampler"] for r in rec["layers"]] == samplers and rec["scenes"] == 2

    got = [tuple(None if a is None else a.copy() for a in o) for o in want]
    got[0][3][1, 7] += 1                                   # one D-FPS pick off by one
    rec, bad = bench.oracle_verdict(got, want, samplers, 1e-4)
    assert not rec["ok"] and not rec["idx_exact"] and any("layer 0" in b and "indices" in b for b in bad)

    got = [tuple(None if a is None else a.copy() for a in o) for o in want]
    got[1][1][0, 3, 5] += 1e-2 * max(1.0, float(np.abs(want[1][1]).max()))
    rec, bad = bench.oracle_verdict(got, want, samplers, 1e-4)
    assert not rec["ok"] and rec["idx_exact"] and any("layer 1: features" in b for b in bad)

    # a score-sampled layer whose picks swapped a near-tie: rows are matched by sampled index, not by position
    got = [tuple(None if a is None else a.copy() for a in o) for o in want]
    perm = np.arange(want[2][3].shape[1])
    perm[[3, 4]] = perm[[4, 3]]
    got[2] = (got[2][0][:, perm], got[2][1][:, :, perm], got[2][2][:, perm], got[2][3][:, perm])
    rec, bad = bench.oracle_verdict(got, want, samplers, 1e-4)
    assert not bad and rec["layers"][2]["picks_shared_with_oracle"] == 1.0


def test_dump_outputs_writes_every_layer_and_samples_within_budget(tmp_path):
    """--dump-outputs: every non-None output of every layer as float32 (floats) / float64 (indices, exact); over the byte
    budget, each array becomes the same seeded sample of its elements, identical from call to call."""
    import torch
    bench = _bench()
    rng = np.random.default_rng(0)
    outs = [(torch.from_numpy(rng.standard_normal((2, 64, 3)).astype(np.float32)),
             torch.from_numpy(rng.standard_normal((2, 16, 64)).astype(np.float16)),
             None,
             torch.from_numpy(rng.integers(0, 1 << 20, (2, 64)).astype(np.int32))),
            (torch.zeros(2, 8, 3), torch.ones(2, 32, 8), torch.full((2, 8, 3), 0.5), torch.arange(16, dtype=torch.int32).view(2, 8))]
    full = bench.dump_outputs(outs, str(tmp_path / "full"))
    assert sorted(full) == ["layer0_features", "layer0_idx", "layer0_xyz", "layer1_cls", "layer1_features", "layer1_idx",
                            "layer1_xyz"]
    for k, o in enumerate(outs):
        for field, t in zip(bench.DUMP_FIELDS, o):
            if t is None:
                continue
            a = np.load(tmp_path / "full" / f"layer{k}_{field}.npy")
            assert a.dtype == (np.float64 if field == "idx" else np.float32)
            np.testing.assert_array_equal(a, t.numpy().astype(a.dtype))
    budget = 2048
    small = bench.dump_outputs(outs, str(tmp_path / "a"), budget=budget)
    again = bench.dump_outputs(outs, str(tmp_path / "b"), budget=budget)
    assert small == again
    assert sum(int(np.load(tmp_path / "a" / f"{n}.npy").nbytes) for n in small) <= budget
    for name in small:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        np.testing.assert_array_equal(a, b)
        assert np.isin(a, np.load(tmp_path / "full" / f"{name}.npy")).all()
