"""A point-record round for the register-resident pruned FPS kernel (fps_pruned.hip), modelled exactly in numpy, with its
per-round counts.  Built into the kernel and measured slower in round 6, not shipped: DESIGN 4.1, profiles/round6/.

Each round every wave publishes its T best points by key {running distance, inverted rank} and the exact running distance
of its (T+1)-th best point (its BOUND); every wave then runs sequential FPS over the 8 T records: take the largest key,
lower every remaining record by the exact update, stop at the first record that does not beat the running bound.  The
running bound collects the own distance of every pick and the BOUND of every EXPOSED wave (no remaining record of it that
is unchanged or still above its BOUND).  The accepted centres are then applied.

`point_record_fps` returns the indices and final running distances (tests/test_fps_point_records_cpu.py holds them against
the C oracle) plus per-round counts; run as a script it prints those counts per round:

    python3 tools/fps_records_model.py [T ...]      # KITTI-shaped, 16 384 -> 4 096, seed 0
"""
import os
import sys

import numpy as np

W = 8  # waves per scene


def sqdist(px, py, pz, cx, cy, cz):
    """fp32 fma(dz, dz, fma(dx, dx, dy * dy)), each subtraction rounded to fp32 (the kernels' and the oracle's order).
    The fmas are evaluated in extended precision and rounded once to fp32."""
    f32, ld = np.float32, np.longdouble
    dx = (np.float32(px) - np.float32(cx)).astype(f32)
    dy = (np.float32(py) - np.float32(cy)).astype(f32)
    dz = (np.float32(pz) - np.float32(cz)).astype(f32)
    t = (dy * dy).astype(f32)
    t = (dx.astype(ld) * dx.astype(ld) + t.astype(ld)).astype(f32)
    t = (dz.astype(ld) * dz.astype(ld) + t.astype(ld)).astype(f32)
    return t


def fmin_raw(d, t):
    """v_min_f32 in IEEE mode: the non-NaN operand."""
    return np.where(np.isnan(d), t, np.fmin(d, t)).astype(np.float32)


def ranks(n, bs):
    """The reference's tie-break rank of point k: bit-reversed (k mod bs), then k / bs (smaller wins)."""
    l2 = bs.bit_length() - 1
    rb = 0
    while (1 << rb) < -(-n // bs):
        rb += 1
    k = np.arange(n, dtype=np.int64)
    low = k & (bs - 1)
    rev = np.zeros_like(low)
    for b in range(l2):
        rev |= ((low >> b) & 1) << (l2 - 1 - b)
    return (rev << rb) | (k >> l2)


def buckets(xyz):
    """Spatially compact 64-point buckets (a cell-key sort, as the kernel's) and the wave of every point."""
    lo, hi = np.nanmin(np.where(np.isfinite(xyz), xyz, np.nan), 0), np.nanmax(np.where(np.isfinite(xyz), xyz, np.nan), 0)
    lo, hi = np.nan_to_num(lo), np.nan_to_num(hi)
    q = np.clip(np.nan_to_num((xyz - lo) / np.maximum(hi - lo, 1e-30) * 16, posinf=15, neginf=0), 0, 15).astype(np.int64)
    key = np.zeros(len(xyz), np.int64)
    for b in range(3, -1, -1):
        for a in range(3):
            key = (key << 1) | ((q[:, a] >> b) & 1)
    order = np.argsort(key, kind="stable")
    bucket = np.empty(len(xyz), np.int64)
    bucket[order] = np.arange(len(xyz)) // 64
    return bucket, bucket % W


def point_record_fps(xyz, m, bs, T=4, temp=None):
    """One scene: (idx, final temp, per-round stats) of the kernel's round rule."""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    t = np.full(n, 1e10, np.float32) if temp is None else np.array(temp, np.float32)
    inv = 0x0FFFFFFF - ranks(n, bs)        # larger wins a distance tie
    bits = t.view(np.int32)                 # (the kernel compares distance bits as signed ints)
    bucket, wave = buckets(xyz)
    members = [np.where(wave == w)[0] for w in range(W)]
    idx = np.zeros(m, np.int32)
    stats = []
    pend = [0] if m > 1 else []
    j = 1
    while True:
        st = dict(pairs=0, buckets_per_wave=np.zeros(W, int), picks=0, loop=0, stop="end")
        if pend:   # apply: per wave, the (bucket, centre) pairs and the distinct buckets the centres reach
            hit = set()
            for c in pend:
                low = fmin_raw(sqdist(X, Y, Z, X[c], Y[c], Z[c]), t)
                h = np.unique(bucket[low.view(np.int32) != t.view(np.int32)])
                st["pairs"] += len(h)
                hit.update(h.tolist())
                t = low
            for g in hit:
                st["buckets_per_wave"][g % W] += 1
            bits = t.view(np.int32)
        if j >= m:
            break
        # candidates: per wave the T best keys and the (T+1)-th distance
        rec, bound = [], np.empty(W, np.float32)
        for w, mem in enumerate(members):
            o = np.lexsort((-inv[mem], -bits[mem]))[:T + 1]
            rec += list(mem[o[:T]])
            bound[w] = t[mem[o[T]]]
        rec = np.array(rec)
        rw = np.repeat(np.arange(W), T)
        v0 = t[rec].copy()
        v = v0.copy()
        alive = np.ones(len(rec), bool)
        exposed = np.zeros(W, bool)
        bnd_bits = np.int32(-2 ** 31)   # the running bound, as distance bits (the kernel compares them as signed ints)
        picked = []
        while len(picked) < m - j and alive.any():
            vb = np.where(alive, v.view(np.int32), np.int32(-2 ** 31))
            cand = np.where(alive & (vb == vb.max()))[0]
            b = cand[np.argmax(inv[rec[cand]])]
            st["loop"] += 1
            if picked and not (v[b] > np.int32(bnd_bits).view(np.float32)):
                st["stop"] = "lowered" if v[b] != v0[b] else "hidden"
                break
            alive[b] = False
            picked.append(b)
            c = rec[b]
            own = fmin_raw(sqdist(X[c], Y[c], Z[c], X[c], Y[c], Z[c]), v[b])
            bnd_bits = max(bnd_bits, np.float32(own).view(np.int32))
            v = fmin_raw(sqdist(X[rec], Y[rec], Z[rec], X[c], Y[c], Z[c]), v)
            shield = alive & ((v.view(np.int32) == v0.view(np.int32)) | (v > bound[rw]))
            for w in range(W):
                if not exposed[w] and not shield[rw == w].any():
                    exposed[w] = True
                    bnd_bits = max(bnd_bits, bound[w].view(np.int32))
        L = len(picked)
        for p, b in enumerate(picked):
            idx[j + p] = rec[b]
        pend = [rec[b] for p, b in enumerate(picked) if j + p != m - 1]
        st["picks"] = L
        j += L
        stats.append(st)
    return idx, t, stats


def scene_fps(xyz, m, bs, T=4, temp=None):
    """(B, N, 3) -> idx (B, m), temp (B, N), stats; bs = the reference's block size for N (oracle.opt_n_threads)."""
    out = [point_record_fps(xyz[b], m, bs, T, None if temp is None else temp[b]) for b in range(len(xyz))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle
    from spsnet_amd import scenes
    N, M = 16384, 4096
    xyz = scenes.make_batch("kitti-lidar-v1", 1, N, seed0=int(os.environ.get("SEED", 0)))[0][0]
    for T in [int(a) for a in sys.argv[1:]] or [3, 4, 6]:
        _, _, st = scene_fps(xyz[None], M, oracle.opt_n_threads(N), T)
        st = st[0]
        R = len(st)
        picks = sum(s["picks"] for s in st)
        pairs = sum(s["pairs"] for s in st)
        per_wave = np.array([s["buckets_per_wave"] for s in st])
        loop = sum(s["loop"] for s in st)
        stops = {k: sum(s["stop"] == k for s in st) for k in ("hidden", "lowered", "end")}
        print(f"T={T}: rounds={R} picks/round={picks / R:.2f} accept-loop steps/round={loop / R:.2f} "
              f"lowered (bucket, centre) pairs/round={pairs / R:.1f} distinct lowered buckets/round: mean wave "
              f"{per_wave.sum(1).mean() / W:.2f}, busiest wave {per_wave.max(1).mean():.2f}; stops={stops}")
