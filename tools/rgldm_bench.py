"""RGLDM candidate matching time: the 28 pairs of 8 device-resident point sets of 20,000
points (the bead count of a C4 view) through spim_rgldm_match at the reference's defaults
(3 neighbours, redundancy 1, ratio 3, threshold 50), and the NumPy restatement
(tests/rgldm_ref.py) of one pair at a reduced size on the same box as the stand-in baseline
(the Java reference cannot run here).

    python tools/rgldm_bench.py [--points 20000] [--views 8] [--reps 5] [--warmup 2]
                                [--baseline-points 2000] [--out profiles/rgldm_bench.json]

Every set sees the same world beads (85 % of them, 0.2 px of noise) under its own translation,
so the matcher finds candidates as it does on real views.  Each call returns after its stream
has drained; a timed call is bracketed by two HIP events on the caller's stream (wall clock
beside it).  The fp64 operation count is DESIGN.md's model: per descriptor pair 8 (nn+re)^2
for the square-distance table and C(nn+re, nn)^2 * nn for the pairings (nn - 1 additions and
one minimum each); the neighbour search is counted apart (8 per point pair and set).
Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def point_sets(views: int, n: int, seed: int = 20140611, box: float = 768.0):
    rng = np.random.default_rng(seed)
    world = rng.uniform(0.0, box, (int(n / 0.85) + 1, 3))
    out = []
    for _ in range(views):
        p = world[rng.permutation(len(world))[:n]] + rng.uniform(-0.2, 0.2, (n, 3)) + rng.uniform(-20, 20, 3)
        out.append(np.ascontiguousarray(p))
    return out


def pair_ops(nn: int, re: int) -> int:
    m = nn + re
    return 8 * m * m + math.comb(m, nn) ** 2 * nn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-points", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgldm_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import registration
    import rgldm_ref as rr

    host = point_sets(a.views, a.points)
    dev = [torch.from_numpy(p).to("cuda:0") for p in host]
    pairs = [(u, v) for u in range(a.views) for v in range(u + 1, a.views)]

    def timed(u, v):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        ia, _ = registration.rgldm_candidates(dev[u], dev[v])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, len(ia)

    for _ in range(a.warmup):
        timed(0, 1)
    per_pair, wall, cands = [], [], []
    for u, v in pairs:
        ms, w, c = timed(u, v)
        per_pair.append(ms)
        wall.append(w)
        cands.append(c)
    first = [timed(0, 1)[0] for _ in range(a.reps)]   # the spread of one pair
    # the descriptor stage alone (one set), to split a call's time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    registration.descriptors(dev[0])
    knn_ms = (time.perf_counter() - t0) * 1e3

    # the stand-in baseline: the NumPy restatement, one pair, reduced size, same box
    nb = a.baseline_points
    base = point_sets(2, nb, seed=7)
    t0 = time.perf_counter()
    want = rr.rgldm(base[0], base[1])
    base_ms = (time.perf_counter() - t0) * 1e3
    got = registration.rgldm_candidates(base[0], base[1], return_all=True)
    same = (np.array_equal(got[0], want["ia"]) and np.array_equal(got[1], want["ib"])
            and np.array_equal(got[3].view(np.uint64), want["best"].view(np.uint64))
            and np.array_equal(got[4].view(np.uint64), want["second"].view(np.uint64)))
    small = [timed_small(registration, torch, base) for _ in range(3)]

    ops = pair_ops(3, 1)
    n = a.points
    med = float(np.median(per_pair))
    r3 = lambda x: round(float(x), 3)
    res = {
        "workload": f"{len(pairs)} pairs of {a.views} device-resident point sets of {n} points, whole "
                    "spim_rgldm_match calls (finite check, descriptors of both sets, matching, merge, "
                    "compaction, results to the host), defaults 3 / 1 / 3 / 50",
        "reps_of_first_pair": a.reps, "warmup": a.warmup,
        "pair_ms": [r3(x) for x in per_pair], "pair_ms_median": r3(med), "pair_ms_min": r3(min(per_pair)),
        "pair_ms_max": r3(max(per_pair)), "total_ms": r3(sum(per_pair)), "total_ms_wall": r3(sum(wall)),
        "first_pair_ms_repeated": [r3(x) for x in first],
        "descriptors_call_ms_wall_one_set": r3(knn_ms),
        "candidates_per_pair_median": int(np.median(cands)),
        "fp64_ops_per_descriptor_pair_model": ops,
        "matching_fp64_ops_per_pair_of_views": ops * n * n,
        "knn_ops_per_pair_of_views_model": 2 * 8 * n * n,
        "matching_fp64_Tops_per_s_whole_call": r3(ops * n * n / (med * 1e-3) / 1e12),
        "baseline": {"what": "NumPy restatement (tests/rgldm_ref.py), one pair, same box, one process",
                     "points": nb, "numpy_ms": r3(base_ms), "gpu_ms_same_size": r3(float(np.median(small))),
                     "gpu_equals_restatement_bit_for_bit": bool(same)},
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def timed_small(registration, torch, base):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    registration.rgldm_candidates(base[0], base[1])
    return (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    main()
