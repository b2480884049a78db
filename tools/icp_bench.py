"""ICP assignment and loop time: one ``spim_icp_assign`` call and a whole ``registration.icp``
run on two device-resident lists of 16,000 points, beside the host time of
``scipy.spatial.cKDTree`` build plus query on the same float coordinates -- the reference's
per-iteration algorithm (SimplePointMatchIdentification.java:32-48 builds a kd-tree of the
target in every iteration) -- and the geometric hashing neighbour search recorded in
profiles/gh_bench.json.

    python tools/icp_bench.py [--sizes 16000] [--reps 15] [--warmup 3] [--out profiles/icp_bench.json]

The lists are those of tools/gh_bench.py (85 % of the world beads in each, 0.05 px of noise),
but B lies under a small rigid offset (0.2 degrees about y, (0.8, -0.5, 0.3) px) instead of a
45 degree rotation, so most points have their partner within max_distance.  Each call returns
after its stream has drained and its results are on the host; a timed call is bracketed by two
HIP events on the caller's stream (wall clock beside it); the median and the spread (min, max)
over --reps are reported.  A whole spim_icp_assign call holds the finite checks of both lists,
apply, assign, merge, resolve, compaction and the copies of nearest / dist / matches to the
host.  The pair model counts per reference-target pair 3 float subtractions, 3 widenings, 3
double products, 2 double additions and a double comparison.  Prints one JSON line and writes
it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# profiles/gh_bench.json at 16,000: two spim_gh_descriptors calls (1.90 ms each), that is the
# neighbour search k_pm_knn<3> of both lists -- 2 n^2 point pairs through the same
# Detection.distanceTo chain -- with their finite checks, descriptors and copies out
GH_KNN_MS_16000 = 3.8


def lists(n: int, seed: int = 20140611, box: float = 768.0):
    rng = np.random.default_rng(seed + n)
    side = box * (n / 20000.0) ** (1.0 / 3.0)          # the bead density of a C4 view at every size
    world = rng.uniform(0.0, side, (int(n / 0.85) + 1, 3))
    a = world[rng.permutation(len(world))[:n]] + rng.uniform(-0.05, 0.05, (n, 3))
    b = world[rng.permutation(len(world))[:n]] + rng.uniform(-0.05, 0.05, (n, 3))
    c, s = np.cos(np.deg2rad(0.2)), np.sin(np.deg2rad(0.2))
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.ascontiguousarray(a), np.ascontiguousarray(b @ rot.T + [0.8, -0.5, 0.3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from scipy.spatial import cKDTree
    from spim_registration_amd import registration

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    r3 = lambda x: round(float(x), 3)

    def stats(fn, reps):
        for _ in range(a.warmup):
            timed(fn)
        runs = [timed(fn) for _ in range(reps)]
        ev, wall = [r[0] for r in runs], [r[1] for r in runs]
        return ({"median": r3(np.median(ev)), "min": r3(min(ev)), "max": r3(max(ev)),
                 "wall_median": r3(np.median(wall))}, runs[-1][2])

    def host_stats(fn, reps):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median": r3(np.median(t)), "min": r3(min(t)), "max": r3(max(t))}

    rows = []
    for n in a.sizes:
        ha, hb = lists(n)
        da, db = torch.from_numpy(ha).to("cuda:0"), torch.from_numpy(hb).to("cuda:0")
        assign_ms, (it, ir) = stats(lambda: registration.icp_assign(da, db), a.reps)
        loop_ms, run = stats(lambda: registration.icp(ha, hb, "rigid"), max(a.reps // 3, 3))
        fa, fb = ha.astype(np.float32), hb.astype(np.float32)
        kd_ms = host_stats(lambda: cKDTree(fa).query(fb, distance_upper_bound=5.0), max(a.reps // 3, 3))
        row = {
            "points_per_list": n,
            "icp_assign_call_ms": assign_ms, "icp_assign_matches": int(len(it)),
            "icp_run_ms": loop_ms, "icp_run_iterations": int(run[4]), "icp_run_assign_calls": int(run[4]) + 1,
            "icp_run_matches": int(len(run[0])), "icp_run_avg_error": float(run[3]),
            "pairs": n * n,
            "icp_pairs_per_s_whole_call": r3(n * n / (assign_ms["median"] * 1e-3) / 1e9),
            "host_ckdtree_build_query_ms": kd_ms,
            "ratio_ckdtree_over_icp_assign": r3(kd_ms["median"] / assign_ms["median"]),
        }
        if n == 16000:
            row["gh_neighbour_search_ms_both_lists"] = GH_KNN_MS_16000
            row["ratio_icp_assign_over_gh_neighbour_search"] = r3(assign_ms["median"] / GH_KNN_MS_16000)
            row["icp_assign_ps_per_pair"] = r3(assign_ms["median"] * 1e9 / (n * n))
            row["gh_neighbour_search_ps_per_pair"] = r3(GH_KNN_MS_16000 * 1e9 / (2 * n * n))
        rows.append(row)
    res = {
        "workload": "two device-resident lists per size, B = A's world beads (85 % each, 0.05 px noise) under a "
                    "rigid offset of 0.2 degrees about y and (0.8, -0.5, 0.3) px; whole C-ABI calls, results to the "
                    "host; max_distance 5; the icp run is registration.icp(model='rigid') from host arrays (uploads, "
                    "every assign call, the host fits and errors)",
        "reps": a.reps, "warmup": a.warmup,
        "timing": "median (min, max) of HIP event pairs around each call, ms; wall median beside it; the host "
                  "kd-tree by perf_counter on this machine's CPU, one thread",
        "icp_pairs_per_s_unit": "1e9 reference-target pairs per second",
        "tiles": list(registration.icp_tile_sizes()),
        "device": torch.cuda.get_device_name(0),
        "sizes": rows,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
