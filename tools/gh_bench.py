"""Geometric hashing candidate matching time: descriptors (spim_gh_descriptors) and matching
(spim_gh_match) for 1k, 4k and 16k points per list, device resident, beside
``rgldm_candidates`` (spim_rgldm_match, reference defaults 3 / 1 / 3 / 50) on the same lists
in the same run.

    python tools/gh_bench.py [--sizes 1000 4000 16000] [--reps 7] [--warmup 2]
                             [--out profiles/gh_bench.json]

List B is list A rotated 45 degrees about y and shifted, with 85 % of the world beads in each
and 0.05 px of noise, so geometric hashing finds candidates and RGLDM (translation invariant)
finds next to none.  Each call returns after its stream has drained and its results are on the
host; a timed call is bracketed by two HIP events on the caller's stream (wall clock beside
it), the median over --reps is reported.  A whole spim_gh_match call holds the finite check,
the neighbour search and descriptors of both lists, matching, merge and compaction; the
descriptor call the neighbour search and descriptors of one list.  The matching model counts
per descriptor pair 6 float subtractions, 6 float products, 6 widenings and 5 double additions.
Prints one JSON line and writes it to --out.
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


def lists(n: int, seed: int = 20140611, box: float = 768.0):
    rng = np.random.default_rng(seed + n)
    side = box * (n / 20000.0) ** (1.0 / 3.0)          # the bead density of a C4 view at every size
    world = rng.uniform(0.0, side, (int(n / 0.85) + 1, 3))
    a = world[rng.permutation(len(world))[:n]] + rng.uniform(-0.05, 0.05, (n, 3))
    b = world[rng.permutation(len(world))[:n]] + rng.uniform(-0.05, 0.05, (n, 3))
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.ascontiguousarray(a), np.ascontiguousarray(b @ rot.T + [13.0, -21.0, 8.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000, 16000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gh_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
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

    def median(fn):
        for _ in range(a.warmup):
            timed(fn)
        runs = [timed(fn) for _ in range(a.reps)]
        return float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs])), runs[-1][2]

    r3 = lambda x: round(float(x), 3)
    rows = []
    for n in a.sizes:
        ha, hb = lists(n)
        da, db = torch.from_numpy(ha).to("cuda:0"), torch.from_numpy(hb).to("cuda:0")
        desc_ms, desc_wall, _ = median(lambda: registration.gh_descriptors(da))
        gh_ms, gh_wall, gh = median(lambda: registration.gh_candidates(da, db))
        rg_ms, rg_wall, rg = median(lambda: registration.rgldm_candidates(da, db))
        match_ms = max(gh_ms - 2.0 * desc_ms, 0.0)      # (the descriptor call also copies its results out)
        rows.append({
            "points_per_list": n,
            "gh_descriptors_ms": r3(desc_ms), "gh_descriptors_ms_wall": r3(desc_wall),
            "gh_match_call_ms": r3(gh_ms), "gh_match_call_ms_wall": r3(gh_wall),
            "gh_match_call_minus_two_descriptor_calls_ms": r3(match_ms),
            "gh_candidates": int(len(gh[0])),
            "rgldm_match_call_ms": r3(rg_ms), "rgldm_match_call_ms_wall": r3(rg_wall),
            "rgldm_candidates": int(len(rg[0])),
            "descriptor_pairs": n * n,
            "gh_pairs_per_s_whole_call": r3(n * n / (gh_ms * 1e-3) / 1e9) if gh_ms > 0 else None,
        })
    res = {
        "workload": "two device-resident lists per size, B = A's world beads (85 % each, 0.05 px noise) rotated "
                    "45 degrees about y and shifted; whole C-ABI calls, results to the host; geometric hashing "
                    "defaults 10 / 50, RGLDM defaults 3 / 1 / 3 / 50",
        "reps": a.reps, "warmup": a.warmup, "timing": "median of HIP event pairs around each call; wall beside it",
        "gh_pairs_per_s_unit": "1e9 descriptor pairs per second",
        "tiles": list(registration.gh_tile_sizes()),
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
