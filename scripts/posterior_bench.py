#!/usr/bin/env python3
"""Times mvc_amd.posterior.compare and .psm (host transfer included) beside a
numpy baseline on the same box, and writes profiles/posterior_bench.json.

Shapes:
  newsim  the reference's call (New_Simulation.R:47-60, n = 200): S = 1000
          saved samples of one parallel-mode chain, the table partition and
          each of the 5 views.
  large   n = 1M, S = 64, 64 clusters per draw (compare only).

The numpy baseline is the only earlier implementation there is (the parent
commit has none on the device): contingency tables by np.bincount, pair by
pair, and the PSM by accumulating t[:, None] == t[None, :] over the draws.
Its compare is timed on a random subset of the pairs and scaled to all of
them; the output says how many.  Device times are medians over repeats after
warm-up calls, each call ending in the library's own stream synchronise.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multiview-clustering_amd")]

import mvc_amd  # noqa: E402
from mvc_amd import data, posterior  # noqa: E402


def device_name():
    """Marketing name and ISA of device 0 as the driver reports them."""
    import torch
    p = torch.cuda.get_device_properties(0)
    return f"{p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs)"


def median_time(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 6) for t in ts]


def numpy_pair(a, b, n):
    """(B, VI) of two compacted labelings by np.bincount."""
    kb = int(b.max()) + 1
    tab = np.bincount(a.astype(np.int64) * kb + b, minlength=(int(a.max()) + 1) * kb).reshape(-1, kb)
    rows, cols = tab.sum(1), tab.sum(0)

    def c2(x):
        return int((x * (x - 1) // 2).sum())

    def h(x):
        x = x[x > 1].astype(np.float64)
        return float((x * np.log(x)).sum())

    return c2(rows) + c2(cols) - 2 * c2(tab), (h(rows) + h(cols) - 2.0 * h(tab.ravel())) / n / math.log(2.0)


def numpy_compare_scaled(lab, max_pairs, rng):
    """Seconds numpy needs for every pair, from a timed random subset; the
    subset's (s, t, B, VI) come back so the device's output can be checked."""
    S, n = lab.shape
    comp = np.stack([np.unique(r, return_inverse=True)[1].reshape(r.shape) for r in lab])
    iu = np.triu_indices(S, 1)
    total = iu[0].size
    pick = np.arange(total) if total <= max_pairs else rng.choice(total, max_pairs, replace=False)
    t0 = time.perf_counter()
    got = [(int(iu[0][k]), int(iu[1][k])) + numpy_pair(comp[iu[0][k]], comp[iu[1][k]], n) for k in pick]
    dt = time.perf_counter() - t0
    return dt * total / max(1, pick.size), got, int(total)


def check_subset(out, got):
    """The device's compare against the numpy pairs: B exactly, VI to 1e-12 relative."""
    for s, t, B, vi in got:
        assert int(out["binder"][s, t]) == B == int(out["binder"][t, s]), (s, t)
        assert math.isclose(out["vi"][s, t], vi, rel_tol=1e-12, abs_tol=1e-12), (s, t)


def numpy_psm(lab):
    n = lab.shape[1]
    cc = np.zeros((n, n), dtype=np.uint32)
    for t in lab:
        cc += t[:, None] == t[None, :]
    return cc / lab.shape[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_bench.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=1000, help="S of the newsim shape")
    ap.add_argument("--large-n", type=int, default=1_000_000)
    ap.add_argument("--large-s", type=int, default=64)
    ap.add_argument("--numpy-pairs", type=int, default=4000, help="pairs the numpy compare is timed on (newsim)")
    ap.add_argument("--numpy-pairs-large", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    result = {"device": device_name(), "warmup": args.warmup, "repeats": args.repeats,
              "timing": "host clock around calls that end in a stream synchronise; H2D / D2H copies included",
              "newsim": [], "large": None}

    y, truth = data.new_simulation(1999)
    S = args.samples
    res = mvc_amd.run_gibbs_cpp(y, S + 100, 100, 1, seed=1999, mode="parallel", quiet=True)
    for view in [None] + list(range(y.shape[0])):
        lab = posterior.draws(res, view=view, compact=True)
        t_cmp, all_cmp = median_time(lambda: posterior.compare(lab), args.warmup, args.repeats)
        t_psm, all_psm = median_time(lambda: posterior.psm(lab), args.warmup, args.repeats)
        np_cmp, got, total = numpy_compare_scaled(lab, args.numpy_pairs, rng)
        check_subset(posterior.compare(lab), got)
        np_psm, _ = median_time(lambda: numpy_psm(lab), 1, 3)
        assert np.array_equal(posterior.psm(lab), numpy_psm(lab))
        row = {"level": "tables" if view is None else f"view{view}", "S": int(lab.shape[0]), "n": int(lab.shape[1]),
               "max_clusters": int(lab.max()) + 1,
               "compare_s": round(t_cmp, 6), "compare_runs_s": all_cmp, "psm_s": round(t_psm, 6), "psm_runs_s": all_psm,
               "numpy_compare_s": round(np_cmp, 3),
               "numpy_compare_note": f"timed on {len(got)} of {total} pairs and scaled",
               "numpy_psm_s": round(np_psm, 6)}
        if view is not None:
            for loss in ("binder", "vi"):
                est, _, _ = posterior.point_estimate(lab, loss)
                row[f"ari_{loss}_estimate"] = mvc_amd.ari(est, truth[view])
            row["ari_last_draw"] = mvc_amd.ari(lab[-1], truth[view])
        result["newsim"].append(row)
        print(json.dumps(row), flush=True)

    n, S = args.large_n, args.large_s
    lab = rng.integers(0, 64, (S, n)).astype(np.int32)
    t_cmp, all_cmp = median_time(lambda: posterior.compare(lab), 1, max(3, args.repeats // 2))
    np_cmp, got, total = numpy_compare_scaled(lab, args.numpy_pairs_large, rng)
    check_subset(posterior.compare(lab), got)
    result["large"] = {"S": S, "n": n, "clusters": 64, "compare_s": round(t_cmp, 6), "compare_runs_s": all_cmp,
                       "numpy_compare_s": round(np_cmp, 3),
                       "numpy_compare_note": f"timed on {len(got)} of {total} pairs and scaled"}
    print(json.dumps(result["large"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out, "device": result["device"]}))


if __name__ == "__main__":
    main()
