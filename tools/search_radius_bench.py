"""Radius search against the unbounded search, in one process:

    search       evaluate.search_device(qf, gf, k)
    radius_*     evaluate.search_device(qf, gf, k, max_dist=tau) with a per-query tau that admits
                 about no item (below the query's nearest), about k items (the distance of its
                 k-th nearest) and every item (+inf)

on search_ab.py's features at Market (3368 x 15913) and MSMT17 (11659 x 82161) size, k = 50, no
labels.  Before any timing each radius result is compared bit for bit with the unbounded list cut at
tau.  Times are HIP events around each call, warm, the variants alternating; minimum and median.

    python tools/search_radius_bench.py [--out FILE] [--sizes market,msmt17] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_ab  # noqa: E402
from search_ab import evaluate, syn  # noqa: E402


def run(name, reps, out):
    Q, G, k, ids, cams, _ = search_ab.SIZES[name]
    qp, gp, _, _ = syn.labels(Q, G, num_ids=ids, num_cams=cams, seed=7, distractor_frac=0.1, junk_frac=0.02)
    q, g = search_ab.features(qp, gp, 7)
    idx, dist = evaluate.search_device(q, g, k)
    inf = torch.full((Q,), float("inf"), device="cuda")
    taus = {"radius_none": torch.nextafter(dist[:, 0], -inf), "radius_k": dist[:, k - 1].clone(), "radius_all": inf}
    variants = {"search": lambda: evaluate.search_device(q, g, k)}
    hits = {}
    for n, tau in taus.items():
        variants[n] = lambda tau=tau: evaluate.search_device(q, g, k, max_dist=tau)
        ri, rd = variants[n]()
        keep = dist <= tau[:, None]
        want_i = torch.where(keep, idx, torch.full_like(idx, -1))
        want_d = torch.where(keep, dist, torch.full_like(dist, float("inf")))
        if not (torch.equal(ri, want_i) and torch.equal(rd.view(torch.int32), want_d.view(torch.int32))):
            raise SystemExit(f"{name}: {n} differs from the unbounded list cut at tau")
        hits[n] = float((ri >= 0).sum(1).float().mean())
    t = {n: [] for n in variants}
    for _ in range(reps):
        for n, fn in variants.items():
            t[n].append(search_ab.timed(fn))
    rec = {"size": name, "Q": Q, "G": G, "D": search_ab.D, "k": k, "reps": reps, "bit_equal": True}
    for n in variants:
        rec[n + "_ms_min"], rec[n + "_ms_median"] = round(min(t[n]), 3), round(float(np.median(t[n])), 3)
        if n != "search":
            rec[n + "_mean_hits"] = round(hits[n], 2)
            rec[n + "_time_over_search"] = round(min(t[n]) / min(t["search"]), 3)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "search_radius_bench.txt"))
    ap.add_argument("--sizes", default="market,msmt17")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_radius_bench: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/search_radius_bench.py on {torch.cuda.get_device_name(0)}: evaluate.search_device with "
                  "max_dist against the unbounded search; HIP events, warm, alternating\n")
        for name in a.sizes.split(","):
            run(name, a.reps, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
