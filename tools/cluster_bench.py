"""DBSCAN from the features against the distance work its three passes imply, in one process and
one build:

    dbscan     cluster.dbscan_device(x, eps, min_samples)                     (reidmi_dbscan_f32)
    sweeps     three back-to-back sweeps of evaluate.euclidean_distance_device(x[band], x) over
               row bands of x into one reused buffer: the N x N x D distance work of the count,
               union and border passes, with the matrix stores the clustering does not make (the
               bands are needed because the matrix itself does not fit at 100 000 rows)
    sklearn    where scikit-learn is importable and N <= --sklearn-max-n: DBSCAN(metric=
               "precomputed") on the host, on the matrix of one such sweep (clamped at 0, zero
               diagonal); its labels are compared with the GPU's before its time is reported

on identity-clustered, L2-normalised features drawn on the device (synthetic.features'
construction: N / 20 identities, `--noise` the scatter around an identity's centre).  eps is the
squared distance at 0.6 of the cosine two crops of one identity have on average, 2 - 1.2 / (1 +
noise^2).  Times are HIP events around each call, warm, the variants alternating; the record has
the minimum and the median of the repetitions, the workspace and the peak of the device memory
allocated during a call above what was allocated before it.

    python tools/cluster_bench.py [--sizes 20000x1792,100000x1792] [--reps 3] [--noise 2.0]
                                  [--min-samples 4] [--band-rows 2048] [--sklearn-max-n 20000] [--out FILE]

--jaccard [--eps 0.6] [--k1 30] [--k2 6] measures the clustering on the k-reciprocal Jaccard distance
instead (run_jaccard): the three passes of reidmi_dbscan_jaccard alone, the re-rank stages that feed
them, the share of (row, chunk) workgroups that return before the walk, and scikit-learn on the dense
matrix of cluster.jaccard_distance_device where N <= --sklearn-max-n.  --sort-ids puts an identity's
crops in adjacent rows (the default is a random order), which is what the early return depends on.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()
from multimodal_reid_amd import cluster, evaluate  # noqa: E402


def features(N, D, ids, noise, seed, sort_ids=False):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pids = torch.randint(0, ids, (N,), device="cuda", generator=gen)
    if sort_ids:  # the crops of an identity in adjacent rows, as a gallery listed by identity has them
        pids = pids.sort().values
    centres = torch.randn(ids, D, device="cuda", generator=gen)
    x = torch.empty(N, D, device="cuda")
    for r0 in range(0, N, 1 << 16):
        p = pids[r0:r0 + (1 << 16)]
        x[r0:r0 + len(p)] = centres[p] + noise * torch.randn(len(p), D, device="cuda", generator=gen)
    return evaluate.l2_normalize_device(x)


def measured(fn):
    """(milliseconds by HIP events, peak bytes allocated during fn above those before it, result)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - before, res


def host_matrix(x, band_rows):
    N = x.shape[0]
    dm = np.empty((N, N), np.float32)
    for r0 in range(0, N, band_rows):
        dm[r0:r0 + band_rows] = evaluate.euclidean_distance_device(x[r0:r0 + band_rows], x).cpu().numpy()
    np.maximum(dm, 0, out=dm)
    np.fill_diagonal(dm, 0)
    return dm


def run(N, D, reps, noise, min_samples, band_rows, sklearn_max_n, out):
    x = features(N, D, max(2, N // 20), noise, 7)
    eps = float(np.float32(2.0 - 1.2 / (1.0 + noise * noise)))
    band = torch.empty((min(band_rows, N), N), device="cuda", dtype=torch.float32)

    def sweeps():
        for _ in range(3):
            for r0 in range(0, N, band_rows):
                rows = min(band_rows, N - r0)
                evaluate.euclidean_distance_device(x[r0:r0 + rows], x, out=band[:rows])

    variants = {"dbscan": lambda: cluster.dbscan_device(x, eps, min_samples), "sweeps": sweeps}
    t, peak = {n: [] for n in variants}, {}
    for name, fn in variants.items():  # warm
        _, peak[name], _ = measured(fn)
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(measured(fn)[0])
    labels, core, counts = (v.cpu().numpy() for v in cluster.dbscan_device(x, eps, min_samples))
    again = cluster.dbscan_device(x, eps, min_samples)[0].cpu().numpy()
    rec = {"N": N, "D": D, "eps": eps, "min_samples": min_samples, "noise": noise, "reps": reps,
           "n_clusters": int(labels.max()) + 1, "noise_points": int((labels < 0).sum()),
           "core_points": int(core.sum()), "mean_neighbours": round(float(counts.mean()), 2),
           "two_runs_equal": bool(np.array_equal(labels, again)), "matrix_bytes": 4 * N * N,
           "workspace_bytes": int(evaluate._lib.load().reidmi_dbscan_workspace_bytes(N, D))}
    for name in variants:
        rec[name + "_ms_min"] = round(min(t[name]), 3)
        rec[name + "_ms_median"] = round(float(np.median(t[name])), 3)
        rec[name + "_peak_bytes_above_features"] = int(peak[name])
    rec["dbscan_time_over_sweeps"] = round(float(np.median(t["dbscan"]) / np.median(t["sweeps"])), 3)
    if N <= sklearn_max_n:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            DBSCAN = None
        if DBSCAN is not None:
            del band
            dm = host_matrix(x, band_rows)
            t0 = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(dm)
            rec["sklearn_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["sklearn_labels_equal"] = bool(np.array_equal(sk.labels_.astype(np.int32), labels))
            rec["sklearn_time_over_dbscan"] = round(rec["sklearn_host_ms"] / float(np.median(t["dbscan"])), 1)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def early_exit_share(Vq, N, jch=8192):
    """The share of (row, chunk) workgroups of a Jaccard pass that return before the walk: those where
    no inverted list of one of V_qe[i]'s columns has an entry in the chunk, the chunk of i itself
    aside.  Computed from the CSR rows with torch, not by the kernels."""
    off, col, _ = Vq
    nch = -(-N // jch)
    row = torch.repeat_interleave(torch.arange(N, device=off.device), torch.diff(off))
    col = col.long()
    colhit = torch.zeros((N, nch), device=off.device, dtype=torch.bool)  # list(c) has an entry in chunk k
    colhit[col, row // jch] = True
    rowhit = torch.zeros((N, nch), device=off.device, dtype=torch.int32)
    for e0 in range(0, len(col), 1 << 22):
        rowhit.index_add_(0, row[e0:e0 + (1 << 22)], colhit[col[e0:e0 + (1 << 22)]].int())
    rowhit[torch.arange(N, device=off.device), torch.arange(N, device=off.device) // jch] = 1
    return 1.0 - float((rowhit > 0).sum().item()) / (N * nch), nch


def run_jaccard(N, D, reps, noise, min_samples, eps, k1, k2, sklearn_max_n, sort_ids, out):
    """--jaccard: DBSCAN on the k-reciprocal Jaccard distance.  `stages`: the re-rank stages that
    build V_qe and its inverted index (cluster._jaccard_stages: rank rows, V, V_qe, CSC, with their
    host synchronisations); `passes`: one reidmi_dbscan_jaccard call on those rows (bounds, count,
    union, border and the O(N) kernels); `whole`: cluster.dbscan_jaccard_device."""
    lib = evaluate._lib
    x = features(N, D, max(2, N // 20), noise, 7, sort_ids)
    n, dev, Vq, csc = cluster._jaccard_stages("cluster_bench", x, k1, k2, False, None)
    labels = torch.empty(N, device=dev, dtype=torch.int32)
    counts = torch.empty(N, device=dev, dtype=torch.int32)
    core = torch.empty(N, device=dev, dtype=torch.uint8)
    n_clusters = torch.empty(1, device=dev, dtype=torch.int32)
    nb = int(lib.load().reidmi_dbscan_jaccard_workspace_bytes(N))
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    sparse = [lib.ptr(t) for t in Vq + csc]

    def passes():
        lib.call("reidmi_dbscan_jaccard", N, *sparse, eps, min_samples, lib.ptr(labels), lib.ptr(counts), lib.ptr(core),
                 lib.ptr(n_clusters), lib.ptr(ws), nb, lib.stream())

    variants = {"stages": lambda: cluster._jaccard_stages("cluster_bench", x, k1, k2, False, None), "passes": passes,
                "whole": lambda: cluster.dbscan_jaccard_device(x, eps, min_samples, k1, k2)}
    t, peak = {v: [] for v in variants}, {}
    for name, fn in variants.items():  # warm
        _, peak[name], _ = measured(fn)
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(measured(fn)[0])
    passes()
    lab, cor, cnt = labels.cpu().numpy(), core.cpu().numpy(), counts.cpu().numpy()
    again = cluster.dbscan_jaccard_device(x, eps, min_samples, k1, k2)[0].cpu().numpy()
    skipped, nch = early_exit_share(Vq, N)
    nnz = int(Vq[0][-1].item())
    rec = {"mode": "jaccard", "rows": "sorted by identity" if sort_ids else "random order", "N": N, "D": D, "k1": k1, "k2": k2, "eps": eps, "eps_fp16": float(np.float16(eps)),
           "min_samples": min_samples, "noise": noise, "reps": reps, "n_clusters": int(n_clusters.item()),
           "noise_points": int((lab < 0).sum()), "core_points": int(cor.sum()),
           "mean_neighbours": round(float(cnt.mean()), 2), "two_runs_equal": bool(np.array_equal(lab, again)),
           "vqe_entries_per_row": round(nnz / N, 1), "chunks_per_row": nch,
           "workgroups_per_pass": N * nch, "early_exit_share": round(skipped, 4),
           "dense_matrix_bytes": 2 * N * N, "workspace_bytes": nb}
    for name in variants:
        rec[name + "_ms_min"] = round(min(t[name]), 3)
        rec[name + "_ms_median"] = round(float(np.median(t[name])), 3)
        rec[name + "_peak_bytes_above_features"] = int(peak[name])
    rec["passes_time_over_stages"] = round(float(np.median(t["passes"]) / np.median(t["stages"])), 3)
    if N <= sklearn_max_n:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            DBSCAN = None
        if DBSCAN is not None:
            del ws
            ms, _, dense = measured(lambda: cluster.jaccard_distance_device(x, k1, k2))
            rec["dense_rows_ms"] = round(ms, 3)
            dm = dense.cpu().numpy().astype(np.float32)  # fp16 values, exactly
            del dense
            np.maximum(dm, 0, out=dm)  # scikit-learn refuses negative entries; eps >= 0 sees no difference
            np.fill_diagonal(dm, 0)
            t0 = time.perf_counter()
            sk = DBSCAN(eps=float(np.float16(eps)), min_samples=min_samples, metric="precomputed").fit(dm)
            rec["sklearn_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["sklearn_labels_equal"] = bool(np.array_equal(sk.labels_.astype(np.int32), lab))
            rec["sklearn_time_over_whole"] = round(rec["sklearn_host_ms"] / float(np.median(t["whole"])), 1)
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jaccard", action="store_true", help="DBSCAN on the k-reciprocal Jaccard distance")
    ap.add_argument("--eps", type=float, default=0.6, help="--jaccard: the Jaccard radius")
    ap.add_argument("--k1", type=int, default=30)
    ap.add_argument("--k2", type=int, default=6)
    ap.add_argument("--sort-ids", action="store_true", help="--jaccard: an identity's crops in adjacent rows")
    ap.add_argument("--sizes", default="20000x1792,100000x1792")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=float, default=2.0)
    ap.add_argument("--min-samples", type=int, default=4)
    ap.add_argument("--band-rows", type=int, default=2048)
    ap.add_argument("--sklearn-max-n", type=int, default=20000)
    ap.add_argument("--out", default=None, help="default: profiles/cluster_bench.txt, or "
                    "profiles/cluster_jaccard_bench.txt with --jaccard")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench: needs the GPU (there is nothing to time without one)")
    a.out = a.out or os.path.join("profiles", "cluster_jaccard_bench.txt" if a.jaccard else "cluster_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.jaccard:
        with open(a.out, "w") as out:
            out.write(f"# tools/cluster_bench.py --jaccard on {torch.cuda.get_device_name(0)}: reidmi_dbscan_jaccard "
                      "(passes) against the re-rank stages that build its V_qe rows and their inverted index "
                      "(stages); HIP events, warm, alternating\n")
            for size in a.sizes.split(","):
                N, D = (int(v) for v in size.split("x"))
                run_jaccard(N, D, a.reps, a.noise, a.min_samples, a.eps, a.k1, a.k2, a.sklearn_max_n, a.sort_ids, out)
        return
    with open(a.out, "w") as out:
        out.write(f"# tools/cluster_bench.py on {torch.cuda.get_device_name(0)}: reidmi_dbscan_f32 against three "
                  "row-band sweeps of reidmi_distmat_f32 over the same rows; HIP events, warm, alternating\n")
        for size in a.sizes.split(","):
            N, D = (int(v) for v in size.split("x"))
            run(N, D, a.reps, a.noise, a.min_samples, a.band_rows, a.sklearn_max_n, out)


if __name__ == "__main__":
    main()
