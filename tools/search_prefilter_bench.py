"""A/B of the pre-filtered search against the exact fused search, in one process:

    A   reidmi_search_f32 (the exact search, unchanged)
    B   search(prefilter=True)'s device path: reidmi_search_prefiltered_f32, the read of the need
        count, and the exact search of the rows it marked
    B'  B without the fp16 copy of the gallery (what a resident copy would save): B minus the time
        of reidmi_rr_feat16 over the gallery, measured in the same alternation

on tools/search_ab.py's features (identity-clustered, L2-normalised; above 200 000 rows drawn on the
device), no labels, at Market (3368 x 15913) and MSMT17 (11659 x 82161) with D = 1280 and at
10 000 x 1 000 000 with D = 1792, k = 10, 50 and 128.  Before any timing B's lists are compared with
A's bit for bit.  Times are HIP events around each arm, warm, arms alternating; each row reports the
minimum and the median of the repetitions, and the pre-filter's statistics: the rows left to the
exact search (and their share), the largest survivor count, the exact distances computed.

    python tools/search_prefilter_bench.py [--out FILE] [--sizes market,msmt17,1m] [--ks 10,50,128]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_ab  # noqa: E402  (its feature construction and timing; it boots the package)

from multimodal_reid_amd import _lib as L, evaluate, synthetic as syn  # noqa: E402

SIZES = {"market": (3368, 15913, 1280, 751, 6, 10), "msmt17": (11659, 82161, 1280, 3060, 15, 5),
         "1m": (10000, 1000000, 1792, 20000, 15, 3)}  # Q, G, D, ids, cameras, repetitions


def run(name, ks, out):
    Q, G, D, ids, cams, reps = SIZES[name]
    qp, gp, _, _ = syn.labels(Q, G, num_ids=ids, num_cams=cams, seed=7, distractor_frac=0.1, junk_frac=0.02)
    search_ab.D = D
    q, g = search_ab.features(qp, gp, 7)
    s = L.stream()
    Gp, Dp = (G + 255) // 256 * 256, (D + 63) // 64 * 64
    g16 = torch.empty(Gp * Dp, device="cuda", dtype=torch.float16)
    ok = torch.ones(1, device="cuda", dtype=torch.int32)
    none = (None,) * 4
    for k in ks:
        if not L.load().reidmi_search_prefilter_applies(Q, G, D, k, 0):
            raise SystemExit(f"{name}, k = {k}: the pre-filter does not apply")
        nb = L.load().reidmi_search_workspace_bytes(Q, G, D, k)
        ws_a = torch.empty(nb, device="cuda", dtype=torch.uint8)
        ia, ib = (torch.empty(Q, k, device="cuda", dtype=torch.int32) for _ in range(2))
        va, vb = (torch.empty(Q, k, device="cuda", dtype=torch.float32) for _ in range(2))
        stats = {}

        def A():
            L.call("reidmi_search_f32", L.ptr(q), Q, D, L.ptr(g), G, D, D, k, *none, L.ptr(ia), L.ptr(va), k,
                   L.ptr(ws_a), nb, s)

        def B():
            stats.update(evaluate._search_prefiltered_into(q, g, k, none, ib, vb, k))

        def C():  # the gallery's fp16 copy alone
            L.call("reidmi_rr_feat16", L.ptr(g), G, D, D, L.ptr(g16), Gp, Dp, L.ptr(ok), s)

        A(), B(), C()
        torch.cuda.synchronize()
        if not (torch.equal(ia, ib) and torch.equal(va.view(torch.int32), vb.view(torch.int32))):
            raise SystemExit(f"{name}, k = {k}: the pre-filtered lists differ from the exact search's")
        t = {"A": [], "B": [], "C": []}
        for _ in range(reps):
            for key, fn in (("A", A), ("B", B), ("C", C)):
                t[key].append(search_ab.timed(fn))
        rec = {"size": name, "Q": Q, "G": G, "D": D, "k": k, "reps": reps, "bit_equal": True,
               "prefilter_workspace_bytes": L.load().reidmi_search_prefiltered_workspace_bytes(Q, G, D, k, 0)}
        for key, label in (("A", "exact"), ("B", "prefiltered"), ("C", "gallery_fp16_copy")):
            rec[label + "_ms_min"], rec[label + "_ms_median"] = round(min(t[key]), 3), round(float(np.median(t[key])), 3)
        rec["prefiltered_resident_ms_min"] = round(min(t["B"]) - min(t["C"]), 3)
        rec["speedup"] = round(min(t["A"]) / min(t["B"]), 3)
        rec["speedup_resident"] = round(min(t["A"]) / max(min(t["B"]) - min(t["C"]), 1e-6), 3)
        rec.update({"need_rows": stats["need_rows"], "need_share": round(stats["need_rows"] / Q, 4),
                    "max_survivors": stats["max_survivors"], "rescored": stats["rescored"],
                    "rescored_per_row": round(stats["rescored"] / Q, 1)})
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        del ws_a
    del q, g, g16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "search_prefilter_bench.txt"))
    ap.add_argument("--sizes", default="market,msmt17,1m")
    ap.add_argument("--ks", default="10,50,128")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_prefilter_bench: needs the GPU (there is nothing to time without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/search_prefilter_bench.py on {torch.cuda.get_device_name(0)}: A = reidmi_search_f32 (exact), "
                  "B = the pre-filtered search with its fallback, gallery_fp16_copy = reidmi_rr_feat16 of the gallery "
                  "alone (B' = B - that); HIP events, warm, alternating\n")
        for name in a.sizes.split(","):
            run(name, [int(k) for k in a.ks.split(",")], out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
