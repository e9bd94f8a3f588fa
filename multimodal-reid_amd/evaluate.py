"""Drop-in for the reference's evaluate.py: same names, arguments, return types
and error behaviour, computed by libreidmi HIP kernels on the GPU.

    euclidean_distance(qf, gf) -> np.ndarray          evaluate.py:7-13
    cosine_similarity(qf, gf) -> np.ndarray           evaluate.py:16-26
    eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50)
                                   -> (cmc np.float32[max_rank], mAP np.float64)   evaluate.py:29-88
    R1_mAP_eval(num_query, max_rank=50, feat_norm=True, reranking=False)           evaluate.py:91-135

Verification and open-set statistics of a labelled split, from the features (reidmi_pair_stats_f32):
pair_stats, pair_stats_blocks, merge_pair_stats, PairStatsAccumulator, R1_mAP_eval.pair_stats, and on
their result verification_curve, threshold_at_far, tar_at_far, equal_error_rate, open_set_rates.

Beyond the reference: ranked search (search, search_blocks, search_sharded), and the step
between "the k nearest" and "the features I rank with" as one kernel (reidmi_combine_rows_f32):
expand_features (AQE / alpha-QE), database_augmentation (DBA), pool_features (multi-query and
tracklet pooling) and R1_mAP_eval(query_expansion=, db_augmentation=); and scoring without the
(Q, G) matrix (reidmi_eval_feat_f32 / reidmi_evf_*): eval_func_features, eval_features_blocks,
eval_features_sharded, mean_inp and R1_mAP_eval(matrix_free=True).

The *_device variants keep everything on the GPU (torch tensors in, torch tensors out)
and are what the fused pipeline (zero_shot_learning.py) uses.

Tie semantics: ranks inside groups of exactly equal distances are ordered by gallery
index (np.argsort(kind="stable")); the reference's unstable argsort orders such groups
in a host-dependent way.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _dev():
    if not torch.cuda.is_available():
        raise _lib.ReidmiError("no GPU visible: the libreidmi path runs on MI355X only")
    return torch.device("cuda", torch.cuda.current_device())


def _as_dev_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.to(device=_dev(), dtype=torch.float32).contiguous()


def _as_dev_i64(x):
    if isinstance(x, torch.Tensor):
        return x.to(device=_dev(), dtype=torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.int64)).to(_dev())


# --------------------------------------------------------------------- kernels
def l2_normalize_device(x):
    """torch.nn.functional.normalize(x, dim=1, p=2) (evaluate.py:114) on the GPU."""
    x = _as_dev_f32(x)
    n, d = x.shape
    y = torch.empty_like(x)
    ws = torch.empty(max(n, 1), device=x.device, dtype=torch.float32)
    _lib.call("reidmi_l2norm_f32", _lib.ptr(x), n, d, d, _lib.ptr(y), d, _lib.ptr(ws), _lib.stream())
    return y


def euclidean_distance_device(qf, gf, out=None, precision="fp32"):
    """(Q,G) fp32 tensor: ||q||^2 + ||g||^2 - 2 q.g.  precision "fp32" (default): exact fp32
    (fmaf chain over k), the reference's distances up to BLAS order; "fp16": the q.g products on
    the fp16 MFMA GEMM (reidmi_distmat_f16, the §8b reduced-precision mode; not bit-exact)."""
    if precision not in ("fp32", "fp16"):
        raise ValueError(f"euclidean_distance_device: precision must be 'fp32' or 'fp16', not {precision!r}")
    qf, gf = _as_dev_f32(qf), _as_dev_f32(gf)
    Q, D = qf.shape
    G = gf.shape[0]
    if out is None:
        out = torch.empty((Q, G), device=qf.device, dtype=torch.float32)
    if precision == "fp16":
        nb = _lib.load().reidmi_distmat_f16_workspace_bytes(Q, G, D)
        ws = torch.empty(max(nb, 1), device=qf.device, dtype=torch.uint8)
        _lib.call("reidmi_distmat_f16", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D,
                  _lib.ptr(out), out.stride(0), _lib.ptr(ws), nb, _lib.stream())
        return out
    ws = torch.empty(Q + G, device=qf.device, dtype=torch.float32)
    _lib.call("reidmi_distmat_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D,
              _lib.ptr(out), out.stride(0), _lib.ptr(ws), _lib.stream())
    return out


def topk_rows_device(x, k, row_div=None, with_values=False):
    """np.argsort(x, axis=1, kind='stable')[:, :k] on the GPU (any k <= columns)."""
    x = _as_dev_f32(x)
    rows, cols = x.shape
    idx = torch.empty((rows, k), device=x.device, dtype=torch.int32)
    val = torch.empty((rows, k), device=x.device, dtype=torch.float32) if with_values else None
    _lib.call("reidmi_topk_rows_f32", _lib.ptr(x), rows, cols, x.stride(0), _lib.ptr(row_div), k, _lib.ptr(idx),
              _lib.ptr(val), k, _lib.stream())
    return (idx, val) if with_values else idx


def _max_dist_rows(what, max_dist, Q):
    """max_dist as a host fp32 [Q] tensor (a number: the same radius for every query), or None.
    Checked before anything touches the GPU."""
    if max_dist is None:
        return None
    if isinstance(max_dist, torch.Tensor):
        t = max_dist.detach()
    else:
        try:
            t = torch.from_numpy(np.asarray(max_dist, dtype=np.float32))
        except (TypeError, ValueError):
            raise _lib.ReidmiError(f"{what}: max_dist must be a number or one number per query") from None
    if t.dim() == 0:
        return t.to(torch.float32).reshape(1).expand(Q)
    if tuple(t.shape) != (Q,):
        raise _lib.ReidmiError(f"{what}: max_dist must be a number or have shape [{Q}] (one radius per query), "
                               f"not {list(t.shape)}")
    return t.to(torch.float32)


# ------------------------------------------------------------- filtered search
# Which gallery items a query may match at all (reidmi_search_filter, include/reidmi.h).  Item j is
# admitted for query i iff every clause that is present holds:
#   valid        ItemAttrs.valid[j] != 0
#   camera mask  0 <= ItemAttrs.camids[j] < 64 and bit camids[j] of QueryFilter.cam_mask[i] is set
#   time window  time_range[i][0] <= ItemAttrs.times[j] <= time_range[i][1]
#   group        ItemAttrs.groups[j] != QueryFilter.groups[i]
# next to the label rule of the four label arrays (not (same pid and same camera)).  The kernels test
# the clauses where they test the label rule (csrc/admit.h): nothing is fetched and filtered later.
class ItemAttrs:
    """The gallery side of a filtered search: one entry per gallery row, each array optional.
    valid (bool / uint8): 0 withdraws the item.  camids, times, groups (integers): the item's camera
    for QueryFilter.cam_mask (0 .. 63), its time stamp for time_range, its group (a tracklet, a
    sequence of inference()'s seqs) for QueryFilter.groups.  Host arrays or device tensors."""

    def __init__(self, valid=None, camids=None, times=None, groups=None):
        self.valid, self.camids, self.times, self.groups = valid, camids, times, groups

    def __getitem__(self, rows):
        """The attributes of a block of gallery rows (a slice or an index array)."""
        return ItemAttrs(*(None if a is None else a[rows] for a in (self.valid, self.camids, self.times, self.groups)))


class QueryFilter:
    """The query side of a filtered search.  cam_mask: one int64 per query read as 64 bits, bit c set
    = camera c may match (cam_mask(), cross_camera_mask()).  time_range: [Q][2] integers (lo, hi), or
    one (lo, hi) pair for every query; both ends are inside the window.  groups: one integer per
    query, items of that group are left out (the query's own tracklet)."""

    def __init__(self, cam_mask=None, time_range=None, groups=None):
        self.cam_mask, self.time_range, self.groups = cam_mask, time_range, groups


def cam_mask(allowed):
    """The int64 whose bit c is set for every camera id c in ``allowed`` (0 .. 63)."""
    m = 0
    for c in allowed:
        c = int(c)
        if not 0 <= c < 64:
            raise _lib.ReidmiError(f"cam_mask: camera ids must be in [0, 64), not {c}")
        m |= 1 << c
    return np.uint64(m).astype(np.int64)


def cross_camera_mask(q_camids):
    """int64 [Q]: for every query every bit but its own camera's (cross-camera-only matching: items
    of the query's camera are dropped whatever their pid)."""
    c = np.asarray(q_camids.cpu() if isinstance(q_camids, torch.Tensor) else q_camids)
    if c.ndim != 1 or c.dtype.kind not in "iu":
        raise _lib.ReidmiError("cross_camera_mask: q_camids must be one integer per query")
    if c.size and (c.min() < 0 or c.max() >= 64):
        raise _lib.ReidmiError("cross_camera_mask: camera ids must be in [0, 64)")
    return (~(np.uint64(1) << c.astype(np.uint64))).astype(np.int64)


_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _filter_array(what, name, x, n, kinds="iu"):
    """x as a torch tensor of shape [n] and an integer (or, for valid, bool) dtype, where it is."""
    if not isinstance(x, torch.Tensor):
        try:
            a = np.asarray(x)
            if a.dtype.kind not in kinds:
                raise TypeError
            if a.dtype == np.uint64:
                a = a.astype(np.int64)  # the same 64 bits
            x = torch.from_numpy(np.ascontiguousarray(a))
        except (TypeError, ValueError):
            raise _lib.ReidmiError(f"{what}: {name} must be an integer array, one entry per row") from None
    allowed = (torch.bool, torch.uint8) if kinds == "biu" else _INT_DTYPES
    if x.dtype not in allowed:
        want = "bool or uint8" if kinds == "biu" else "an integer dtype"
        raise _lib.ReidmiError(f"{what}: {name} must have {want}, not {x.dtype}")
    if tuple(x.shape) != (n,):
        raise _lib.ReidmiError(f"{what}: {name} must have shape [{n}], not {list(x.shape)}")
    return x.detach()


class _Filter:
    """A checked filter: tensors (host or device) until to(), then device tensors the C struct points to."""
    NAMES = ("g_valid", "g_cam", "q_cam_mask", "g_time", "q_time_lo", "q_time_hi", "g_group", "q_group")

    def __init__(self, **kw):
        for n in self.NAMES:
            setattr(self, n, kw.get(n))

    def to(self, dev):
        f = _Filter()
        for n in self.NAMES:
            t = getattr(self, n)
            if t is not None:
                t = t.to(device=dev, dtype=torch.uint8 if n == "g_valid" else torch.int64).contiguous()
            setattr(f, n, t)
        return f

    def rows(self, rows):
        """The filter of a subset of the queries."""
        f = _Filter(**{n: getattr(self, n) for n in self.NAMES})
        for n in self.NAMES:
            if n.startswith("q_") and getattr(self, n) is not None:
                setattr(f, n, getattr(self, n)[rows].contiguous())
        return f

    def struct(self):
        s = _lib.structs("reidmi_filter.h")["reidmi_search_filter"]()
        for n in self.NAMES:
            t = getattr(self, n)
            setattr(s, n, None if t is None else t.data_ptr())
        return s


def _check_query_filter(what, q_filter, Q):
    """QueryFilter -> {q_cam_mask, q_time_lo, q_time_hi, q_group} tensors; host code only."""
    if q_filter is None:
        return {}
    if not isinstance(q_filter, QueryFilter):
        raise _lib.ReidmiError(f"{what}: q_filter must be an evaluate.QueryFilter")
    out = {}
    if q_filter.cam_mask is not None:
        out["q_cam_mask"] = _filter_array(what, "q_filter.cam_mask", q_filter.cam_mask, Q)
    if q_filter.time_range is not None:
        tr = q_filter.time_range
        if not isinstance(tr, torch.Tensor):
            try:
                a = np.asarray(tr)
                if a.dtype.kind not in "iu":
                    raise TypeError
                tr = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
            except (TypeError, ValueError):
                raise _lib.ReidmiError(f"{what}: q_filter.time_range must hold integers") from None
        if tr.dtype not in _INT_DTYPES:
            raise _lib.ReidmiError(f"{what}: q_filter.time_range must have an integer dtype, not {tr.dtype}")
        if tuple(tr.shape) == (2,):
            tr = tr.reshape(1, 2).expand(Q, 2)
        if tuple(tr.shape) != (Q, 2):
            raise _lib.ReidmiError(f"{what}: q_filter.time_range must be one (lo, hi) pair or have shape [{Q}, 2], "
                                   f"not {list(tr.shape)}")
        out["q_time_lo"], out["q_time_hi"] = tr[:, 0].detach(), tr[:, 1].detach()
    if q_filter.groups is not None:
        out["q_group"] = _filter_array(what, "q_filter.groups", q_filter.groups, Q)
    return out


_CLAUSES = (("camera mask", "g_attrs.camids", "g_cam", "q_filter.cam_mask", "q_cam_mask"),
            ("time window", "g_attrs.times", "g_time", "q_filter.time_range", "q_time_lo"),
            ("group", "g_attrs.groups", "g_group", "q_filter.groups", "q_group"))


def _check_filter(what, g_attrs, G, qside):
    """ItemAttrs of G rows and a checked query side -> _Filter, or None when neither holds anything.
    Raises for a clause with one side only and, with a camera mask, for a camera id outside [0, 64):
    on the host for a host array, one device reduction and one synchronisation for a device tensor."""
    if g_attrs is None and not qside:
        return None
    if g_attrs is not None and not isinstance(g_attrs, ItemAttrs):
        raise _lib.ReidmiError(f"{what}: g_attrs must be an evaluate.ItemAttrs")
    g = {}
    if g_attrs is not None:
        if g_attrs.valid is not None:
            g["g_valid"] = _filter_array(what, "g_attrs.valid", g_attrs.valid, G, "biu")
        for name, key in (("camids", "g_cam"), ("times", "g_time"), ("groups", "g_group")):
            if getattr(g_attrs, name) is not None:
                g[key] = _filter_array(what, "g_attrs." + name, getattr(g_attrs, name), G)
    for clause, gname, gkey, qname, qkey in _CLAUSES:
        if (gkey in g) != (qkey in qside):
            have, miss = (gname, qname) if gkey in g else (qname, gname)
            raise _lib.ReidmiError(f"{what}: the {clause} clause has {have} but no {miss}")
    if "g_cam" in g and G:
        c = g["g_cam"]
        if bool(((c < 0) | (c >= 64)).any()):
            raise _lib.ReidmiError(f"{what}: g_attrs.camids must be in [0, 64) when a camera mask is given")
    if not g and not qside:
        return None
    return _Filter(**g, **qside)


def search_device(qf, gf, k, q_pids=None, q_camids=None, g_pids=None, g_camids=None, with_dist=True, max_dist=None,
                  prefilter=False, return_stats=False, _sample_stride=0, g_attrs=None, q_filter=None):
    """The k nearest gallery rows of every query row (reidmi_search_f32: the selection runs in the
    distance kernel's epilogue, no (Q,G) matrix): (idx int32 [Q][k], dist fp32 [Q][k] or None) on the
    GPU, bit for bit euclidean_distance_device + topk_rows_device.  With the four label arrays, gallery
    items of the query's pid and camera are skipped (evaluate.py:46-48) and short rows are padded with
    -1 / +inf.  1 <= k <= min(G, 128).
    max_dist (a number, or a [Q] array or tensor; default None: no limit, reidmi_search_f32 as ever):
    only items at a distance <= max_dist of their query are ranked (reidmi_search_bounded_f32's radius
    form: the limit is the kernel's first threshold, nothing is filtered afterwards).  Rows are padded
    with -1 / +inf, so (idx >= 0).sum(1) is the number of hits, up to k; a query with nothing within
    its radius gets an all-padded row.  A NaN or -inf radius admits nothing.
    prefilter (default False): the same lists, bit for bit, through reidmi_search_prefiltered_f32: an
    fp16 MFMA product bounds every distance, and only the few items per row that can still be among
    the k nearest are computed exactly.  Where the pre-filter does not apply (a small gallery or D:
    reidmi_search_prefilter_applies) the exact search runs instead; rows it cannot decide (distances
    too concentrated, features beyond fp16's range) are searched exactly afterwards.  Reading how many
    such rows there are is this path's one synchronisation with the GPU.  Faster on large galleries,
    slower on small ones.
    return_stats: also return a dict: applied (the pre-filtered call ran), need_rows (rows it left to
    the exact search), max_survivors, rescored (exact distances it computed), range_failed.
    g_attrs (ItemAttrs) / q_filter (QueryFilter): the filtered search (reidmi_search_filtered_f32).
    Only admitted items are ranked: the clauses of the table above ItemAttrs, tested in the kernel
    next to the label rule, with or without labels, max_dist and prefilter; a query with fewer than
    k admitted items gets a short row, one with none an all-padded row.  A clause needs both its
    sides (valid has the gallery side only); shapes, dtypes and the pairing are checked before
    anything touches the GPU, and with a camera mask the gallery's camera ids must lie in [0, 64):
    for a device tensor that check costs one device reduction and one synchronisation, for a host
    array nothing.  With prefilter, the rows it marks go through the filtered exact search with the
    same filter; a selective filter starves the pre-filter's 1/16 sample and overflows its survivor
    lists, so most rows fall back (need_rows in return_stats) and the exact filtered search alone is
    the faster call.  Both None: the unfiltered kernels, as before."""
    tau = _max_dist_rows("search", max_dist, qf.shape[0])
    flt = _check_filter("search", g_attrs, gf.shape[0], _check_query_filter("search", q_filter, qf.shape[0]))
    qf, gf = _as_dev_f32(qf), _as_dev_f32(gf)
    flt = None if flt is None else flt.to(qf.device)
    Q, D = qf.shape
    G = gf.shape[0]
    labels = (q_pids, q_camids, g_pids, g_camids)
    given = sum(a is not None for a in labels)
    if given not in (0, 4):
        raise _lib.ReidmiError("search: pass all four label arrays or none")
    qp, qc, gp, gc = (_as_dev_i64(a) for a in labels) if given else (None,) * 4
    k = int(k)
    idx = torch.empty((Q, max(k, 0)), device=qf.device, dtype=torch.int32)
    dist = torch.empty((Q, max(k, 0)), device=qf.device, dtype=torch.float32) if with_dist else None
    bound = None if tau is None else (tau.to(qf.device).contiguous(), None, 1, 0)
    stats = dict(_NO_PREFILTER)
    if prefilter:
        stats = _search_prefiltered_into(qf, gf, k, (qp, qc, gp, gc), idx, dist, max(k, 1), bound, _sample_stride,
                                         flt)
    else:
        _search_into(qf, gf, k, (qp, qc, gp, gc), idx, dist, max(k, 1), bound, flt)
    return (idx, dist, stats) if return_stats else (idx, dist)


def _search_into(qf, gf, k, labels, idx, dist, ldo, bound=None, flt=None):
    """reidmi_search_f32 of device features (and device labels, or four Nones) into rows of pitch ldo.
    bound: None, or reidmi_search_bounded_f32's (bound_dist, bound_idx or None, ldb, index_base), the
    first two device tensors (or views) whose element i * ldb belongs to query i.  flt: None, or a
    _Filter on the device (reidmi_search_filtered_f32)."""
    Q, D = qf.shape
    G = gf.shape[0]
    nb = _lib.load().reidmi_search_workspace_bytes(Q, G, D, k)
    ws = torch.empty(max(nb, 16), device=qf.device, dtype=torch.uint8)
    if flt is not None:
        bd, bi, ldb, base = (None, None, 1, 0) if bound is None else bound
        _lib.call("reidmi_search_filtered_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D, k,
                  *(_lib.ptr(a) for a in labels), ctypes.byref(flt.struct()), _lib.ptr(bd), _lib.ptr(bi), ldb, base,
                  _lib.ptr(idx), _lib.ptr(dist), ldo, _lib.ptr(ws), nb, _lib.stream())
        return
    if bound is None:
        _lib.call("reidmi_search_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D, k,
                  *(_lib.ptr(a) for a in labels), _lib.ptr(idx), _lib.ptr(dist), ldo, _lib.ptr(ws), nb, _lib.stream())
        return
    bd, bi, ldb, base = bound
    _lib.call("reidmi_search_bounded_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D, k,
              *(_lib.ptr(a) for a in labels), _lib.ptr(bd), _lib.ptr(bi), ldb, base, _lib.ptr(idx), _lib.ptr(dist),
              ldo, _lib.ptr(ws), nb, _lib.stream())


_NO_PREFILTER = {"applied": False, "need_rows": 0, "max_survivors": 0, "rescored": 0, "range_failed": 0}


def _search_prefiltered_into(qf, gf, k, labels, idx, dist, ldo, bound=None, sample_stride=0, flt=None):
    """_search_into through reidmi_search_prefiltered_f32 (same arguments; idx / dist are [Q][>= k]
    tensors of pitch ldo): the exact search where the pre-filter does not apply, else the pre-filtered
    call, then the exact search of the rows it marked in need, scattered back.  Returns search_device's
    stats dict.  stats.tolist() below is the one synchronisation."""
    Q, D = qf.shape
    G = gf.shape[0]
    L = _lib.load()
    if Q == 0 or not L.reidmi_search_prefilter_applies(Q, G, D, k, sample_stride):
        _search_into(qf, gf, k, labels, idx, dist, ldo, bound, flt)
        return dict(_NO_PREFILTER)
    nb = L.reidmi_search_prefiltered_workspace_bytes(Q, G, D, k, sample_stride)
    ws = torch.empty(nb, device=qf.device, dtype=torch.uint8)
    need = torch.empty(Q, device=qf.device, dtype=torch.int32)
    stats = torch.empty(4, device=qf.device, dtype=torch.int32)
    bd, bi, ldb, base = (None, None, 1, 0) if bound is None else bound
    if flt is None:
        _lib.call("reidmi_search_prefiltered_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D, k,
                  *(_lib.ptr(a) for a in labels), _lib.ptr(bd), _lib.ptr(bi), ldb, base, _lib.ptr(idx), _lib.ptr(dist),
                  ldo, sample_stride, _lib.ptr(need), _lib.ptr(stats), _lib.ptr(ws), nb, _lib.stream())
    else:
        _lib.call("reidmi_search_prefiltered_filtered_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G,
                  gf.stride(0), D, k, *(_lib.ptr(a) for a in labels), ctypes.byref(flt.struct()), _lib.ptr(bd),
                  _lib.ptr(bi), ldb, base, _lib.ptr(idx), _lib.ptr(dist), ldo, sample_stride, _lib.ptr(need),
                  _lib.ptr(stats), _lib.ptr(ws), nb, _lib.stream())
    st = stats.tolist()
    if st[0]:
        rows = torch.nonzero(need).squeeze(1)
        n = rows.numel()
        sub_lab = labels if labels[0] is None else (labels[0][rows], labels[1][rows], labels[2], labels[3])
        sub_bound = None if bound is None else (bd[rows].contiguous(), None if bi is None else bi[rows].contiguous(),
                                                1, base)
        sidx = torch.empty((n, k), device=qf.device, dtype=torch.int32)
        sdist = None if dist is None else torch.empty((n, k), device=qf.device, dtype=torch.float32)
        _search_into(qf[rows].contiguous(), gf, k, sub_lab, sidx, sdist, k, sub_bound,
                     None if flt is None else flt.rows(rows))
        idx[rows, :k] = sidx
        if dist is not None:
            dist[rows, :k] = sdist
    return {"applied": True, "need_rows": st[0], "max_survivors": st[1], "rescored": st[2], "range_failed": st[3]}


def search(qf, gf, k, q_pids=None, q_camids=None, g_pids=None, g_camids=None, with_dist=True, max_dist=None,
           prefilter=False, g_attrs=None, q_filter=None):
    """search_device, returned as numpy arrays."""
    idx, dist = search_device(qf, gf, k, q_pids, q_camids, g_pids, g_camids, with_dist, max_dist, prefilter,
                              g_attrs=g_attrs, q_filter=q_filter)
    return idx.cpu().numpy(), (dist.cpu().numpy() if with_dist else None)


def merge_lists_device(in_idx, in_dist, k, base=None, with_dist=True):
    """Joins S partial rank lists per query (reidmi_search_merge_f32): in_idx int32 / in_dist fp32
    [S][Q][k_in] device tensors of the same strides, rows as search_device writes them (padding -1 /
    +inf); base: device int64 [S], the global index of list s's index 0 (None: all zero).  Returns
    (idx int32 [Q][k], dist fp32 [Q][k] or None): the k smallest present entries by (distance, global
    index), whatever the order of the lists."""
    S, Q, k_in = in_idx.shape
    if in_dist.shape != in_idx.shape or in_dist.stride() != in_idx.stride() or in_idx.stride(2) != 1:
        raise _lib.ReidmiError("merge_lists: in_idx and in_dist must share one [S][Q][k_in] layout with unit entries")
    _lib.require_cuda(in_idx, in_dist, base)
    k = int(k)
    idx = torch.empty((Q, max(k, 0)), device=in_idx.device, dtype=torch.int32)
    dist = torch.empty((Q, max(k, 0)), device=in_idx.device, dtype=torch.float32) if with_dist else None
    _lib.call("reidmi_search_merge_f32", _lib.ptr(in_idx), _lib.ptr(in_dist), S, Q, k_in, in_idx.stride(0),
              in_idx.stride(1), _lib.ptr(base), k, _lib.ptr(idx), _lib.ptr(dist), max(k, 1), _lib.stream())
    return idx, dist


def _labels_given(what, *labels):
    given = sum(a is not None for a in labels)
    if given not in (0, len(labels)):
        raise _lib.ReidmiError(f"{what}: pass all {len(labels)} label arrays or none")
    return bool(given)


# carry_bound's default in SearchAccumulator / search_blocks.  On: at 10 000 x 1 000 000, D = 1792 it was
# no slower at any measured row (1 / 8 / 64 blocks, k = 10 and 128: 1.00 / 0.93 / 0.79 and 1.00 / 0.69 /
# 0.38 of the time without it; DESIGN.md §5, profiles/search_blocks_carry_bench.txt).
CARRY_BOUND_DEFAULT = True


class SearchAccumulator:
    """search_device over a gallery that arrives in blocks: add() each block (a device or host
    tensor, or a numpy array; a host block is on the device for the call only), then result().  Each
    block is searched by reidmi_search_f32 and its list joined with the carried one by
    reidmi_search_merge_f32 (S = 2, the block's indices moved by the number of items before it).  A
    (query, item) distance does not depend on the block the item came in, and the join orders by
    (distance, global index), so the result is bit for bit search_device(qf, torch.cat(blocks), k,
    ...) for every way of cutting the gallery.  With q_pids / q_camids every block comes with its
    g_pids / g_camids (evaluate.py:46-48's removal), without them none does.
    Carried state: three [Q][k] lists of 8 bytes an entry (the carried one, the block's, the join's
    output: the join never writes what it reads) and, during add(), the workspace of one block's
    search; nothing grows with the gallery.
    carry_bound: from the second block on, search each block under the carried list's k-th key
    (reidmi_search_bounded_f32's key form: column k-1 of the carried list in place, index_base = the
    items before the block), so that a block's workgroups start with the threshold the earlier blocks
    reached and append only what can enter the carried list; a not-yet-full row holds +inf / -1 there,
    which admits everything.  The join and the result are the same either way.  Default True: measured
    no slower at any row of DESIGN.md §5's table and up to 2.6 times faster (64 blocks, k = 128);
    False searches every block unbounded, as before the bounded search existed.
    max_dist (a number or one per query): only items within that distance of their query are ranked,
    rows padded with -1 / +inf as search_device(max_dist=) pads them.  It bounds the first block (the
    radius form) and, with carry_bound, every row whose carried list is not yet full; a full row's
    k-th key is at or below the radius, so it is the tighter bound and takes over.  No block is ever
    searched under a bound that admits more than the radius.
    prefilter (default False): every block's search goes through search_device(prefilter=True)'s
    path, the carried bound and the radius as its bound arguments; a block too small for the
    pre-filter takes the exact search.  The result is the same, bit for bit.
    q_filter (QueryFilter): the filtered search; every add() then brings the block's g_attrs
    (ItemAttrs) with the gallery side of each of its clauses (g_attrs.valid needs no q_filter), checked
    as search_device checks them.  Bit for bit search_device(..., g_attrs=, q_filter=) over the
    concatenation, carry_bound on or off: the carried key is an admitted item's, so it bounds admitted
    items exactly.  A block in which nothing is admitted adds nothing."""

    def __init__(self, qf, k, q_pids=None, q_camids=None, with_dist=True, carry_bound=CARRY_BOUND_DEFAULT,
                 max_dist=None, prefilter=False, _sample_stride=0, q_filter=None):
        self.prefilter, self._sample_stride = bool(prefilter), int(_sample_stride)
        self._qside = _check_query_filter("SearchAccumulator", q_filter, qf.shape[0])
        if not isinstance(carry_bound, (bool, np.bool_)):
            raise _lib.ReidmiError("SearchAccumulator: carry_bound must be True or False")
        tau = _max_dist_rows("SearchAccumulator", max_dist, qf.shape[0])
        self.carry_bound = bool(carry_bound)
        self.qf = _as_dev_f32(qf)
        self._tau = None if tau is None else tau.to(self.qf.device).contiguous()
        self.k = int(k)
        if not 1 <= self.k <= 128:
            raise _lib.ReidmiError("SearchAccumulator: need 1 <= k <= 128")
        self.labels = _labels_given("SearchAccumulator", q_pids, q_camids)
        self.qp, self.qc = (_as_dev_i64(q_pids), _as_dev_i64(q_camids)) if self.labels else (None, None)
        self.with_dist = with_dist
        Q, dev = self.qf.shape[0], self.qf.device
        # slot 1 takes each block's list; the carried list and the join's output alternate between 0 and 2
        self._idx = torch.full((3, Q, self.k), -1, device=dev, dtype=torch.int32)
        self._dist = torch.full((3, Q, self.k), float("inf"), device=dev, dtype=torch.float32)
        self._carried = 0
        self.count = 0  # gallery items added so far

    def add(self, gf_block, g_pids=None, g_camids=None, g_attrs=None):
        if _labels_given("SearchAccumulator.add", g_pids, g_camids) != self.labels:
            raise _lib.ReidmiError("SearchAccumulator.add: gallery labels go with query labels: every block has "
                                   "them or none has")
        rows = int(gf_block.shape[0])
        flt = _check_filter("SearchAccumulator.add", g_attrs, rows, self._qside)
        if rows == 0:
            return
        gf = _as_dev_f32(gf_block)
        flt = None if flt is None else flt.to(gf.device)
        lab = (self.qp, self.qc, _as_dev_i64(g_pids), _as_dev_i64(g_camids)) if self.labels else (None,) * 4
        if self.labels and (lab[2].numel() != rows or lab[3].numel() != rows):
            raise _lib.ReidmiError("SearchAccumulator.add: one label per gallery row")
        if self.count + rows >= 2 ** 31:
            raise _lib.ReidmiError("SearchAccumulator: gallery indices must fit int32")
        kb = min(self.k, rows)
        slot = self._carried if self.count == 0 else 1
        if kb < self.k:  # the search writes [0, kb) of a row
            self._idx[slot].fill_(-1)
            self._dist[slot].fill_(float("inf"))
        if self.prefilter:
            _search_prefiltered_into(self.qf, gf, kb, lab, self._idx[slot], self._dist[slot], self.k, self._bound(),
                                     self._sample_stride, flt)
        else:
            _search_into(self.qf, gf, kb, lab, self._idx[slot], self._dist[slot], self.k, self._bound(), flt)
        if self.count:
            c = self._carried
            lo = min(c, 1)  # lists lo and lo + 1
            base = torch.tensor([0, self.count] if c == 0 else [self.count, 0], dtype=torch.int64,
                                device=self.qf.device)
            Q, k = self.qf.shape[0], self.k
            _lib.call("reidmi_search_merge_f32", _lib.ptr(self._idx[lo]), _lib.ptr(self._dist[lo]), 2, Q, k, Q * k, k,
                      _lib.ptr(base), k, _lib.ptr(self._idx[2 - c]), _lib.ptr(self._dist[2 - c]), k, _lib.stream())
            self._carried = 2 - c
        self.count += rows

    def _bound(self):
        """The next block's bound for _search_into: the carried k-th key and / or the radius."""
        k = self.k
        if self.count == 0 or not self.carry_bound:
            return None if self._tau is None else (self._tau, None, 1, self.count)
        bd, bi = self._dist[self._carried][:, k - 1], self._idx[self._carried][:, k - 1]
        if self._tau is None:
            return bd, bi, k, self.count
        full = bi >= 0  # else the radius, with every tie at it in: no index reaches 2^31 - 1
        return (torch.where(full, bd, self._tau), torch.where(full, bi, torch.full_like(bi, 2 ** 31 - 1)), 1,
                self.count)

    def result(self):
        """(idx int32 [Q][k], dist fp32 [Q][k] or None) on the device, as search_device."""
        if self.count < self.k:
            raise _lib.ReidmiError(f"SearchAccumulator: need 1 <= k <= G, and {self.count} gallery items were added "
                                   f"for k = {self.k}")
        return self._idx[self._carried], (self._dist[self._carried] if self.with_dist else None)


def search_blocks_device(qf, blocks, k, q_pids=None, q_camids=None, with_dist=True,
                         carry_bound=CARRY_BOUND_DEFAULT, max_dist=None, prefilter=False, q_filter=None):
    """SearchAccumulator over ``blocks``: an iterable of feature blocks or, with query labels, of
    (features, g_pids, g_camids) tuples; with a filter, of (features, g_pids, g_camids, g_attrs)
    tuples (the labels None without query labels).  Bit for bit search_device over their
    concatenation (with the same max_dist and filter), whatever carry_bound and prefilter are."""
    acc = SearchAccumulator(qf, k, q_pids, q_camids, with_dist, carry_bound, max_dist, prefilter, q_filter=q_filter)
    for b in blocks:
        acc.add(*b) if isinstance(b, (tuple, list)) else acc.add(b)
    return acc.result()


def search_blocks(qf, blocks, k, q_pids=None, q_camids=None, with_dist=True, carry_bound=CARRY_BOUND_DEFAULT,
                  max_dist=None, prefilter=False, q_filter=None):
    """search_blocks_device, returned as numpy arrays."""
    idx, dist = search_blocks_device(qf, blocks, k, q_pids, q_camids, with_dist, carry_bound, max_dist, prefilter,
                                     q_filter)
    return idx.cpu().numpy(), (dist.cpu().numpy() if with_dist else None)


def search_sharded_device(qf_local, gf_local, k, q_pids=None, q_camids=None, g_pids=None, g_camids=None,
                          with_dist=True):
    """search_device under R1_mAP_eval(sharded=True)'s contract (distributed.py): every rank passes
    ITS query rows and ITS gallery rows (contiguous shards in rank order, labels likewise) and gets
    the full (idx int32 [Q][k], dist fp32 [Q][k] or None), bit for bit the one-process search_device
    over the rank-ordered concatenations.  The query features and labels are all-gathered, every rank
    searches all queries against its own gallery shard, and the [Q][k] lists (8 bytes an entry) and
    the shard sizes are all-gathered and joined by reidmi_search_merge_f32 with the shard offsets as
    bases: gallery features never travel.  A shard of fewer than k rows, or none, contributes padded
    rows.  Needs an initialised process group."""
    from . import distributed as rd
    if not rd._initialized():
        raise _lib.ReidmiError("search_sharded needs an initialised torch.distributed process group")
    labels = _labels_given("search_sharded", q_pids, q_camids, g_pids, g_camids)
    qf_local, gf = _as_dev_f32(qf_local), _as_dev_f32(gf_local)
    k = int(k)
    if not 1 <= k <= 128:
        raise _lib.ReidmiError("search_sharded: need 1 <= k <= 128")
    qf, _ = rd.gather_rows_var(qf_local)
    lab = (None,) * 4
    if labels:
        ql, _ = rd.gather_rows_var(torch.stack([_as_dev_i64(q_pids), _as_dev_i64(q_camids)], 1))
        lab = (ql[:, 0].contiguous(), ql[:, 1].contiguous(), _as_dev_i64(g_pids), _as_dev_i64(g_camids))
    Q, rows = qf.shape[0], gf.shape[0]
    idx = torch.full((Q, k), -1, device=qf.device, dtype=torch.int32)
    dist = torch.full((Q, k), float("inf"), device=qf.device, dtype=torch.float32)
    if rows:
        _search_into(qf, gf, min(k, rows), lab, idx, dist, k)
    all_idx, all_dist, base = rd.gather_lists(idx, dist, rows)
    if int(base[-1]) < k:
        raise _lib.ReidmiError(f"search_sharded: need 1 <= k <= G, and the shards hold {int(base[-1])} gallery items")
    return merge_lists_device(all_idx, all_dist, k, base[:-1].to(qf.device), with_dist)


def search_sharded(qf_local, gf_local, k, q_pids=None, q_camids=None, g_pids=None, g_camids=None, with_dist=True):
    """search_sharded_device, returned as numpy arrays."""
    idx, dist = search_sharded_device(qf_local, gf_local, k, q_pids, q_camids, g_pids, g_camids, with_dist)
    return idx.cpu().numpy(), (dist.cpu().numpy() if with_dist else None)


# ------------------------------------------- combined rows: query expansion, DBA, group pooling
_COMBINE_MODES = {"sum": 0, "mean": 1, "max": 2}


def _rows_f32(x, what):
    """A 2-D fp32 device tensor with unit column stride; the row pitch is kept (no copy of a view
    such as buf[:, :d])."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    x = x.to(device=_dev(), dtype=torch.float32)
    if x.dim() != 2:
        raise _lib.ReidmiError(f"combine_rows: {what} must be 2-D")
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _pitch(x):
    return max(x.stride(0), x.shape[1]) if x.shape[0] > 1 else x.shape[1]


def combine_rows_device(src, offsets, idx, w=None, base=None, base_w=1.0, mode="sum", normalize=False):
    """out[r] = f(base_w * base[r], {w[t] * src[idx[t]] : offsets[r] <= t < offsets[r + 1]}), f = sum,
    mean or max over the list, then optionally the L2 normalisation (reidmi_combine_rows_f32: one
    kernel, no [rows][entries][D] intermediate).  src fp32 [n_src][D] and base fp32 [rows][D] or None
    (unit column stride, any row pitch); offsets int64 [rows + 1] starting at 0, ascending, ending at
    len(idx); idx int32; w fp32 like idx, or None (= 1; "max" takes none).  Entries < 0 are skipped
    (search's padding); an entry >= n_src raises ReidmiError.  The arithmetic is fixed bit for bit
    (include/reidmi.h): one fp32 accumulator per column, the entries added in list order, product
    and sum each rounded, never fused; normalize=True equals l2_normalize_device of the
    normalize=False result.  Returns fp32 [rows][D] on the device."""
    if mode not in _COMBINE_MODES:
        raise _lib.ReidmiError(f"combine_rows: mode must be 'sum', 'mean' or 'max', not {mode!r}")
    src = _rows_f32(src, "src")
    dev = src.device
    offsets = _as_dev_i64(offsets).reshape(-1)
    idx = (idx if isinstance(idx, torch.Tensor) else torch.from_numpy(np.asarray(idx)))
    idx = idx.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    rows = offsets.numel() - 1
    n_src, d = src.shape
    if rows < 0:
        raise _lib.ReidmiError("combine_rows: offsets needs rows + 1 entries")
    if w is not None:
        w = (w if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w)))
        w = w.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if w.numel() != idx.numel():
            raise _lib.ReidmiError("combine_rows: one weight per list entry")
    if base is not None:
        base = _rows_f32(base, "base")
        if tuple(base.shape) != (rows, d):
            raise _lib.ReidmiError("combine_rows: base must be [rows][D]")
    # the kernel trusts the offsets (they index idx): check them before it runs
    if not bool(((offsets[0] == 0) & (offsets[-1] == idx.numel()) & (offsets[1:] >= offsets[:-1]).all()).item()):
        raise _lib.ReidmiError("combine_rows: offsets must start at 0, ascend and end at len(idx)")
    out = torch.empty((rows, d), device=dev, dtype=torch.float32)
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("reidmi_combine_rows_f32", _lib.ptr(src), n_src, d, _pitch(src), _lib.ptr(offsets), _lib.ptr(idx),
              _lib.ptr(w), rows, _lib.ptr(base), 0 if base is None else _pitch(base), float(base_w),
              _COMBINE_MODES[mode], int(bool(normalize)), _lib.ptr(out), d, _lib.ptr(bad), _lib.stream())
    n_bad = int(bad.item())
    if n_bad:
        raise _lib.ReidmiError(f"combine_rows: {n_bad} list entries point past the {n_src} source rows")
    return out


def _alpha(alpha):
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or alpha < 0:
        raise _lib.ReidmiError(f"expand_features: alpha must be an integer >= 0, not {alpha!r}")
    return int(alpha)


def expand_features_device(xf, gf, k, alpha=0, include_x=True):
    """Query expansion: x' = normalise((x if include_x) + sum_i w_i g_nn_i) over the k nearest rows
    of gf, nearest first (search_device(xf, gf, k) without labels: expansion never sees pids; ties by
    gallery index).  alpha == 0: w_i = 1 (average query expansion, Chum et al.).  alpha >= 1 (an
    integer): w_i = s_i ** alpha (alpha-QE, Radenovic et al.) with s = clamp(1 - dist / 2, 0), which
    is the cosine when the rows are unit length (dist is the squared Euclidean distance, 2 - 2 cos);
    the power is s multiplied by itself alpha - 1 times in fp32, left to right, no pow.  One
    reidmi_combine_rows_f32 call on the lists (no [Q][k][D] tensor); fp32 [Q][D] on the device,
    bit-reproducible.  1 <= k <= min(G, 128)."""
    alpha = _alpha(alpha)
    xf, gf = _as_dev_f32(xf), _as_dev_f32(gf)
    idx, dist = search_device(xf, gf, k, with_dist=alpha > 0)
    w = None
    if alpha:
        s = (1.0 - dist * 0.5).clamp_(min=0.0)
        w = s
        for _ in range(alpha - 1):
            w = w * s
    Q, k = idx.shape
    offsets = torch.arange(Q + 1, device=xf.device, dtype=torch.int64) * k
    return combine_rows_device(gf, offsets, idx, w, base=xf if include_x else None, base_w=1.0, mode="sum",
                               normalize=True)


def expand_features(xf, gf, k, alpha=0, include_x=True):
    """expand_features_device, returned as a numpy array."""
    return expand_features_device(xf, gf, k, alpha, include_x).cpu().numpy()


def database_augmentation_device(gf, k, alpha=0):
    """Database augmentation: every gallery row replaced by the normalised (weighted) sum of its k
    nearest gallery rows, itself included once, through its own list (it is its own nearest row):
    expand_features_device(gf, gf, k, alpha, include_x=False)."""
    return expand_features_device(gf, gf, k, alpha, include_x=False)


def database_augmentation(gf, k, alpha=0):
    """database_augmentation_device, returned as a numpy array."""
    return database_augmentation_device(gf, k, alpha).cpu().numpy()


def multi_query_groups(pids, camids):
    """The group key of Market-1501's multi-query protocol: one int64 key per (pid, camera), ordered
    by pid, then camera (so np.unique's key order is that order)."""
    pids = np.asarray(pids.cpu() if isinstance(pids, torch.Tensor) else pids, dtype=np.int64).reshape(-1)
    cams = np.asarray(camids.cpu() if isinstance(camids, torch.Tensor) else camids, dtype=np.int64).reshape(-1)
    if pids.shape != cams.shape:
        raise _lib.ReidmiError("multi_query_groups: one camera per pid")
    if cams.size == 0:
        return pids.copy()
    lo = cams.min()
    return pids * (cams.max() - lo + 1) + (cams - lo)


def pool_features_device(feat, groups, mode="mean", normalize=False):
    """Pools the rows of feat that share a group key (multi-query crops of one (pid, camera):
    multi_query_groups; tracklets: inference()'s seqs): (pooled fp32 [U][D] on the device, keys int64
    [U], inverse int64 [n]; the last two numpy, as np.unique(groups, return_inverse=True) gives
    them).  Row u pools the rows with key keys[u] in ascending row index; mode "mean", "sum" or
    "max"; normalize: L2-normalise the pooled rows.  The lists (CSR) are built on the host, the
    pooling is one reidmi_combine_rows_f32 call with the fixed arithmetic of combine_rows_device."""
    feat = _rows_f32(feat, "feat")
    groups = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups).reshape(-1)
    if groups.dtype.kind not in "iu":
        raise _lib.ReidmiError("pool_features: groups must be integer keys")
    groups = groups.astype(np.int64)
    if groups.size != feat.shape[0]:
        raise _lib.ReidmiError("pool_features: one group key per row")
    keys, inverse, counts = np.unique(groups, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1).astype(np.int64)
    offsets = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    idx = np.argsort(inverse, kind="stable").astype(np.int32)
    pooled = combine_rows_device(feat, offsets, idx, mode=mode, normalize=normalize)
    return pooled, keys, inverse


def pool_features(feat, groups, mode="mean", normalize=False):
    """pool_features_device with the pooled rows returned as a numpy array."""
    pooled, keys, inverse = pool_features_device(feat, groups, mode, normalize)
    return pooled.cpu().numpy(), keys, inverse


def eval_rows_device(dist, q_pids, g_pids, q_camids, g_camids):
    """Per-query (valid, first_match_rank, AP, n_kept) for eval_func (evaluate.py:40-80), any
    number of positives per query.  (valid = -1 / overflow = 1 were a capacity signal of older
    builds; aggregate_cmc_map still refuses them.)"""
    dist = _as_dev_f32(dist)
    Q, G = dist.shape
    qp, gp, qc, gc = (_as_dev_i64(a) for a in (q_pids, g_pids, q_camids, g_camids))
    dev = dist.device
    valid = torch.empty(Q, device=dev, dtype=torch.int32)
    first = torch.empty(Q, device=dev, dtype=torch.int64)
    ap = torch.empty(Q, device=dev, dtype=torch.float64)
    nkept = torch.empty(Q, device=dev, dtype=torch.int64)
    overflow = torch.empty(1, device=dev, dtype=torch.int32)  # written by the call
    ws = torch.empty(_lib.load().reidmi_eval_rows_workspace_bytes(G), device=dev, dtype=torch.uint8)
    _lib.call("reidmi_eval_rows", _lib.ptr(dist), Q, G, dist.stride(0), _lib.ptr(qp), _lib.ptr(gp), _lib.ptr(qc),
              _lib.ptr(gc), _lib.ptr(valid), _lib.ptr(first), _lib.ptr(ap), _lib.ptr(nkept), _lib.ptr(overflow),
              _lib.ptr(ws), ws.numel(), _lib.stream())
    return valid, first, ap, nkept, overflow


def aggregate_cmc_map(valid, first, ap, nkept, num_g, max_rank=50, overflow=None):
    """evaluate.py:37-39,82-88 on the per-query results, with numpy's exact arithmetic:
    CMC = float32 count / float32 num_valid, mAP = np.mean of the float64 APs in query order."""
    valid = np.asarray(valid)
    if (overflow is not None and int(np.asarray(overflow).reshape(-1)[0])) or \
            (valid.dtype != bool and (valid < 0).any()):
        raise _lib.ReidmiError("eval_rows: a query was not evaluated (overflow flag or valid < 0)")
    valid = valid > 0
    first, ap, nkept = np.asarray(first), np.asarray(ap), np.asarray(nkept)
    if num_g < max_rank:
        max_rank = num_g
        print("Note: number of gallery samples is quite small, got {}".format(num_g))
    num_valid = int(valid.sum())
    assert num_valid > 0, "Error: all query identities do not appear in gallery"
    lens = np.minimum(nkept[valid], max_rank)
    if (lens != lens[0]).any():
        # the reference's np.asarray(all_cmc) on ragged rows (evaluate.py:84)
        raise ValueError("setting an array element with a sequence. The requested array has an "
                         "inhomogeneous shape after 1 dimensions.")
    L = int(lens[0])
    f = first[valid]
    counts = (f[:, None] <= np.arange(L)[None, :]).sum(0)
    cmc = counts.astype(np.float32) / float(num_valid)
    mAP = np.mean(ap[valid])
    return cmc, mAP


# ------------------------------------------------- matrix-free scoring (reidmi_evf_*)
def _np_i64(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.int64).reshape(-1)


def _max_pid_count(g_pids):
    """The most gallery items one pid has: no query can have more matches."""
    g_pids = _np_i64(g_pids)
    return int(np.unique(g_pids, return_counts=True)[1].max()) if g_pids.size else 1


class _EvfState:
    """The caller-owned state of a scoring run (include/reidmi.h): per query a list of up to cap
    matches (8 bytes each), the counts, and the histogram the count stage fills."""

    def __init__(self, Q, cap, dev):
        self.Q, self.cap, self.dev = Q, max(int(cap), 1), dev
        self.pos = torch.zeros((Q, self.cap), device=dev, dtype=torch.int64)
        self.pos_cnt = torch.zeros(Q, device=dev, dtype=torch.int32)
        self.junk_cnt = torch.zeros(Q, device=dev, dtype=torch.int32)
        self.overflow = torch.zeros(1, device=dev, dtype=torch.int32)
        self.hist = None

    def grow(self, cap):
        """Room for lists of `cap` entries (the lists met so far are kept)."""
        if cap > self.cap:
            pos = torch.zeros((self.Q, cap), device=self.dev, dtype=torch.int64)
            pos[:, :self.cap] = self.pos
            self.pos, self.cap = pos, cap

    def _block(self, name, qf, lab, gf, base, tail):
        Q, D = qf.shape
        rows = gf.shape[0]
        nb = _lib.load().reidmi_evf_workspace_bytes(Q, rows)
        ws = torch.empty(max(nb, 16), device=self.dev, dtype=torch.uint8)
        _lib.call(name, _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), rows, gf.stride(0), D,
                  *(_lib.ptr(a) for a in lab), int(base), self.cap, _lib.ptr(self.pos), _lib.ptr(self.pos_cnt), *tail,
                  _lib.ptr(ws), nb, _lib.stream())

    def matches(self, qf, lab, gf, base):
        self._block("reidmi_evf_matches", qf, lab, gf, base, (_lib.ptr(self.junk_cnt), _lib.ptr(self.overflow)))

    def append(self, pos, pos_cnt):
        _lib.call("reidmi_evf_append", _lib.ptr(self.pos), _lib.ptr(self.pos_cnt), _lib.ptr(pos), _lib.ptr(pos_cnt),
                  self.Q, self.cap, _lib.ptr(self.overflow), _lib.stream())

    def sort(self):
        _lib.call("reidmi_evf_sort", _lib.ptr(self.pos), _lib.ptr(self.pos_cnt), self.Q, self.cap, _lib.stream())
        self.hist = torch.zeros((self.Q, self.cap + 1), device=self.dev, dtype=torch.int32)

    def count(self, qf, lab, gf, base):
        self._block("reidmi_evf_count", qf, lab, gf, base, (_lib.ptr(self.hist),))

    def finish(self, g_total):
        Q, dev = self.Q, self.dev
        valid = torch.empty(Q, device=dev, dtype=torch.int32)
        first = torch.empty(Q, device=dev, dtype=torch.int64)
        last = torch.empty(Q, device=dev, dtype=torch.int64)
        npos = torch.empty(Q, device=dev, dtype=torch.int32)
        ap = torch.empty(Q, device=dev, dtype=torch.float64)
        nkept = torch.empty(Q, device=dev, dtype=torch.int64)
        _lib.call("reidmi_evf_finish", _lib.ptr(self.pos_cnt), _lib.ptr(self.hist), _lib.ptr(self.junk_cnt), Q, self.cap,
                  int(g_total), _lib.ptr(self.overflow), _lib.ptr(valid), _lib.ptr(first), _lib.ptr(last),
                  _lib.ptr(npos), _lib.ptr(ap), _lib.ptr(nkept), _lib.stream())
        return valid, first, last, npos, ap, nkept, self.overflow


def eval_features_device(qf, gf, q_pids, g_pids, q_camids, g_camids, cap=None):
    """eval_rows_device(euclidean_distance_device(qf, gf), ...) without the (Q, G) matrix
    (reidmi_eval_feat_f32: the ranks are counted in the distance kernel's epilogue): device
    (valid, first, last, npos, ap, nkept, overflow), valid / first / ap / nkept bit for bit those of
    the two calls; last: the kept-rank of the last match (-1 without one), npos: the number of
    matches (mean_inp).  cap: the capacity of a query's match list; None: the largest count of one
    pid in the gallery (no query can overflow)."""
    qf, gf = _as_dev_f32(qf), _as_dev_f32(gf)
    Q, D = qf.shape
    G = gf.shape[0]
    cap = _max_pid_count(g_pids) if cap is None else int(cap)
    qp, gp, qc, gc = (_as_dev_i64(a) for a in (q_pids, g_pids, q_camids, g_camids))
    dev = qf.device
    valid = torch.empty(Q, device=dev, dtype=torch.int32)
    first = torch.empty(Q, device=dev, dtype=torch.int64)
    last = torch.empty(Q, device=dev, dtype=torch.int64)
    npos = torch.empty(Q, device=dev, dtype=torch.int32)
    ap = torch.empty(Q, device=dev, dtype=torch.float64)
    nkept = torch.empty(Q, device=dev, dtype=torch.int64)
    overflow = torch.empty(1, device=dev, dtype=torch.int32)  # written by the call
    nb = _lib.load().reidmi_eval_feat_workspace_bytes(Q, G, D, cap)
    ws = torch.empty(max(nb, 16), device=dev, dtype=torch.uint8)
    _lib.call("reidmi_eval_feat_f32", _lib.ptr(qf), Q, qf.stride(0), _lib.ptr(gf), G, gf.stride(0), D, _lib.ptr(qp),
              _lib.ptr(qc), _lib.ptr(gp), _lib.ptr(gc), cap, _lib.ptr(valid), _lib.ptr(first), _lib.ptr(last),
              _lib.ptr(npos), _lib.ptr(ap), _lib.ptr(nkept), _lib.ptr(overflow), _lib.ptr(ws), nb, _lib.stream())
    return valid, first, last, npos, ap, nkept, overflow


def _aggregate_features(res, num_g, max_rank):
    valid, first, last, npos, ap, nkept, overflow = res
    torch.cuda.current_stream().synchronize()
    return aggregate_cmc_map(valid.cpu().numpy(), first.cpu().numpy(), ap.cpu().numpy(), nkept.cpu().numpy(), num_g,
                             max_rank, overflow.cpu().numpy())


def eval_func_features(qf, gf, q_pids, g_pids, q_camids, g_camids, max_rank=50):
    """eval_func(euclidean_distance(qf, gf), q_pids, g_pids, q_camids, g_camids, max_rank) without the
    (Q, G) matrix: the same (cmc, mAP) bit for bit, and the same errors."""
    gf = _as_dev_f32(gf)
    return _aggregate_features(eval_features_device(qf, gf, q_pids, g_pids, q_camids, g_camids), gf.shape[0],
                               max_rank)


def eval_features_blocks_device(qf, blocks, q_pids, q_camids):
    """eval_features_device over a gallery that arrives in blocks: ``blocks`` is a re-iterable of
    (gf_block, g_pids, g_camids), or a callable returning such an iterator.  It is walked twice,
    the matches first (reidmi_evf_matches; the lists grow with the largest pid count met), then the
    counts (reidmi_evf_count); a host block is on the device for its call only, so one block is
    resident at a time.  Bit for bit eval_features_device over the concatenation, for every way of
    cutting the gallery.  Returns (its seven tensors, the gallery size)."""
    qf = _as_dev_f32(qf)
    qp, qc = _as_dev_i64(q_pids), _as_dev_i64(q_camids)
    walk = blocks if callable(blocks) else (lambda: iter(blocks))
    st = _EvfState(qf.shape[0], 1, qf.device)
    seen = {}
    sizes = []

    def block(b, base):
        gf, gp, gc = b
        if base + int(gf.shape[0]) >= 2 ** 31:
            raise _lib.ReidmiError("eval_features_blocks: gallery indices must fit int32")
        gf, gp, gc = _as_dev_f32(gf), _as_dev_i64(gp), _as_dev_i64(gc)
        if gp.numel() != gf.shape[0] or gc.numel() != gf.shape[0]:
            raise _lib.ReidmiError("eval_features_blocks: one label per gallery row")
        return gf, (qp, qc, gp, gc)

    base = 0
    for b in walk():
        rows = int(b[0].shape[0])
        sizes.append(rows)
        if rows == 0:
            continue
        for pid, n in zip(*np.unique(_np_i64(b[1]), return_counts=True)):
            seen[int(pid)] = seen.get(int(pid), 0) + int(n)
        st.grow(max(seen.values()))
        gf, lab = block(b, base)
        st.matches(qf, lab, gf, base)
        base += rows
    total = base
    if total == 0:
        raise _lib.ReidmiError("eval_features_blocks: the gallery is empty")
    st.sort()
    base = 0
    for n, b in enumerate(walk()):
        rows = int(b[0].shape[0])
        if n >= len(sizes) or rows != sizes[n]:
            raise _lib.ReidmiError("eval_features_blocks: the second walk over the blocks differs from the first")
        if rows == 0:
            continue
        gf, lab = block(b, base)
        st.count(qf, lab, gf, base)
        base += rows
    if base != total:
        raise _lib.ReidmiError("eval_features_blocks: the second walk over the blocks differs from the first")
    return st.finish(total), total


def eval_features_blocks(qf, blocks, q_pids, q_camids, max_rank=50):
    """eval_func_features over a gallery in blocks (eval_features_blocks_device): (cmc, mAP)."""
    res, total = eval_features_blocks_device(qf, blocks, q_pids, q_camids)
    return _aggregate_features(res, total, max_rank)


def eval_features_sharded_device(qf_local, gf_local, q_pids, q_camids, g_pids, g_camids):
    """eval_features_device under search_sharded's contract: every rank passes ITS query rows and ITS
    gallery rows (contiguous shards in rank order, labels likewise).  The query features, the query
    labels and the gallery pids (for the list capacity) are all-gathered; every rank collects all
    queries' matches in its own shard; the lists ([Q][cap] entries of 8 bytes) and their counts are
    all-gathered and appended; every rank counts its own shard; the histograms and removed-item
    counts are sum-all-reduced, and every rank finishes all queries.  No gallery feature leaves its
    rank.  Returns (the seven tensors of eval_features_device for all queries, the gallery size),
    bit for bit the one-process result."""
    from . import distributed as rd
    if not rd._initialized():
        raise _lib.ReidmiError("eval_features_sharded needs an initialised torch.distributed process group")
    rank, W = rd.world()
    qf_local, gf = _as_dev_f32(qf_local), _as_dev_f32(gf_local)
    dev = gf.device
    qf, _ = rd.gather_rows_var(qf_local)
    ql, _ = rd.gather_rows_var(torch.stack([_as_dev_i64(q_pids), _as_dev_i64(q_camids)], 1))
    gp, gc = _as_dev_i64(g_pids), _as_dev_i64(g_camids)
    gp_all, ns = rd.gather_rows_var(gp)
    total, base, rows = sum(ns), sum(ns[:rank]), gf.shape[0]
    if total == 0:
        raise _lib.ReidmiError("eval_features_sharded: the gallery is empty")
    if total >= 2 ** 31:
        raise _lib.ReidmiError("eval_features_sharded: gallery indices must fit int32")
    lab = (ql[:, 0].contiguous(), ql[:, 1].contiguous(), gp, gc)
    Q = qf.shape[0]
    mine = _EvfState(Q, _max_pid_count(gp_all), dev)
    if rows:
        mine.matches(qf, lab, gf, base)
    lists, _ = rd.gather_rows_var(mine.pos[None])
    counts, _ = rd.gather_rows_var(mine.pos_cnt[None])
    st = _EvfState(Q, mine.cap, dev)
    for r in range(W):
        st.append(lists[r].contiguous(), counts[r].contiguous())
    st.junk_cnt = mine.junk_cnt
    st.sort()
    if rows:
        st.count(qf, lab, gf, base)
    st.hist = rd.all_reduce_sum(st.hist)
    st.junk_cnt = rd.all_reduce_sum(st.junk_cnt)
    return st.finish(total), total


def eval_features_sharded(qf_local, gf_local, q_pids, q_camids, g_pids, g_camids, max_rank=50):
    """eval_func_features over gallery shards (eval_features_sharded_device): every rank returns the
    one-process (cmc, mAP) bit for bit."""
    res, total = eval_features_sharded_device(qf_local, gf_local, q_pids, q_camids, g_pids, g_camids)
    return _aggregate_features(res, total, max_rank)


def mean_inp(valid, last, npos):
    """mINP (Ye et al., "Deep Learning for Person Re-identification: A Survey and Outlook"): the
    mean over the valid queries of npos / (last + 1) in float64, last the 0-based kept-rank of the
    query's last match (eval_features_device's outputs)."""
    valid, last, npos = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a) for a in (valid, last, npos))
    v = valid > 0
    if not v.any():
        raise _lib.ReidmiError("mean_inp: no valid query")
    return np.mean(npos[v].astype(np.float64) / (last[v].astype(np.float64) + 1.0))


# ------------------------------- verification / open-set statistics (reidmi_pair_stats_f32)
PAIR_STATS_MAX_EDGES = 255


def default_edges():
    """255 equal steps over [0, 4], the range of squared distances between unit vectors."""
    return (np.arange(1, PAIR_STATS_MAX_EDGES + 1, dtype=np.float64) * (4.0 / PAIR_STATS_MAX_EDGES)).astype(np.float32)


def _edges(what, edges):
    """edges as a contiguous host fp32 array, checked as the library checks it."""
    if edges is None:
        return default_edges()
    if isinstance(edges, torch.Tensor):
        edges = edges.detach().cpu().numpy()
    try:
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float32)).reshape(-1)
    except (TypeError, ValueError):
        raise _lib.ReidmiError(f"{what}: edges must be a 1-D array of numbers") from None
    if not 1 <= e.size <= PAIR_STATS_MAX_EDGES:
        raise _lib.ReidmiError(f"{what}: need 1 <= len(edges) <= {PAIR_STATS_MAX_EDGES}, not {e.size}")
    if not np.isfinite(e).all():
        raise _lib.ReidmiError(f"{what}: edges must be finite")
    if (e[1:] < e[:-1]).any():
        raise _lib.ReidmiError(f"{what}: edges must be non-decreasing")
    return e


class PairStats:
    """The statistics of a labelled split (reidmi_pair_stats_f32, include/reidmi.h):
        edges      host fp32 [E]
        hist_pos   int64 [E + 1]: genuine pairs per bin, bin = np.searchsorted(edges, d, side="left")
        hist_neg   int64 [E + 1]: impostor pairs per bin
        near_pos   (dist fp32 [Q], idx int32 [Q]): every query's nearest genuine item, +inf / -1 without one
        near_neg   likewise, the nearest impostor
    The arrays are device tensors (pair_stats_device) or numpy arrays (pair_stats, .numpy())."""

    def __init__(self, edges, hist_pos, hist_neg, near_pos, near_neg):
        self.edges, self.hist_pos, self.hist_neg = edges, hist_pos, hist_neg
        self.near_pos, self.near_neg = tuple(near_pos), tuple(near_neg)

    def numpy(self):
        def host(a):
            return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return PairStats(self.edges, host(self.hist_pos), host(self.hist_neg), tuple(host(a) for a in self.near_pos),
                         tuple(host(a) for a in self.near_neg))


class PairStatsAccumulator:
    """pair_stats_device over a gallery that arrives in blocks: add() each block (a device or host
    tensor, or a numpy array; a host block is on the device for the call only), then result().  The
    counts are integer sums and the nearest items minima of unique (distance, global index) keys, so
    the result is bit for bit the one-call result for every way of cutting the gallery and every order
    of the blocks.  q_camids None: every block comes without g_camids and nothing is removed for its
    camera.  A block's rows stand at the global indices index_base .. index_base + rows: by default
    the number of rows added before it (the blocks in gallery order); a caller that feeds them in
    another order passes each block's own index_base.  exclude_self: the gallery is the query set
    itself, and the pair of a row with itself (global index == query row) is left out.
    Carried state: two histograms and two [Q] (dist, idx) pairs; nothing grows with the gallery."""

    def __init__(self, qf, q_pids, q_camids=None, edges=None, exclude_self=False):
        if not isinstance(exclude_self, (bool, np.bool_)):
            raise _lib.ReidmiError("PairStatsAccumulator: exclude_self must be True or False")
        self.edges = _edges("PairStatsAccumulator", edges)
        if q_pids is None:
            raise _lib.ReidmiError("PairStatsAccumulator: q_pids are required")
        if isinstance(qf, (np.ndarray, torch.Tensor)) and qf.ndim != 2:
            raise _lib.ReidmiError("PairStatsAccumulator: qf must be [Q][D]")
        self.qf = _as_dev_f32(qf)
        Q, dev = self.qf.shape[0], self.qf.device
        self.qp = _as_dev_i64(q_pids)
        self.cams = q_camids is not None
        self.qc = _as_dev_i64(q_camids) if self.cams else None
        if self.qp.numel() != Q or (self.cams and self.qc.numel() != Q):
            raise _lib.ReidmiError("PairStatsAccumulator: one label per query row")
        self.exclude_self = bool(exclude_self)
        E = self.edges.size
        self.hist_pos = torch.zeros(E + 1, device=dev, dtype=torch.int64)  # the library's uint64 counters
        self.hist_neg = torch.zeros(E + 1, device=dev, dtype=torch.int64)
        self.pos_dist = torch.full((Q,), float("inf"), device=dev, dtype=torch.float32)
        self.neg_dist = torch.full((Q,), float("inf"), device=dev, dtype=torch.float32)
        self.pos_idx = torch.full((Q,), -1, device=dev, dtype=torch.int32)
        self.neg_idx = torch.full((Q,), -1, device=dev, dtype=torch.int32)
        self.count = 0  # gallery items added so far

    def add(self, gf_block, g_pids, g_camids=None, index_base=None):
        if (g_camids is not None) != self.cams:
            raise _lib.ReidmiError("PairStatsAccumulator.add: gallery cameras go with query cameras: every block has "
                                   "them or none has")
        if g_pids is None:
            raise _lib.ReidmiError("PairStatsAccumulator.add: g_pids are required")
        rows = int(gf_block.shape[0])
        base = self.count if index_base is None else int(index_base)
        if base < 0 or base + rows > 2 ** 31 - 1:
            raise _lib.ReidmiError("PairStatsAccumulator.add: gallery indices must fit int32 "
                                   "(index_base >= 0, index_base + rows <= 2^31 - 1)")
        if rows == 0:
            return
        gf = _as_dev_f32(gf_block)
        Q, D = self.qf.shape
        if gf.dim() != 2 or gf.shape[1] != D:
            raise _lib.ReidmiError(f"PairStatsAccumulator.add: a block must be [rows][{D}]")
        gp = _as_dev_i64(g_pids)
        gc = _as_dev_i64(g_camids) if self.cams else None
        if gp.numel() != rows or (self.cams and gc.numel() != rows):
            raise _lib.ReidmiError("PairStatsAccumulator.add: one label per gallery row")
        nb = _lib.load().reidmi_pair_stats_workspace_bytes(Q, rows)
        ws = torch.empty(max(nb, 16), device=self.qf.device, dtype=torch.uint8)
        _lib.call("reidmi_pair_stats_f32", _lib.ptr(self.qf), Q, self.qf.stride(0), _lib.ptr(gf), rows, gf.stride(0), D,
                  _lib.ptr(self.qp), _lib.ptr(self.qc), _lib.ptr(gp), _lib.ptr(gc),
                  ctypes.c_void_p(self.edges.ctypes.data), int(self.edges.size), base,
                  base if self.exclude_self else -1, _lib.ptr(self.hist_pos), _lib.ptr(self.hist_neg),
                  _lib.ptr(self.pos_dist), _lib.ptr(self.pos_idx), _lib.ptr(self.neg_dist), _lib.ptr(self.neg_idx),
                  _lib.ptr(ws), nb, _lib.stream())
        self.count += rows

    def result(self):
        """A PairStats of device tensors."""
        if self.count == 0:
            raise _lib.ReidmiError("PairStatsAccumulator: the gallery is empty")
        return PairStats(self.edges, self.hist_pos, self.hist_neg, (self.pos_dist, self.pos_idx),
                         (self.neg_dist, self.neg_idx))


def pair_stats_device(qf, gf, q_pids, g_pids, q_camids=None, g_camids=None, edges=None, exclude_self=False,
                      index_base=0):
    """The genuine / impostor distance histograms and every query's nearest genuine and nearest
    impostor item, from the features (reidmi_pair_stats_f32: counted in the distance kernel's
    epilogue, no (Q, G) matrix): a PairStats of device tensors.  The distance is
    euclidean_distance_device's, bit for bit.  A pair is genuine when the pids are equal, impostor
    when they differ; with q_camids / g_camids (both or neither) the gallery items of the query's pid
    and camera are removed (evaluate.py:46-48) and counted nowhere.  edges: up to 255 finite,
    non-decreasing thresholds (None: default_edges()); hist[0..t].sum() is the number of pairs at a
    distance <= edges[t], the pairs search(max_dist=edges[t]) and cluster.dbscan(eps=edges[t]) admit.
    exclude_self: gf is qf itself, and the pair of a row with itself is left out.  index_base: the
    global index of gf's first row (a gallery shard; merge_pair_stats joins the shards' results)."""
    acc = PairStatsAccumulator(qf, q_pids, q_camids, edges, exclude_self)
    if int(gf.shape[0]) < 1:
        raise _lib.ReidmiError("pair_stats: the gallery is empty")
    acc.add(gf, g_pids, g_camids, index_base)
    return acc.result()


def pair_stats(qf, gf, q_pids, g_pids, q_camids=None, g_camids=None, edges=None, exclude_self=False, index_base=0):
    """pair_stats_device, returned as numpy arrays."""
    return pair_stats_device(qf, gf, q_pids, g_pids, q_camids, g_camids, edges, exclude_self, index_base).numpy()


def pair_stats_blocks_device(qf, blocks, q_pids, q_camids=None, edges=None, exclude_self=False):
    """PairStatsAccumulator over ``blocks``: an iterable of (features, g_pids) or (features, g_pids,
    g_camids) tuples in gallery order.  Bit for bit pair_stats_device over their concatenation."""
    acc = PairStatsAccumulator(qf, q_pids, q_camids, edges, exclude_self)
    for b in blocks:
        acc.add(*b)
    return acc.result()


def pair_stats_blocks(qf, blocks, q_pids, q_camids=None, edges=None, exclude_self=False):
    """pair_stats_blocks_device, returned as numpy arrays."""
    return pair_stats_blocks_device(qf, blocks, q_pids, q_camids, edges, exclude_self).numpy()


def merge_pair_stats(a, b):
    """The statistics of two gallery parts (blocks, or the shards of several ranks: what they would
    exchange) as one: the histograms added, and per query the smaller (distance, global index) key of
    the two nearest items; an entry without an item (-1) loses to any item.  Both parts must use the
    same edges, the same queries and one global index space (pair_stats_device(index_base=)).  Device
    or numpy PairStats, both of one kind; the result is of that kind."""
    if not isinstance(a, PairStats) or not isinstance(b, PairStats):
        raise _lib.ReidmiError("merge_pair_stats: two PairStats are required")
    if a.edges.shape != b.edges.shape or not np.array_equal(a.edges.view(np.uint32), b.edges.view(np.uint32)):
        raise _lib.ReidmiError("merge_pair_stats: the two results were counted under different edges")
    dev = isinstance(a.hist_pos, torch.Tensor)
    if dev != isinstance(b.hist_pos, torch.Tensor):
        raise _lib.ReidmiError("merge_pair_stats: pass two device results or two numpy results")
    if tuple(a.near_pos[0].shape) != tuple(b.near_pos[0].shape):
        raise _lib.ReidmiError("merge_pair_stats: the two results have different numbers of queries")
    where = torch.where if dev else np.where

    def nearest(x, y):
        (xd, xi), (yd, yi) = x, y
        take_y = (yi >= 0) & ((xi < 0) | (yd < xd) | ((yd == xd) & (yi < xi)))
        return where(take_y, yd, xd), where(take_y, yi, xi)

    return PairStats(a.edges, a.hist_pos + b.hist_pos, a.hist_neg + b.hist_neg, nearest(a.near_pos, b.near_pos),
                     nearest(a.near_neg, b.near_neg))


def _host_stats(stats):
    if not isinstance(stats, PairStats):
        raise _lib.ReidmiError("a PairStats (pair_stats / pair_stats_device) is required")
    return stats.numpy()


def _ratio(num, den):
    """num / den in float64; NaN where den is 0 (an empty class)."""
    num = np.asarray(num, dtype=np.float64)
    return num / den if den > 0 else np.full(num.shape, np.nan)


def verification_curve(stats):
    """(far, tar) float64 [E]: at the threshold edges[t], the share of the impostor pairs and of the
    genuine pairs with a distance <= edges[t] (the false accept rate and the true accept rate of
    "same identity iff d <= edges[t]").  A class without pairs gives NaN."""
    s = _host_stats(stats)
    neg, pos = s.hist_neg.astype(np.int64), s.hist_pos.astype(np.int64)
    return _ratio(np.cumsum(neg)[:-1], int(neg.sum())), _ratio(np.cumsum(pos)[:-1], int(pos.sum()))


def _target(what, far):
    far = float(far)
    if not 0.0 <= far <= 1.0:
        raise _lib.ReidmiError(f"{what}: the target false accept rate must lie in [0, 1]")
    return far


def threshold_at_far(stats, far):
    """The largest edge whose false accept rate is at or below ``far`` (float; the edges are the only
    thresholds the histogram knows).  NaN when even the first edge accepts more, or without
    impostor pairs."""
    target = _target("threshold_at_far", far)
    s = _host_stats(stats)
    f, _ = verification_curve(s)
    ok = np.nonzero(f <= target)[0]
    return float(s.edges[ok[-1]]) if ok.size else float("nan")


def tar_at_far(stats, far):
    """The true accept rate at threshold_at_far(stats, far); NaN when that is NaN or without
    genuine pairs."""
    target = _target("tar_at_far", far)
    f, t = verification_curve(stats)
    ok = np.nonzero(f <= target)[0]
    return float(t[ok[-1]]) if ok.size else float("nan")


def equal_error_rate(stats):
    """The rate at which the false accept rate and the false reject rate 1 - TAR cross, both
    interpolated linearly between the two neighbouring edges that bracket the crossing (below the
    first edge the curve starts at FAR 0 / FRR 1, above the last it ends at FAR 1 / FRR 0).  NaN
    when a class has no pairs."""
    f, t = verification_curve(stats)
    if np.isnan(f).any() or np.isnan(t).any():
        return float("nan")
    far = np.concatenate([[0.0], f, [1.0]])
    frr = np.concatenate([[1.0], 1.0 - t, [0.0]])
    k = int(np.nonzero(far - frr >= 0.0)[0][0])  # >= 1: far - frr starts at -1 and ends at +1
    f0, f1, r0, r1 = far[k - 1], far[k], frr[k - 1], frr[k]
    s = (r0 - f0) / ((f1 - f0) - (r1 - r0))  # the denominator is (f1 - r1) - (f0 - r0) > 0
    return float(f0 + s * (f1 - f0))


def open_set_rates(stats, thresholds):
    """(dir, far) float64 arrays shaped like ``thresholds``: the open-set detection-and-identification
    rate and the false alarm rate of rank-1 identification under a distance threshold.  A query is
    known when the gallery holds a genuine item for it (near_pos idx >= 0).  A known query is
    identified at tau iff its nearest genuine item comes before its nearest impostor in the order
    of the rank lists (distance, then global index: what search puts first) and lies within tau;
    DIR(tau) is their share of the known queries.  An unknown query raises a false alarm iff its
    nearest impostor lies within tau; FAR(tau) is their share of the unknown queries.  A class
    without queries gives NaN."""
    s = _host_stats(stats)
    tau = np.asarray(thresholds, dtype=np.float64)
    (pd, pi), (nd, ni) = s.near_pos, s.near_neg
    known = pi >= 0
    first = known & ((ni < 0) | (pd < nd) | ((pd == nd) & (pi < ni)))
    t = tau.reshape(-1, 1)
    hit = (first[None, :] & (pd[None, :].astype(np.float64) <= t)).sum(1)
    alarm = ((~known & (ni >= 0))[None, :] & (nd[None, :].astype(np.float64) <= t)).sum(1)
    return (_ratio(hit, int(known.sum())).reshape(tau.shape),
            _ratio(alarm, int((~known).sum())).reshape(tau.shape))


# ------------------------------------------------------------ reference surface
def euclidean_distance(qf, gf):
    """evaluate.py:7-13 — returns a numpy float32 (Q,G) matrix."""
    return euclidean_distance_device(qf, gf).cpu().numpy()


def cosine_similarity(qf, gf):
    """evaluate.py:16-26 — arccos of the clipped cosine, numpy float32 (Q,G)."""
    from .ops import cosine_distance_device
    return cosine_distance_device(_as_dev_f32(qf), _as_dev_f32(gf)).cpu().numpy()


def eval_func_device(dist, q_pids, g_pids, q_camids, g_camids, max_rank=50):
    valid, first, ap, nkept, overflow = eval_rows_device(dist, q_pids, g_pids, q_camids, g_camids)
    torch.cuda.current_stream().synchronize()
    return aggregate_cmc_map(valid.cpu().numpy(), first.cpu().numpy(), ap.cpu().numpy(), nkept.cpu().numpy(),
                             dist.shape[1], max_rank, overflow.cpu().numpy())


def eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50):
    """evaluate.py:29-88 — Market-1501 CMC/mAP with same-pid-same-camera removal."""
    return eval_func_device(_as_dev_f32(distmat), q_pids, g_pids, q_camids, g_camids, max_rank)


class R1_mAP_eval():
    """evaluate.py:91-135.  Features stay on the GPU (the reference copies them to the CPU).
    As in the reference, ``max_rank`` is stored but compute() scores with eval_func's
    default 50 (evaluate.py:132): the CMC is 50 long whatever max_rank was given.

    ``sharded=True`` (torch.distributed process group, one process per GPU, SURVEY.md §8e;
    the contract: distributed.py): every rank holds ITS shard: its updates are its query rows
    followed by its gallery rows, and ``num_query`` is its own query count.  compute() then
    all-gathers the feature blocks and
    labels (gallery-sharded embed + RCCL all-gather, the north star's exchange step), scores
    the query rows shard(Q, rank, W) against the whole gallery (exact distance, or the
    row-sharded k-reciprocal re-rank), all-gathers the per-query results and reduces them in
    global query order: every rank returns the CMC/mAP of the single-process run over the
    rank-ordered concatenation of the shards, bit for bit (contiguous shards in rank order =
    the single-process order).  Default (``sharded=False``): the reference's single-process
    semantics on this process's data, no collective even under a process group.

    ``query_expansion`` / ``db_augmentation``: None (the default: today's path, untouched) or
    ``(k, alpha)``.  After the normalisation the gallery rows become
    database_augmentation_device(gf, k, alpha) when db_augmentation is given, then the query rows
    become expand_features_device(qf, gf, k, alpha) (against that gallery) when query_expansion is;
    compute() and rank_lists() then proceed on those features exactly as without.  Not with
    ``sharded=True`` (ReidmiError).

    ``matrix_free=True`` (default False: today's paths, untouched): compute() scores from the
    features without the (Q, G) distance matrix — eval_func_features locally (after the expansion
    above), eval_features_sharded under ``sharded=True`` (the ranks exchange match lists and rank
    histograms; no feature all-gather) — and returns the default's (cmc, mAP) bit for bit.  Not with
    ``reranking=True`` (ReidmiError): the re-ranked distance has no feature form."""

    def __init__(self, num_query, max_rank=50, feat_norm=True, reranking=False, sharded=False,
                 query_expansion=None, db_augmentation=None, matrix_free=False):
        super(R1_mAP_eval, self).__init__()
        self.num_query = num_query
        self.max_rank = max_rank
        self.feat_norm = feat_norm
        self.reranking = reranking
        self.sharded = sharded
        self.query_expansion = query_expansion
        self.db_augmentation = db_augmentation
        self.matrix_free = matrix_free
        self._check_expansion()
        self._check_matrix_free()

    def _check_matrix_free(self):
        if self.matrix_free and self.reranking:
            raise _lib.ReidmiError("R1_mAP_eval: matrix_free=True is not available with reranking=True (the "
                                   "re-ranked distance has no feature form)")

    def _check_expansion(self):
        if self.query_expansion is None and self.db_augmentation is None:
            return False
        if self.sharded:
            raise _lib.ReidmiError("R1_mAP_eval: query_expansion / db_augmentation are not available with "
                                   "sharded=True")
        for name, v in (("query_expansion", self.query_expansion), ("db_augmentation", self.db_augmentation)):
            if v is not None and (not isinstance(v, (tuple, list)) or len(v) != 2):
                raise _lib.ReidmiError(f"R1_mAP_eval: {name} must be None or (k, alpha)")
        return True

    def _expand(self, feats):
        """The features compute() / rank_lists() score: DBA on the gallery rows, then QE on the query
        rows against that gallery (each when asked for); ``feats`` itself when neither is."""
        if not self._check_expansion():
            return feats
        qf, gf = feats[:self.num_query], feats[self.num_query:]
        if self.db_augmentation is not None:
            gf = database_augmentation_device(gf, *self.db_augmentation)
        if self.query_expansion is not None:
            qf = expand_features_device(qf, gf, *self.query_expansion)
        return torch.cat([qf, gf], dim=0)

    def reset(self):
        self.feats = []
        self.pids = []
        self.camids = []

    def update(self, output):  # called once for each batch
        feat, pid, camid = output
        self.feats.append(_as_dev_f32(feat))
        self.pids.extend(np.asarray(pid.cpu() if isinstance(pid, torch.Tensor) else pid))
        self.camids.extend(np.asarray(camid.cpu() if isinstance(camid, torch.Tensor) else camid))

    def compute(self):  # called after each epoch
        from . import distributed as rd
        self._check_expansion()
        self._check_matrix_free()
        feats = torch.cat(self.feats, dim=0)
        if self.feat_norm:
            print("The test feature is normalized")
            feats = l2_normalize_device(feats)
        if self.sharded:
            if not rd._initialized():
                raise _lib.ReidmiError("R1_mAP_eval(sharded=True) needs an initialised torch.distributed process group")
            if self.matrix_free:
                return self._compute_matrix_free(feats, eval_features_sharded)
            return self._compute_sharded(feats)
        with rd.local():
            if self.matrix_free:
                return self._compute_matrix_free(self._expand(feats), eval_func_features)
            return self._compute_local(self._expand(feats))

    def _compute_matrix_free(self, feats, score):
        nq = self.num_query
        pids, camids = np.asarray(self.pids), np.asarray(self.camids)
        print('=> Computing DistMat with euclidean_distance')
        if score is eval_func_features:
            cmc, mAP = score(feats[:nq], feats[nq:], pids[:nq], pids[nq:], camids[:nq], camids[nq:])
        else:
            cmc, mAP = score(feats[:nq], feats[nq:], pids[:nq], camids[:nq], pids[nq:], camids[nq:])
        self._print(cmc, mAP)
        return cmc, mAP

    def _compute_local(self, feats):
        qf = feats[:self.num_query]
        q_pids = np.asarray(self.pids[:self.num_query])
        q_camids = np.asarray(self.camids[:self.num_query])
        gf = feats[self.num_query:]
        g_pids = np.asarray(self.pids[self.num_query:])
        g_camids = np.asarray(self.camids[self.num_query:])
        if self.reranking:
            print('=> Enter reranking')
            from .reranking import re_ranking_device
            distmat = re_ranking_device(qf, gf, k1=50, k2=15, lambda_value=0.3)
        else:
            print('=> Computing DistMat with euclidean_distance')
            distmat = euclidean_distance_device(qf, gf)
        cmc, mAP = eval_func_device(distmat, q_pids, g_pids, q_camids, g_camids)
        self._print(cmc, mAP)
        return cmc, mAP

    def rank_lists(self, k=10, remove_same_cam=True, prefilter=False, g_attrs=None, q_filter=None):
        """The ranked lists behind compute()'s scores (SURVEY.md §8e "top-max_rank rank lists for
        output"): numpy (idx int32 [num_query][k], dist fp32 [num_query][k]) of the query rows against
        the gallery rows, features normalised as compute() does, nearest first, ties by gallery index;
        with remove_same_cam the gallery items of the query's pid and camera are left out
        (evaluate.py:46-48; short rows end in -1 / +inf).  With ``reranking=True`` the lists are those
        of the k-reciprocal re-ranked distance compute() scores (k1 = 50, k2 = 15, lambda = 0.3;
        reranking.re_ranking_search, no (Q, G) matrix), dist the re-ranked distances; otherwise the
        Euclidean neighbours (search).  1 <= k <= min(num_gallery, 128).  ``sharded=False``:
        single-process semantics on this process's data, no collective.  ``sharded=True`` (the shards
        of compute()'s contract): every rank returns the lists of the whole split, all queries in rank
        order against the rank-ordered gallery, bit for bit the single-process lists.  The Euclidean
        lists come from search_sharded (every rank searches its own gallery shard, the ranks exchange
        lists, not features); the re-ranked ones gather features and labels as compute() does (the
        k-reciprocal stages need the whole gallery) and shard the rows (re_ranking_search(sharded=True)).
        prefilter: the single-process Euclidean lists through search(prefilter=True), the same lists
        bit for bit; the re-ranked and sharded paths do not take it.
        g_attrs / q_filter (ItemAttrs of the gallery rows, QueryFilter of the query rows): the
        single-process Euclidean lists through search(g_attrs=, q_filter=), e.g.
        q_filter=QueryFilter(cam_mask=cross_camera_mask(q_camids)) with g_attrs=ItemAttrs(camids=g_camids)
        for cross-camera-only lists; the re-ranked and sharded paths refuse a filter."""
        from . import distributed as rd
        self._check_expansion()
        if (g_attrs is not None or q_filter is not None) and (self.sharded or self.reranking):
            raise _lib.ReidmiError("R1_mAP_eval.rank_lists: g_attrs / q_filter go with the single-process Euclidean "
                                   "lists only (not sharded=True or reranking=True)")
        feats = torch.cat(self.feats, dim=0)
        if self.feat_norm:
            feats = l2_normalize_device(feats)
        nq = self.num_query
        lab = ()
        if remove_same_cam:
            lab = (np.asarray(self.pids[:nq]), np.asarray(self.camids[:nq]), np.asarray(self.pids[nq:]),
                   np.asarray(self.camids[nq:]))
        if self.sharded:
            if not rd._initialized():
                raise _lib.ReidmiError("R1_mAP_eval(sharded=True) needs an initialised torch.distributed process group")
            if not self.reranking:
                return search_sharded(feats[:nq], feats[nq:], k, *lab)
            from .reranking import re_ranking_search
            qf, _ = rd.gather_rows_var(feats[:nq].contiguous())
            gf, _ = rd.gather_rows_var(feats[nq:].contiguous())
            if remove_same_cam:
                both = _as_dev_i64(np.stack([np.asarray(self.pids, np.int64), np.asarray(self.camids, np.int64)], 1))
                ql, _ = rd.gather_rows_var(both[:nq].contiguous())
                gl, _ = rd.gather_rows_var(both[nq:].contiguous())
                lab = (ql[:, 0], ql[:, 1], gl[:, 0], gl[:, 1])
            return re_ranking_search(qf, gf, k, 50, 15, 0.3, *lab, sharded=True)
        with rd.local():
            feats = self._expand(feats)
            if self.reranking:
                from .reranking import re_ranking_search
                return re_ranking_search(feats[:nq], feats[nq:], k, 50, 15, 0.3, *lab)
            return search(feats[:nq], feats[nq:], k, *lab, prefilter=prefilter, g_attrs=g_attrs, q_filter=q_filter)

    def pair_stats(self, edges=None):
        """pair_stats (numpy) of the query rows against the gallery rows on the features and labels
        compute() scores: after the normalisation and the query expansion / database augmentation,
        with the same-pid-same-camera removal.  The thresholds read off it (threshold_at_far) are on
        the scale of rank_lists' distances, search(max_dist=) and cluster.dbscan(eps=).  Not with
        ``sharded=True`` (the ranks would have to exchange their statistics: merge_pair_stats joins
        them, a collective wrapper does not exist yet) and not with ``reranking=True`` (the re-ranked
        distance has no feature form): ReidmiError."""
        if self.sharded:
            raise _lib.ReidmiError("R1_mAP_eval.pair_stats is not available with sharded=True (no collective "
                                   "wrapper yet: compute pair_stats per shard and join them with merge_pair_stats)")
        if self.reranking:
            raise _lib.ReidmiError("R1_mAP_eval.pair_stats is not available with reranking=True (the re-ranked "
                                   "distance has no feature form)")
        from . import distributed as rd
        self._check_expansion()
        feats = torch.cat(self.feats, dim=0)
        if self.feat_norm:
            feats = l2_normalize_device(feats)
        nq = self.num_query
        pids, camids = np.asarray(self.pids), np.asarray(self.camids)
        with rd.local():
            feats = self._expand(feats)
            return pair_stats(feats[:nq], feats[nq:], pids[:nq], pids[nq:], camids[:nq], camids[nq:], edges)

    @staticmethod
    def _print(cmc, mAP):
        print("Rank@{:d}:{:.1%}, Rank@{:d}:{:.1%}, Rank@{:d}:{:.1%}, mAP:{:.1%}".format(
            1, cmc[0], 5, cmc[4], 10, cmc[9], mAP))

    def _compute_sharded(self, feats):
        from . import distributed as rd
        rank, W = rd.world()
        nq = self.num_query
        lab = torch.from_numpy(np.stack([np.asarray(self.pids, np.int64), np.asarray(self.camids, np.int64)], 1))
        qf, _ = rd.gather_rows_var(feats[:nq].contiguous())
        gf, _ = rd.gather_rows_var(feats[nq:].contiguous())
        ql, _ = rd.gather_rows_var(lab[:nq].contiguous())
        gl, _ = rd.gather_rows_var(lab[nq:].contiguous())
        Q, G = qf.shape[0], gf.shape[0]
        qlo, qhi = rd.shard(Q, rank, W)
        if self.reranking:
            print('=> Enter reranking')
            from .reranking import re_ranking_sharded
            d = re_ranking_sharded(qf, gf, 50, 15, 0.3)  # this rank's rows shard(Q, rank, W)
        else:
            print('=> Computing DistMat with euclidean_distance')
            d = euclidean_distance_device(qf[qlo:qhi], gf)
        ql, gl = ql.numpy(), gl.numpy()
        valid, first, ap, nkept, ovf = eval_rows_device(d, ql[qlo:qhi, 0], gl[:, 0], ql[qlo:qhi, 1], gl[:, 1])
        if int(ovf.item()):
            raise _lib.ReidmiError("eval_rows: a query was not evaluated (overflow flag)")
        rows = rd.gather_rows(rd.pack_rows(valid, first, ap, nkept), Q)
        cmc, mAP = aggregate_cmc_map(*rd.unpack_rows(rows), G, 50)
        self._print(cmc, mAP)
        return cmc, mAP
