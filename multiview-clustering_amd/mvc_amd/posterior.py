"""Posterior clustering summary of the sampler's draws, on the device.

The step the reference's script leaves to ``mcclust`` / ``mcclust.ext`` after
``run_gibbs_cpp`` (New_Simulation.R:5-7 loads them; :189 scores only the last
draw): the posterior similarity matrix (``comp.psm``) and a point estimate
chosen from the draws by expected Binder loss (``minbinder(method="draws")``)
or expected variation of information.  ``draws`` is plain numpy indexing;
``compare``, ``psm`` and ``point_estimate`` run in libmvc_hip.so
(mvc_partition_compare / mvc_partition_psm, include/mvc.h) and raise
``MvcError`` on failure.  Labels are ``int32 [S, n]``: S draws of a labeling
of n items, any values.
"""
import ctypes

import numpy as np

from . import _lib as L

MAX_DRAWS = L.POSTERIOR_MAX_DRAWS     # S cap of compare()
PSM_MAX_N = L.POSTERIOR_PSM_MAX_N     # n cap of psm()
LDS_CELLS = L.POSTERIOR_LDS_CELLS     # pairs with ra*rb + ra + rb beyond this leave the LDS kernel

_ip = ctypes.POINTER(ctypes.c_int32)


def draws(res, view=None, compact=False):
    """Labels of every saved sample: ``int32 [S_total, n]``.

    ``res`` is a result dict of ``run_gibbs_cpp`` or a list of them (chains
    are pooled, chain-major).  ``view=None`` gives the table partition
    (``table_of``); ``view=v`` gives view v's clusters ``dish_of[v][table_of]``,
    exactly as ``get_final_clusters`` derives them (New_Simulation.R:135-149)
    but for every saved sample.  ``compact=True`` renumbers each sample's dish
    ids 0..K-1 in ascending raw id (the same partitions; what
    mvc_result_labels returns).  No GPU work."""
    chains = [res] if isinstance(res, dict) else list(res)
    rows = []
    for r in chains:
        for s in range(len(r["table_of"])):
            t = np.asarray(r["table_of"][s])
            if view is None:
                rows.append(t)
                continue
            d = np.asarray(r["dish_of"][s][view])
            if compact:
                d = np.unique(d, return_inverse=True)[1].reshape(d.shape)
            rows.append(d[t])
    if not rows:
        raise ValueError("draws: the result holds no saved samples")
    return np.ascontiguousarray(np.stack(rows), dtype=np.int32)


def _labels(labels):
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 2:
        raise ValueError("labels must have shape [S, n]")
    return lab


def compare(labels, device=0):
    """Every pair of draws compared through its contingency table
    (mvc_partition_compare).  Returns a dict: ``binder`` (uint64 [S, S], item
    pairs on which two draws disagree), ``vi`` (float64 [S, S], variation of
    information in bits, ``mcclust.ext::VI``), ``binder_sum`` / ``vi_sum``
    (row sums; divide by S for the expected loss of each draw), ``best_binder``
    / ``best_vi`` (their argmins, ties to the lowest index)."""
    lab = _labels(labels)
    S, n = lab.shape
    cap = min(max(S, 0), MAX_DRAWS)   # above the cap the library refuses before writing anything
    binder = np.empty((cap, cap), dtype=np.uint64)
    vi = np.empty((cap, cap), dtype=np.float64)
    bsum = np.empty(cap, dtype=np.uint64)
    vsum = np.empty(cap, dtype=np.float64)
    best = np.empty(2, dtype=np.int32)
    up = ctypes.POINTER(ctypes.c_uint64)
    dp = ctypes.POINTER(ctypes.c_double)
    buf = L.errbuf()
    L.check(L.lib().mvc_partition_compare(device, lab.ctypes.data_as(_ip), S, n, binder.ctypes.data_as(up),
                                          vi.ctypes.data_as(dp), bsum.ctypes.data_as(up), vsum.ctypes.data_as(dp),
                                          best.ctypes.data_as(_ip), buf, len(buf)), buf)
    return {"binder": binder, "vi": vi, "binder_sum": bsum, "vi_sum": vsum,
            "best_binder": int(best[0]), "best_vi": int(best[1])}


def psm_counts(labels, device=0):
    """Co-clustering counts ``uint32 [n, n]``: the number of draws in which
    items i and j share a label (mvc_partition_psm)."""
    lab = _labels(labels)
    S, n = lab.shape
    # beyond the cap the library reports MVC_ERR_UNSUPPORTED before it looks
    # at the output, so none is allocated
    counts = np.empty((n, n), dtype=np.uint32) if n <= PSM_MAX_N else None
    buf = L.errbuf()
    out = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if counts is not None else None
    L.check(L.lib().mvc_partition_psm(device, lab.ctypes.data_as(_ip), S, n, out, buf, len(buf)), buf)
    return counts


def psm(labels, device=0):
    """Posterior similarity matrix ``float64 [n, n]`` (``mcclust::comp.psm``):
    the device's exact counts divided by S."""
    lab = _labels(labels)
    return psm_counts(lab, device) / lab.shape[0]


def point_estimate(labels, loss="binder", device=0):
    """The draw that minimises the posterior expected loss over the draws:
    ``(labels[best], best, expected_loss)`` with ``expected_loss = sum / S``.
    ``loss="binder"`` is ``mcclust::minbinder(method="draws")``; ``loss="vi"``
    minimises the exact expected VI over the draws (not ``minVI``'s lower
    bound)."""
    if loss not in ("binder", "vi"):
        raise ValueError('loss must be "binder" or "vi"')
    lab = _labels(labels)
    c = compare(lab, device)
    best = c["best_" + loss]
    return lab[best].copy(), best, float(c[loss + "_sum"][best]) / lab.shape[0]
