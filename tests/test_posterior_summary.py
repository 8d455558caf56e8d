"""Posterior clustering summary (mvc_amd.posterior): pairwise Binder distance
and VI of the draws, expected losses and their argmins, the posterior
similarity matrix, and the labels of a result gathered on the device.

The reference here is numpy alone, written without the device code:
contingency tables by np.add.at, B from the pair sums, VI by math.fsum (an
exactly rounded sum), the PSM by broadcasting.  mcclust / mcclust.ext are R
packages absent here; the formulas are those of include/mvc.h.

Integer outputs (binder, binder_sum, best_binder, PSM counts) must match the
reference bit for bit.  VI is allowed the recursive-summation bound

    |vi - ref| <= 4 (m + 4) 2^-52 sum|terms| / (n ln 2)

with m the nonzero cells and margins of the pair (the device adds m terms in
some fixed order, each from a 1-ulp log; the reference's fsum is exact);
vi_sum the sum of its row's bounds.
"""
import ctypes
import math

import numpy as np
import pytest

LN2 = math.log(2.0)


# --------------------------------------------------------------------------
# numpy reference
# --------------------------------------------------------------------------
def ref_pair(a, b):
    """(B, VI in bits, VI bound) of two labelings."""
    n = a.size
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    tab = np.zeros((ua.size, ub.size), dtype=np.int64)
    np.add.at(tab, (ia.ravel(), ib.ravel()), 1)
    rows, cols = tab.sum(1), tab.sum(0)

    def c2(x):
        return int((x * (x - 1) // 2).sum())

    def xlnx(x):
        x = x[x > 0].astype(np.float64)
        return [float(v) for v in x * np.log(x)], x.size

    B = c2(rows) + c2(cols) - 2 * c2(tab)
    tr, mr = xlnx(rows)
    tc, mc = xlnx(cols)
    tj, mj = xlnx(tab.ravel())
    terms = tr + tc + [-2.0 * v for v in tj]
    vi = math.fsum(terms) / n / LN2
    bound = 4.0 * (mr + mc + mj + 4) * 2.0 ** -52 * math.fsum(abs(v) for v in terms) / (n * LN2)
    return B, vi, bound


def ref_compare(labels):
    labels = np.asarray(labels)
    S = labels.shape[0]
    binder = np.zeros((S, S), dtype=np.uint64)
    vi = np.zeros((S, S))
    bound = np.zeros((S, S))
    for s in range(S):
        for t in range(s + 1, S):
            B, v, e = ref_pair(labels[s], labels[t])
            binder[s, t] = binder[t, s] = B
            vi[s, t] = vi[t, s] = v
            bound[s, t] = bound[t, s] = e
    bsum = binder.sum(1, dtype=np.uint64)
    vsum = np.array([math.fsum(vi[s]) for s in range(S)])
    return {"binder": binder, "vi": vi, "bound": bound, "binder_sum": bsum, "vi_sum": vsum,
            "best_binder": int(np.argmin(bsum)), "best_vi": int(np.argmin(vsum))}


def ref_psm_counts(labels):
    labels = np.asarray(labels)
    return (labels[:, :, None] == labels[:, None, :]).sum(0).astype(np.uint32)


# --------------------------------------------------------------------------
# inputs (the GPU cases) and their references, computed once
# --------------------------------------------------------------------------
def _lds_cells():
    from mvc_amd import posterior
    return posterior.LDS_CELLS


def _case(name):
    rng = np.random.default_rng(11)
    if name == "s7_n257":          # n no multiple of the wave or the block; 1..8 clusters per draw; LDS path
        ks = [1, 2, 3, 4, 5, 6, 7]
        ks[6] = 8
        return np.stack([rng.integers(0, k, 257) for k in ks])
    if name == "s2_n1":
        return np.array([[5], [-2]])
    if name == "s1_n50":
        return rng.integers(0, 4, (1, 50))
    if name == "block_vs_singletons_n300":     # ranges 1 and 300
        return np.stack([np.zeros(300, int), np.arange(300)])
    if name == "lds_limit_under":  # 1 * n + 1 + n = LDS_CELLS - 1 words: the widest pair the LDS kernel takes
        n = (_lds_cells() - 1) // 2
        return np.stack([np.full(n, 7), np.arange(n)])
    if name == "lds_limit_over":   # one label more: the same shape through global scratch
        n = (_lds_cells() - 1) // 2 + 1
        return np.stack([np.full(n, 7), np.arange(n)])
    if name == "offsets":          # negative and offset labels, as tests/test_ari.py
        return np.stack([rng.integers(-3, 3, 257), rng.integers(100, 140, 257), rng.integers(-3, 3, 257)])
    if name == "mixed_paths":      # 3000 x 500 goes through global scratch, the other pairs through LDS
        n = 200_000
        return np.stack([rng.integers(0, 3000, n), rng.integers(0, 5, n), rng.integers(0, 500, n),
                         rng.integers(0, 5, n)])
    if name == "winner_front":     # one draw three times among five, the copies first
        a, b, c = rng.integers(0, 4, 120), rng.integers(0, 3, 120), rng.integers(0, 6, 120)
        return np.stack([a, a, a, b, c])
    if name == "winner_spread":    # the same draws, the copies apart
        x = _case("winner_front")
        return x[[0, 3, 1, 4, 2]]
    raise KeyError(name)


COMPARE_CASES = ["s7_n257", "s2_n1", "s1_n50", "block_vs_singletons_n300", "lds_limit_under", "lds_limit_over",
                 "offsets", "mixed_paths"]
_REF = {}


def _ref(name):
    if name not in _REF:
        lab = _case(name)
        lab.flags.writeable = False
        r = ref_compare(lab)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _REF[name] = (lab, r)
    return _REF[name]


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_reference_agrees_with_brute_force():
    rng = np.random.default_rng(3)
    lab = np.stack([rng.integers(0, k, 23) for k in (1, 2, 3, 5, 4)])
    S = lab.shape[0]
    r = ref_compare(lab)
    same = lab[:, :, None] == lab[:, None, :]                  # [S, n, n]
    iu = np.triu_indices(lab.shape[1], 1)
    for s in range(S):
        for t in range(S):
            assert int(r["binder"][s, t]) == int((same[s] != same[t])[iu].sum())
    # minbinder's loss of a draw, sum_{i<j} |1(c_i = c_j) - psm_ij|, is linear in the draws behind the PSM,
    # so it equals the mean over t of B(s, t)
    psm = ref_psm_counts(lab) / S
    for s in range(S):
        loss = np.where(same[s], 1.0 - psm, psm)[iu].sum()
        assert math.isclose(loss, int(r["binder_sum"][s]) / S, rel_tol=1e-12, abs_tol=1e-12)
    assert r["best_binder"] == int(np.argmin([np.where(same[s], 1.0 - psm, psm)[iu].sum() for s in range(S)]))


def test_reference_known_answers():
    B, vi, _ = ref_pair(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]))
    assert B == 4 and vi == 2.0
    B, vi, _ = ref_pair(np.array([3, 3, 9]), np.array([1, 1, 0]))     # the same partition
    assert B == 0 and vi == 0.0
    assert np.array_equal(ref_psm_counts(np.array([[0, 0, 1], [0, 1, 1]])), [[2, 1, 0], [1, 2, 1], [0, 1, 2]])


def _hand_result(rng, S, n, V):
    tab, dish = [], []
    for _ in range(S):
        T = int(rng.integers(1, 7))
        t = rng.integers(0, T, n)
        t[:T] = np.arange(T)                                   # every table occupied
        tab.append(t.astype(np.int32))
        dish.append([rng.integers(0, 40, T).astype(np.int32) for _ in range(V)])   # raw ids with gaps
    return {"table_of": tab, "dish_of": dish}


def test_draws_match_get_final_clusters():
    import mvc_amd
    from mvc_amd import posterior
    rng = np.random.default_rng(5)
    S, n, V = 6, 31, 3
    chains = [_hand_result(rng, S, n, V), _hand_result(rng, S, n, V)]
    for res in (chains[0], chains):
        pool = [res] if isinstance(res, dict) else res
        want_t = np.stack([r["table_of"][s] for r in pool for s in range(S)])
        got = posterior.draws(res)
        assert got.dtype == np.int32 and np.array_equal(got, want_t)
        for v in range(V):
            want = np.stack([mvc_amd.get_final_clusters({"table_of": r["table_of"][:s + 1],
                                                         "dish_of": r["dish_of"][:s + 1]})[:, v]
                             for r in pool for s in range(S)])
            got = posterior.draws(res, view=v)
            assert got.dtype == np.int32 and got.shape == (len(pool) * S, n) and np.array_equal(got, want)
            comp = posterior.draws(res, view=v, compact=True)
            for a, b in zip(comp, want):                       # the same partition, labels 0..K-1 in raw-id order
                assert np.array_equal(a, np.unique(b, return_inverse=True)[1].reshape(b.shape))


def test_posterior_host_code_under_sanitizers(tmp_path):
    """The host-only pieces (dish-id compaction, the split of the pairs between
    the LDS and the global-scratch kernels) as a stand-alone program under
    AddressSanitizer and UBSan."""
    import os
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "posterior_host_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "include"), "-I", os.path.join(root, "multiview-clustering_amd", "csrc"),
                        "-o", str(exe), os.path.join(root, "tests", "posterior_host_check.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", COMPARE_CASES)
def test_compare_integers_bitwise(name):
    from mvc_amd import posterior
    lab, ref = _ref(name)
    out = posterior.compare(lab)
    S = lab.shape[0]
    assert out["binder"].dtype == np.uint64 and out["binder"].shape == (S, S)
    assert np.array_equal(out["binder"], out["binder"].T) and not out["binder"].diagonal().any()
    assert np.array_equal(out["binder"], ref["binder"])
    assert np.array_equal(out["binder_sum"], ref["binder_sum"])
    assert out["best_binder"] == ref["best_binder"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", COMPARE_CASES)
def test_compare_vi_within_derived_bound(name):
    from mvc_amd import posterior
    lab, ref = _ref(name)
    out = posterior.compare(lab)
    err = np.abs(out["vi"] - ref["vi"])
    print(f"{name}: max |vi - ref| / bound = {np.max(err / np.where(ref['bound'] > 0, ref['bound'], 1.0)):.3g}, "
          f"max |vi - ref| = {err.max():.3g}")
    assert np.array_equal(out["vi"], out["vi"].T) and not out["vi"].diagonal().any()
    assert (err <= ref["bound"]).all()
    row_bound = ref["bound"].sum(1)
    assert (np.abs(out["vi_sum"] - ref["vi_sum"]) <= row_bound).all()
    b = out["best_vi"]
    assert 0 <= b < lab.shape[0]
    assert ref["vi_sum"][b] - ref["vi_sum"].min() <= row_bound[b]
    again = posterior.compare(lab)                             # no floating-point atomics: the same bits
    assert np.array_equal(out["vi"].view(np.uint64), again["vi"].view(np.uint64))
    assert np.array_equal(out["vi_sum"].view(np.uint64), again["vi_sum"].view(np.uint64))


@pytest.mark.gpu
def test_compare_clear_winner():
    """One draw three times among five.  With the copies first their rows are
    the same terms added in the same order, so their vi_sum tie exactly and
    the lowest index wins, as in the reference.  With the copies apart the
    rows are equal only up to the rounding of a transposed table's sum, so any
    copy may win; it must be a copy."""
    from mvc_amd import posterior
    lab, ref = _ref("winner_front")
    out = posterior.compare(lab)
    assert ref["best_vi"] == 0 and ref["best_binder"] == 0
    assert out["best_vi"] == ref["best_vi"]
    assert out["best_binder"] == ref["best_binder"]
    est, best, loss = posterior.point_estimate(lab, "vi")
    assert best == 0 and np.array_equal(est, lab[0])
    assert abs(loss - ref["vi_sum"][0] / 5) <= ref["bound"].sum(1)[0] / 5
    est, best, loss = posterior.point_estimate(lab, "binder")
    assert best == 0 and np.array_equal(est, lab[0]) and loss == int(ref["binder_sum"][0]) / 5
    lab2, ref2 = _ref("winner_spread")
    out2 = posterior.compare(lab2)
    assert out2["best_vi"] in (0, 2, 4) and out2["best_binder"] == 0 == ref2["best_binder"]


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", [(1, 4), (65, 5), (200, 33), (257, 3)])
def test_psm_counts_bitwise(n, S):
    from mvc_amd import posterior
    rng = np.random.default_rng(n + S)
    lab = np.stack([rng.integers(-2, 1 + s % 7, n) for s in range(S)])
    ref = ref_psm_counts(lab)
    got = posterior.psm_counts(lab)
    assert got.dtype == np.uint32 and np.array_equal(got, ref)
    assert np.array_equal(got, got.T) and (got.diagonal() == S).all()
    p = posterior.psm(lab)
    assert p.dtype == np.float64 and np.array_equal(p.view(np.uint64), (ref / S).view(np.uint64))


@pytest.mark.gpu
def test_psm_refuses_n_above_the_cap():
    from mvc_amd import MvcError, posterior
    from mvc_amd import _lib as L
    n = posterior.PSM_MAX_N + 1
    assert n == 16385
    with pytest.raises(MvcError) as e:
        posterior.psm(np.zeros((2, n), dtype=np.int32))        # refused before the 1 GiB of counts exist anywhere
    assert e.value.code == L.MVC_ERR_UNSUPPORTED and "MVC_POSTERIOR_PSM_MAX_N" in str(e.value)


@pytest.mark.gpu
def test_end_to_end_estimate_of_a_run():
    """run_gibbs_cpp on the reference's shape (New_Simulation.R:47-60), then
    the port of its :189: the ARI of the Binder / VI estimate per view."""
    import mvc_amd
    from mvc_amd import data, posterior
    y, truth = data.new_simulation(1999)
    V, n = y.shape
    dev = {}
    res = mvc_amd.run_gibbs_cpp(y, 60, 10, 1, seed=7, mode="parallel", n_chains=2, quiet=True, labels=dev)
    S = len(res[0]["table_of"])
    assert S == 50 and sorted(dev) == list(range(-1, V))
    assert np.array_equal(dev[-1], posterior.draws(res))
    for v in range(V):
        assert dev[v].shape == (2 * S, n)
        assert np.array_equal(dev[v], posterior.draws(res, view=v, compact=True))
        raw = posterior.draws(res, view=v)
        for loss in ("binder", "vi"):
            est, best, exp_loss = posterior.point_estimate(raw, loss)
            assert np.array_equal(est, raw[best]) and math.isfinite(exp_loss) and exp_loss >= 0.0
            ari = mvc_amd.ari(est, truth[v])
            assert math.isfinite(ari)
            # the compacted draws are the same partitions: the same Binder choice
            if loss == "binder":
                assert posterior.point_estimate(dev[v], loss)[1] == best


@pytest.mark.gpu
def test_argument_errors():
    import mvc_amd
    from mvc_amd import _lib as L
    from mvc_amd import posterior
    from mvc_amd.sampler import _view_ptrs, make_config
    lib = L.lib()
    ip = ctypes.POINTER(ctypes.c_int32)
    for bad in (np.zeros((0, 5), dtype=np.int32), np.zeros((3, 0), dtype=np.int32)):
        for fn in (posterior.compare, posterior.psm):
            with pytest.raises(mvc_amd.MvcError) as e:
                fn(bad)
            assert e.value.code == L.MVC_ERR_ARG and "must be >= 1" in str(e.value)
    with pytest.raises(mvc_amd.MvcError) as e:
        posterior.compare(np.zeros((posterior.MAX_DRAWS + 1, 1), dtype=np.int32))
    assert e.value.code == L.MVC_ERR_ARG and "MVC_POSTERIOR_MAX_DRAWS" in str(e.value)
    buf = L.errbuf()
    assert lib.mvc_partition_compare(0, None, 2, 2, None, None, None, None, None, buf, len(buf)) == L.MVC_ERR_ARG
    assert b"NULL" in buf.value
    buf = L.errbuf()
    assert lib.mvc_partition_psm(0, None, 2, 2, None, buf, len(buf)) == L.MVC_ERR_ARG and b"NULL" in buf.value
    lab = np.zeros((2, 2), dtype=np.int32)
    buf = L.errbuf()
    assert lib.mvc_partition_psm(0, lab.ctypes.data_as(ip), 2, 2, None, buf, len(buf)) == L.MVC_ERR_ARG
    assert b"counts is NULL" in buf.value
    # every output of compare may be NULL
    buf = L.errbuf()
    assert lib.mvc_partition_compare(0, lab.ctypes.data_as(ip), 2, 2, None, None, None, None, None, buf,
                                     len(buf)) == L.MVC_OK
    # mvc_result_labels: NULL result, NULL output, level outside [-1, V)
    buf = L.errbuf()
    assert lib.mvc_result_labels(None, -1, lab.ctypes.data_as(ip), buf, len(buf)) == L.MVC_ERR_ARG
    assert b"NULL" in buf.value
    y = np.random.default_rng(0).normal(size=(2, 12, 1))
    cfg = make_config(12, 2, 1, M=3, mode="parallel")
    res = ctypes.c_void_p()
    buf = L.errbuf()
    L.check(lib.mvc_run(ctypes.byref(cfg), _view_ptrs(y), ctypes.byref(res), buf, len(buf)), buf)
    try:
        out = np.empty((3, 12), dtype=np.int32)
        for level in (-2, 2):
            buf = L.errbuf()
            assert lib.mvc_result_labels(res, level, out.ctypes.data_as(ip), buf, len(buf)) == L.MVC_ERR_ARG
            assert b"level" in buf.value
        buf = L.errbuf()
        assert lib.mvc_result_labels(res, 0, None, buf, len(buf)) == L.MVC_ERR_ARG and b"NULL" in buf.value
        buf = L.errbuf()
        assert lib.mvc_result_labels(res, 1, out.ctypes.data_as(ip), buf, len(buf)) == L.MVC_OK
    finally:
        lib.mvc_result_free(res)
