"""Reuters-21578 views for BASELINE config 3.

The three count views of dataset/reuters/data pre-process.R:50-108 (body DTM,
title DTM, binary <D> values) are built by scripts/reuters_build.py and
committed as CSR counts under tests/golden/reuters/ (reuters_counts.npz and
the body view's column indices in BODY_PARTS pieces, every file below
1 MiB; 2.3 MB in all).  The R script stops at
the count matrices (it never calls the sampler); feeding them to the Gaussian
sampler is this build's choice:

    x = log1p(counts)  ->  x @ R_v,  R_v ~ N(0, 1/D) iid, Philox-free numpy
    PCG64 stream seeded per view (seed, v)  ->  D = 64 dims per view.

The clustering is scored (mcclust::arandi, as New_Simulation.R:189 scores
its clusters) against the 6 most frequent TOPICS labels: documents whose
TOPICS hold exactly one of them; the other documents are clustered but not
scored.

Label leak: the reference's third view holds every <D> value of a document
(pre-process.R:88-102), and the TOPICS values (the ARI truth) are <D> values
too -- 120 of its 445 columns.  views(..., drop_topics=True) zeroes those 120
columns (the random projection then never sees them), so an ARI computed on
it measures clustering from the other fields (body, title, PLACES, PEOPLE,
ORGS, EXCHANGES) alone.  The default keeps the reference's view.

Scale: views(..., standardize=True) centres every projected dimension and
scales it to unit variance.  The raw title and <D> projections are 5-14x
narrower than the reference's N(0, 1) prior on the dish means (DESIGN.md §6:
on them the model keeps most documents in near-singleton tables, ARI ~0.002).
"""
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DATA_DIR = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tests", "golden", "reuters")
COUNTS = os.path.join(DATA_DIR, "reuters_counts.npz")
BODY_PARTS = 3


def body_part(k, data_dir=DATA_DIR):
    """File of piece k of body_indices (consecutive slices, np.array_split)."""
    return os.path.join(data_dir, f"reuters_body_indices_{k}.npz")


def _load():
    """Every array of the committed counts by name; body_indices joined from its pieces."""
    with np.load(COUNTS) as z:
        d = {k: z[k] for k in z.files}
    parts = []
    for k in range(BODY_PARTS):
        with np.load(body_part(k)) as p:
            parts.append(p["body_indices"])
    d["body_indices"] = np.concatenate(parts)
    return d


def _csr(z, name, ncol):
    from scipy.sparse import csr_matrix
    indptr = z[f"{name}_indptr"]
    indices = z[f"{name}_indices"]
    data = z[f"{name}_data"] if f"{name}_data" in z else np.ones(indices.size, np.uint16)
    return csr_matrix((data.astype(np.float64), indices, indptr), shape=(indptr.size - 1, int(ncol)))


def counts():
    """(body, title, topics) count matrices (scipy CSR, documents x terms)."""
    z = _load()
    return (_csr(z, "body", z["body_terms"]), _csr(z, "title", z["title_terms"]),
            _csr(z, "topics", z["topics_terms"]))


def topics_columns():
    """Column indices of the third view whose <D> value is a TOPICS value."""
    with np.load(COUNTS) as z:
        names, topics = z["topics_names"], set(z["label_names"].tolist())
    return np.array([j for j, x in enumerate(names.tolist()) if x in topics], np.int64)


def views(D=64, seed=2026, drop_topics=False, standardize=False):
    """float64 [3][N][D]: log1p(counts) @ R_v per view, R_v ~ N(0, 1/D).
    drop_topics: zero the third view's TOPICS columns (the ARI truth) first.
    standardize: every projected dimension centred and scaled to unit
    variance, the scale of New_Simulation.R:47-60's data under the
    reference's N(0, 1) dish-mean prior (multiview_utils.cpp:307-338; the raw
    projections have per-dimension standard deviations of 0.65-0.96 (body),
    0.18-0.22 (title) and 0.07-0.15 (<D> values), and means up to 0.7)."""
    out = []
    for v, X in enumerate(counts()):
        X = X.copy()
        X.data = np.log1p(X.data)
        if v == 2 and drop_topics:
            keep = np.ones(X.shape[1])
            keep[topics_columns()] = 0.0
            X = X.multiply(keep[None, :]).tocsr()
        R = np.random.default_rng([seed, v]).standard_normal((X.shape[1], D)) / np.sqrt(D)
        Y = np.asarray(X @ R)
        if standardize:
            sd = Y.std(axis=0)
            Y = (Y - Y.mean(axis=0)) / np.where(sd > 0, sd, 1.0)
        out.append(np.ascontiguousarray(Y))
    return np.stack(out)


def topic_truth(top=6):
    """(labels[N] int32: index among the `top` most frequent TOPICS when the
    document has exactly one of them, else -1; their names; their counts)."""
    with np.load(COUNTS) as z:
        indptr, indices, names = z["label_indptr"], z["label_indices"], z["label_names"]
    N = indptr.size - 1
    freq = np.bincount(indices, minlength=names.size)
    order = np.argsort(-freq, kind="stable")[:top]
    rank = np.full(names.size, -1, np.int32)
    rank[order] = np.arange(top)
    lab = np.full(N, -1, np.int32)
    for i in range(N):
        r = rank[indices[indptr[i]:indptr[i + 1]]]
        r = r[r >= 0]
        if r.size == 1:
            lab[i] = r[0]
    return lab, [str(names[k]) for k in order], freq[order].tolist()
