"""NumPy restatement of the MiniBatchKMeans reduction the device runs (rvc_amd/index_train.py + csrc/minibatch.hip):
sklearn 1.7.2 ``MiniBatchKMeans(n_clusters, batch_size=..., compute_labels=False, init="random").fit`` on dense rows
with unit sample weights, from sklearn's ``_kmeans.py`` and ``_k_means_minibatch.pyx`` -- written apart from the
package, which the tests compare against it.

  draws      one ``numpy.random.RandomState``, in sklearn's order: the validation rows; per init the candidate rows
             (only if init_size < n) and ``choice(m, k, replace=False, p=ones(m, f32) / m)``; per step the batch
             and, on a reassigning step with centres to reassign, ``choice(bs, replace=False, size=...)``
  labels     the f64 argmin of the squared distances sum((x - c)^2), the lowest index on equal values
  inertia    the f64 sum of those distances (sklearn sums f32 values: the fixtures keep to runs whose stopping rule
             is decided by more than 1e-6 relative, ``min_ewa_gap``)
  update     per centre with members: row = centre * weight (f32, rounded), += the members in batch order (f32),
             weight += members, row *= f32(1) / weight; no member: copied
  reassign   ``to = w < f32(ratio) * w.max()``, trimmed to 0.5 bs by ``np.argsort(w)``; the chosen batch rows
             replace the centres; ``w[to] = w[~to].min()``

It records per step the smallest gap between a row's best and next different squared distance (``gap``), that gap
over ``kmeans_ref.tolerance`` (``gap_tol``: above 1 the device's f32 assignment must agree), and over the run the
smallest relative distance |ewa - ewa_min| / ewa_min of a stopping-rule comparison (``min_ewa_gap``).
"""
import os

import numpy as np

import kmeans_ref as kr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"A": (3000, 16, 40, 256), "B": (2000, 8, 10, 4096), "C": (20000, 16, 200, 64)}  # (n, d, k, batch_size)
QUALITY = (5000, 32, 300, 128)
QUALITY_SEEDS = tuple(range(8))
DATA_SEED = {"A": 101, "B": 102, "C": 103, "Q": 104}


def blobs(n, d, seed, nclusters=25):
    """f32 rows of ``nclusters`` Gaussian clusters: centres 4 N(0, 1), unit noise."""
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.standard_normal((nclusters, d))
    x = centres[rs.randint(0, nclusters, n)] + rs.standard_normal((n, d))
    return np.ascontiguousarray(x, dtype=np.float32)


def sizes(n, k, batch_size, max_iter=100):
    bs = min(int(batch_size), n)
    init_size = 3 * bs
    if init_size < k:
        init_size = 3 * k
    return bs, min(init_size, n), (max_iter * n) // bs


def sqdist(x, c, chunk=1 << 22):
    """f64 [n][k] of sum((x - c)^2) over the dimensions, from the operands as they are stored."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    rows = max(1, chunk // (c.shape[0] * x.shape[1]))
    for i in range(0, x.shape[0], rows):
        e = x[i:i + rows, None, :] - c[None, :, :]
        out[i:i + rows] = (e * e).sum(-1)
    return out


def labels_inertia(x, c):
    d2 = sqdist(x, c)
    labels = d2.argmin(1)
    return labels.astype(np.int32), float(d2[np.arange(len(labels)), labels].sum()), d2


def inertia(x, c, labels):
    """The f64 inertia of given labels."""
    e = np.asarray(x, np.float64) - np.asarray(c, np.float64)[np.asarray(labels, np.int64)]
    return float((e * e).sum(1).sum())


def full_inertia(x, c):
    """The f64 inertia of all rows against their nearest centres (the quality figure)."""
    return float(sqdist(x, c).min(1).sum())


def decision_gap(d2, x, c):
    """(smallest gap best -> next different value over the rows, smallest gap / tolerance)."""
    best = d2.min(1)
    rest = np.where(d2 > best[:, None], d2, np.inf).min(1)
    gap = rest - best
    return float(gap.min()), float((gap / kr.tolerance(x, c)).min())


def update(xb, labels, cent, weights):
    """_minibatch_update_dense: (new centres, new weights), f32, the inputs untouched."""
    xb = np.asarray(xb, np.float32)
    new = np.array(cent, dtype=np.float32, copy=True)
    w = np.array(weights, dtype=np.float32, copy=True)
    labels = np.asarray(labels, np.int64)
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    for m in np.split(order, cuts):
        c = labels[m[0]]
        row = new[c] * w[c]
        row = np.cumsum(np.vstack([row[None, :], xb[m]]), axis=0, dtype=np.float32)[-1]  # sequential f32 adds
        w[c] = w[c] + np.float32(len(m))
        new[c] = row * (np.float32(1.0) / w[c])
    return new, w


def fma_case():
    """(centres [2][8], weights [2], batch [2][8], both rows in centre 0) on which contracting centre * weight + x
    into an fma changes the result: f32(1/3) * 3 = 1 + 2^-25 exactly, which rounds to 1, and 1 + 0.75 * 2^-24 stays
    1; one rounding of the exact 1 + 1.25 * 2^-24 gives 1 + 2^-23."""
    cent = np.array([[np.float32(1) / np.float32(3)] * 8, [0.5] * 8], np.float32)
    w = np.array([3.0, 0.0], np.float32)
    xb = np.zeros((2, 8), np.float32)
    xb[0] = np.float32(0.75 * 2.0 ** -24)
    return cent, w, xb


def reassign(xb, cent, weights, rs, ratio=0.01):
    """The reassignment of ``_mini_batch_step`` in place on cent / weights: (centres, batch rows they took)."""
    bs = xb.shape[0]
    to = weights < np.float32(ratio) * weights.max()
    if to.sum() > 0.5 * bs:
        to[np.argsort(weights)[int(0.5 * bs):]] = False
    picked = np.zeros(0, np.int64)
    if to.sum():
        picked = np.asarray(rs.choice(bs, replace=False, size=int(to.sum())), np.int64)
        cent[to] = xb[picked]
    weights[to] = np.min(weights[~to])
    return np.nonzero(to)[0].astype(np.int64), picked


def fit(x, k, batch_size, random_state, max_iter=100, max_no_improvement=10, ratio=0.01, n_init=3, stop_after=None,
        states=()):
    """The run.  Returns (centres, hist): hist["n_steps"], ["min_ewa_gap"], ["init"] (the centres before step 0) and
    per step ["batch"], ["labels"], ["inertia"], ["reassign"] (the step's flag), ["to"], ["picked"], ["gap"],
    ["gap_tol"].  For the steps in ``states``, hist["state"][i] = (centres before, weights before, centres after,
    weights after).  ``stop_after`` ends the run after that many steps."""
    x = np.ascontiguousarray(x)
    n = x.shape[0]
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    bs, init_size, n_steps = sizes(n, k, batch_size, max_iter)
    valid = rs.randint(0, n, init_size)
    best = cent = None
    for _ in range(n_init):
        cand = x[rs.randint(0, n, init_size)] if init_size < n else x
        w = np.ones(cand.shape[0], x.dtype)
        trial = cand[rs.choice(cand.shape[0], size=k, replace=False, p=w / w.sum())]
        val = labels_inertia(x[valid], trial)[1]
        if best is None or val < best:
            best, cent = val, trial
    cent = np.array(cent, copy=True)
    weights = np.zeros(k, x.dtype)
    hist = {"init": cent.copy(), "batch": [], "labels": [], "inertia": [], "reassign": [], "to": [], "picked": [],
            "gap": [], "gap_tol": [], "state": {}, "n_steps": 0, "min_ewa_gap": np.inf}
    ewa = ewa_min = None
    no_improvement = since = 0
    alpha = min(bs * 2.0 / (n + 1), 1)
    states = set(states)
    for i in range(n_steps if stop_after is None else min(n_steps, stop_after)):
        batch = rs.randint(0, n, bs)
        xb = x[batch]
        since += bs
        flag = bool((weights == 0).any() or since >= 10 * k)
        if flag:
            since = 0
        labels, val, d2 = labels_inertia(xb, cent)
        gap, gap_tol = decision_gap(d2, xb, cent)
        new, new_w = update(xb, labels, cent, weights)
        to = picked = np.zeros(0, np.int64)
        if flag and ratio > 0:
            to, picked = reassign(xb, new, new_w, rs, ratio)
        if i in states:
            hist["state"][i] = (cent, weights, new.copy(), new_w.copy())
        cent, weights = new, new_w
        for key, v in (("batch", batch), ("labels", labels), ("inertia", val), ("reassign", flag), ("to", to),
                       ("picked", picked), ("gap", gap), ("gap_tol", gap_tol)):
            hist[key].append(v)
        hist["n_steps"] = i + 1
        if i == 0:
            continue
        b = val / bs
        ewa = b if ewa is None else ewa * (1 - alpha) + b * alpha
        if ewa_min is not None:
            hist["min_ewa_gap"] = min(hist["min_ewa_gap"], abs(ewa - ewa_min) / ewa_min)
        if ewa_min is None or ewa < ewa_min:
            no_improvement, ewa_min = 0, ewa
        else:
            no_improvement += 1
        if max_no_improvement is not None and no_improvement >= max_no_improvement:
            break
    return cent, hist


def load_fixture(name):
    """tests/golden/minibatch_<name>.npz as a dict; rows stored in parts (a file-size limit) are joined."""
    z = dict(np.load(os.path.join(GOLDEN, f"minibatch_{name}.npz"), allow_pickle=False))
    parts = [z.pop("x")] if "x" in z else []
    p = 1
    while os.path.exists(os.path.join(GOLDEN, f"minibatch_{name}_x{p}.npz")):
        parts.append(np.load(os.path.join(GOLDEN, f"minibatch_{name}_x{p}.npz"))["x"])
        p += 1
    if parts:
        z["x"] = np.ascontiguousarray(np.concatenate(parts, axis=0))
    return z
