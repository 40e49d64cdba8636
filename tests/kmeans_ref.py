"""NumPy restatement of the IVF training the device runs (rvc_amd/index_train.py + csrc/kmeans.hip), from faiss's
published Clustering.cpp / utils/random.cpp -- written apart from the package, which the tests compare against it:

  rand_perm          std::mt19937(seed), for i < n - 1 swap i with i + mt() % (n - i)
  dist64             f64 squared distances [n][k]
  tolerance          tol_i = 2 (d + 2) 2^-24 (||x_i|| + max_j ||c_j||)^2: the first-order worst case of an f32
                     product chain of length d, the two f32 norms and the final subtraction, doubled because two
                     candidates are compared; it holds for any summation order and is derived, not measured
  update             per centroid the f32 sum of its rows in ascending row order from 0 (np.cumsum adds
                     sequentially), times f32 1 / count; empty lists keep the previous centroid
  split              faiss split_clusters with std::mt19937(seed), rand_float = mt() / float(mt.max())
"""
import numpy as np


def mt_raw(seed, count):
    return np.random.RandomState(seed)._bit_generator.random_raw(count)


def rand_perm(n, seed):
    perm = list(range(n))
    raw = mt_raw(seed, max(n - 1, 1))
    for i in range(n - 1):
        j = i + int(raw[i]) % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm, dtype=np.int64)


def clustered(n, d, nclusters, seed, spread=0.3):
    """Clustered Gaussians: nclusters unit-variance centres, rows = a centre + spread * noise, f32."""
    g = np.random.default_rng(seed)
    centres = g.standard_normal((nclusters, d))
    x = centres[g.integers(0, nclusters, n)] + spread * g.standard_normal((n, d))
    return np.ascontiguousarray(x, dtype=np.float32)


def dist64(x, c):
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    d2 = (x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :]
    return np.maximum(d2, 0.0)


def tolerance(x, c):
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    d = x.shape[1]
    return 2.0 * (d + 2) * 2.0 ** -24 * (np.sqrt((x * x).sum(1)) + np.sqrt((c * c).sum(1)).max()) ** 2


def check_assign(x, c, assign, dist=None, cap=0.005):
    """The acceptance rule of an assignment; returns the rows that differ from the f64 argmin (near ties)."""
    d2 = dist64(x, c)
    tol = tolerance(x, c)
    n = x.shape[0]
    assign = np.asarray(assign, np.int64)
    assert assign.shape == (n,) and assign.min() >= 0 and assign.max() < c.shape[0]
    got = d2[np.arange(n), assign]
    excess = got - d2.min(1)
    worst = int(np.argmax(excess - tol))
    assert (excess <= tol).all(), (worst, excess[worst], tol[worst])
    differ = np.nonzero(assign != d2.argmin(1))[0]
    assert len(differ) <= cap * n, (len(differ), n)
    if dist is not None:
        err = np.abs(np.asarray(dist, np.float64) - got)
        assert (err <= tol).all(), (err.max(), tol[np.argmax(err - tol)])
    return differ


def lists(assign, k):
    """(list_off [k + 1], ids [n]): the stable sort of the rows by list."""
    assign = np.asarray(assign, np.int64)
    ids = np.argsort(assign, kind="stable").astype(np.int64)
    off = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(assign, minlength=k), out=off[1:])
    return off, ids


def update(x, assign, k, prev):
    x = np.asarray(x, np.float32)
    off, ids = lists(assign, k)
    out = np.array(prev, dtype=np.float32, copy=True)
    for j in range(k):
        m = ids[off[j]:off[j + 1]]
        if len(m):
            s = np.cumsum(x[m], axis=0, dtype=np.float32)[-1]
            out[j] = s * (np.float32(1.0) / np.float32(len(m)))
    return out, np.diff(off)


def split(cent, counts, n, seed=1234):
    """faiss split_clusters on f32 centroids [k][d] (in place); returns the number of splits."""
    k, d = cent.shape
    h = np.asarray(counts, np.float32).copy()
    if not (h == 0).any():
        return 0
    gen = np.random.RandomState(seed)._bit_generator
    eps = np.float32(1.0 / 1024.0)
    one = np.float32(1.0)
    even = np.arange(d) % 2 == 0
    nsplit = 0
    for ci in range(k):
        if h[ci] != 0:
            continue
        cj = 0
        while True:
            p = np.float32((float(h[cj]) - 1.0) / float(np.float32(n - k)))
            r = np.float32(gen.random_raw()) / np.float32(4294967295)
            if r < p:
                break
            cj = (cj + 1) % k
        cent[ci] = cent[cj]
        cent[ci] = np.where(even, cent[ci] * (one + eps), cent[ci] * (one - eps))
        cent[cj] = np.where(even, cent[cj] * (one - eps), cent[cj] * (one + eps))
        h[ci] = h[cj] / np.float32(2)
        h[cj] -= h[ci]
        nsplit += 1
    return nsplit


def lloyd_step(x, cent, seed=1234):
    """One restated iteration with the f64 argmin: (new centroids, assignment, f64 objective, splits)."""
    d2 = dist64(x, cent)
    assign = d2.argmin(1)
    obj = float(d2[np.arange(len(assign)), assign].sum())
    new, counts = update(x, assign, cent.shape[0], cent)
    nsplit = split(new, counts, x.shape[0], seed)
    return new, assign, obj, nsplit


def objective(x, cent, assign):
    return float(dist64(x, cent)[np.arange(len(assign)), np.asarray(assign, np.int64)].sum())
