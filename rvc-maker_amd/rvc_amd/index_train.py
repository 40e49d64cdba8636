"""Build the retrieval index on the device: ``main/inference/create_index.py:51-84`` without faiss.

The reference calls ``faiss.index_factory(d, "IVF{n},Flat")``, ``train``, ``add`` in 8192-row batches and
``write_index``.  Training is faiss's ``Clustering::train`` as ``IndexIVF::train`` reaches it (``cp.niter = 10``,
``seed = 1234``, one redo, L2, no subsampling below 256 rows per centroid -- which
``n_ivf = min(int(16 sqrt N), N // 39)`` never reaches for N <= 2e5), restated here from faiss's published
``Clustering.cpp`` / ``utils/random.cpp``:

  initial centroids   ``x[perm[:k]]``, ``perm = rand_perm(n, seed + 1)``: ``std::mt19937(seed + 1)`` and, for
                      ``i < n - 1``, swap ``i`` with ``i + mt() % (n - i)``
  each iteration      assign every row to its nearest centroid; new centroid = f32 sum of its rows in row order
                      times ``1.f / count``; then ``split_clusters``: every empty cluster ``ci`` takes a copy of a
                      cluster ``cj`` drawn with ``std::mt19937(seed)`` (walk ``cj = 0, 1, ...`` cyclically until
                      ``rand_float < (count[cj] - 1) / (n - k)``), the two perturbed by ``1 +- 1/1024`` on alternate
                      dimensions, the count halved between them

Assign, lists, update and the row gathers are kmeans.hip kernels (``ops.kmeans_*``); the host keeps the loop, the
permutation and the split over the k counts, which are read back once per iteration -- the only synchronisation.
faiss is not installed where this is built, so equality with faiss's own centroids is unpinned, like the ``.index``
layout of ``faiss_index.py``; what is pinned is this restatement (tests/kmeans_ref.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
from .faiss_index import IVFFlatIndex
from .retrieval import IVFFlatDevice

EPS = np.float32(1.0 / 1024.0)
MAX_ROWS_FAISS = 2e5  # create_index.py:63: above it "Auto" / "KMeans" first reduce with MiniBatchKMeans


def mt19937_raw(seed: int, count: int) -> np.ndarray:
    """The first ``count`` outputs of ``std::mt19937(seed)`` (numpy's legacy seeding is init_genrand)."""
    return np.random.RandomState(int(seed))._bit_generator.random_raw(int(count)).astype(np.uint64)


def rand_perm(n: int, seed: int) -> np.ndarray:
    """faiss ``rand_perm(perm, n, seed)``."""
    if n < 2:
        return np.arange(n, dtype=np.int64)
    step = (mt19937_raw(seed, n - 1) % (n - np.arange(n - 1, dtype=np.uint64))).tolist()
    perm = list(range(n))  # the swaps depend on one another: a plain loop, on Python ints
    for i, s in enumerate(step):
        j = i + s
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm, dtype=np.int64)


class _Mt19937Floats:
    """``rand_float = mt() / float(mt.max())`` of one ``std::mt19937(seed)``, read ahead in blocks."""

    def __init__(self, seed):
        self.gen = np.random.RandomState(int(seed))._bit_generator
        self.buf = np.zeros(0, np.float32)
        self.pos = 0

    def peek(self, m):
        if self.pos + m > len(self.buf):
            more = self.gen.random_raw(max(m, 1 << 16)).astype(np.uint32).astype(np.float32) / np.float32(4294967295.0)
            self.buf = np.concatenate([self.buf[self.pos:], more])
            self.pos = 0
        return self.buf[self.pos:self.pos + m]

    def skip(self, m):
        self.pos += m


def split_plan(counts: np.ndarray, n: int, seed: int = 1234):
    """faiss ``split_clusters`` over the k counts: the (ci, cj) copies in order; ``counts`` (f32) is updated in
    place as faiss updates ``hassign``.  The walk ``cj = 0, 1, ...`` draws one float per step; it is evaluated a
    cycle of k draws at a time (a walk is about (n - k) / mean count steps long)."""
    k = len(counts)
    plan = []
    empty = np.nonzero(counts == 0)[0]
    if len(empty) == 0:
        return plan
    rnd = _Mt19937Floats(seed)
    denom = np.float64(np.float32(n - k))

    def prob(h):
        return ((np.asarray(h, np.float64) - 1.0) / denom).astype(np.float32)

    p = prob(counts)
    for ci in range(k):
        if counts[ci] != 0:  # a cluster filled by an earlier split of this call stays
            continue
        while True:
            hit = np.nonzero(rnd.peek(k) < p)[0]
            if len(hit):
                cj = int(hit[0])
                rnd.skip(cj + 1)
                break
            rnd.skip(k)
        plan.append((ci, cj))
        counts[ci] = counts[cj] / np.float32(2)
        counts[cj] = counts[cj] - counts[ci]
        p[[ci, cj]] = prob(counts[[ci, cj]])
    return plan


def _apply_splits(cent: torch.Tensor, plan):
    d = cent.shape[1]
    even = (torch.arange(d, device=cent.device) % 2 == 0)
    one = torch.ones(d, device=cent.device)
    up = torch.where(even, one + float(EPS), one - float(EPS))  # ci: even dims * (1 + EPS), odd * (1 - EPS)
    dn = torch.where(even, one - float(EPS), one + float(EPS))  # cj: the opposite
    for ci, cj in plan:
        src = cent[cj].clone()
        cent[ci] = src * up
        cent[cj] = src * dn


def kmeans(x_dev: torch.Tensor, k: int, niter: int = 10, seed: int = 1234, init=None, history: bool = False):
    """faiss ``Clustering::train`` on device rows ``x_dev`` [n][d] f32 -> centroids [k][d] (device).

    ``init`` [k][d] overrides the initial centroids.  ``history=True`` returns ``(centroids, hist)`` with
    ``hist["centroids"]`` (niter + 1 arrays: before every iteration and the result), ``hist["assign"]`` and
    ``hist["objective"]`` (the f64 sum of the f32 distances) per iteration, as NumPy arrays."""
    if x_dev.dim() != 2 or x_dev.dtype != torch.float32 or not x_dev.is_cuda:
        raise TypeError("kmeans: a CUDA f32 [n][d] tensor")
    x = x_dev.contiguous()
    n, d = x.shape
    k = int(k)
    if k < 1 or n < k:
        raise ValueError(f"kmeans: {n} rows cannot train {k} centroids")
    hist = {"centroids": [], "assign": [], "objective": []}
    if n == k:
        cent = x.clone()
        if history:
            hist["centroids"].append(cent.cpu().numpy())
        return (cent, hist) if history else cent
    if init is None:
        perm = rand_perm(n, seed + 1)
        cent = ops.gather_rows(x, torch.from_numpy(perm[:k].copy()).to(x.device))
    else:
        cent = torch.as_tensor(init, dtype=torch.float32).to(x.device).contiguous().clone()
        if tuple(cent.shape) != (k, d):
            raise ValueError(f"kmeans: init must be [{k}][{d}]")
    objs = []
    for _ in range(niter):
        assign, dist = ops.kmeans_assign(x, cent)
        list_off, ids, counts = ops.kmeans_lists(assign, k)
        new = ops.kmeans_update(x, list_off, ids, cent)
        if history:
            hist["centroids"].append(cent)
            hist["assign"].append(assign)
            objs.append(dist.double().sum())
        plan = split_plan(counts.cpu().numpy().astype(np.float32), n, seed)  # the iteration's one synchronisation
        if plan:
            _apply_splits(new, plan)
        cent = new
    if not history:
        return cent
    hist["centroids"] = [c.cpu().numpy() for c in hist["centroids"]] + [cent.cpu().numpy()]
    hist["assign"] = [a.cpu().numpy() for a in hist["assign"]]
    hist["objective"] = [float(o.item()) for o in objs]
    return cent, hist


def build_lists(x_dev: torch.Tensor, nlist: int, niter: int = 10, seed: int = 1234):
    """Train, assign to the final centroids and sort into lists, all on the device:
    (centroids [nlist][d], list_off int64 [nlist + 1], ids int64 [n], codes [n][d] list-major)."""
    x = x_dev.contiguous()
    cent = kmeans(x, nlist, niter=niter, seed=seed)
    assign, _ = ops.kmeans_assign(x, cent)
    list_off, ids, _ = ops.kmeans_lists(assign, nlist)
    return cent, list_off, ids, ops.gather_rows(x, ids)


def _host_index(cent, list_off, ids, codes, nprobe):
    off = list_off.cpu().numpy()
    cut = off[1:-1]
    return IVFFlatIndex(cent.shape[1], cent.cpu().numpy(), np.split(codes.cpu().numpy(), cut),
                        np.split(ids.cpu().numpy(), cut), nprobe=nprobe, ntotal=int(ids.numel()))


def build_index(x_dev: torch.Tensor, nlist: int, nprobe: int = 1, niter: int = 10, seed: int = 1234) -> IVFFlatIndex:
    """``index_factory("IVF{nlist},Flat")`` + ``train(x)`` + ``add(x)``: the host image ``write`` serialises."""
    return _host_index(*build_lists(x_dev, nlist, niter, seed), nprobe)


def build_device(x_dev: torch.Tensor, nlist: int, nprobe: int = 1, niter: int = 10, seed: int = 1234) -> IVFFlatDevice:
    """The same index, searchable at once (``IVFFlatDevice.from_lists``)."""
    cent, list_off, ids, codes = build_lists(x_dev, nlist, niter, seed)
    return IVFFlatDevice.from_lists(cent, list_off, ids, codes, x_dev.contiguous(), nprobe)


def n_ivf_rule(n: int) -> int:
    """create_index.py:66."""
    return min(int(16 * np.sqrt(n)), n // 39)


def index_names(n_ivf: int, model_name: str, version: str, nprobe: int = 1):
    """The reference's two file names (create_index.py:71, :82)."""
    tail = f"_IVF{n_ivf}_Flat_nprobe_{nprobe}_{model_name}_{version}.index"
    return "trained" + tail, "added" + tail


def load_features(exp_dir: str, version: str) -> np.ndarray:
    """create_index.py:51-58: the sorted ``{version}_extracted/*.npy``, concatenated."""
    feature_dir = os.path.join(exp_dir, f"{version}_extracted")
    return np.concatenate([np.load(os.path.join(feature_dir, name)) for name in sorted(os.listdir(feature_dir))], axis=0)


def create_index(exp_dir: str, version: str = "v2", index_algorithm: str = "Auto", rng=None, device="cuda") -> str:
    """create_index.py:51-84: writes ``total_fea.npy`` and the trained / added index pair under ``exp_dir`` and
    returns the added index's path.  ``rng`` (a NumPy Generator or RandomState) shuffles the rows; None uses
    ``np.random.shuffle`` as the reference does."""
    big_npy = load_features(exp_dir, version)
    d = 256 if version == "v1" else 768
    if big_npy.ndim != 2 or big_npy.shape[1] != d:
        raise ValueError(f"create_index: {version} features must be [N][{d}], got {big_npy.shape}")
    if big_npy.shape[0] > MAX_ROWS_FAISS and index_algorithm in ("Auto", "KMeans"):  # before any copy of the rows
        raise NotImplementedError(
            f"create_index: {big_npy.shape[0]} rows > 2e5 under index_algorithm={index_algorithm!r} means the "
            "reference's sklearn MiniBatchKMeans reduction to 10000 rows, which is not on the device path yet; "
            'index_algorithm="Faiss" (the reference\'s own option) indexes every row')
    n_ivf = n_ivf_rule(big_npy.shape[0])
    if n_ivf == 0:  # faiss refuses IVF0 after the reference has written total_fea.npy; here nothing is written
        raise ValueError(f"create_index: {big_npy.shape[0]} rows give n_ivf = 0 (at least 39 rows are needed)")
    idx = np.arange(big_npy.shape[0])
    (np.random if rng is None else rng).shuffle(idx)
    big_npy = big_npy[idx]
    np.save(os.path.join(exp_dir, "total_fea.npy"), big_npy)
    model_name = os.path.basename(os.path.normpath(exp_dir))
    trained_name, added_name = index_names(n_ivf, model_name, version)
    x = torch.from_numpy(np.ascontiguousarray(big_npy, dtype=np.float32)).to(device)
    cent, list_off, ids, codes = build_lists(x, n_ivf)
    c = cent.cpu().numpy()
    none_c, none_i = np.zeros((0, d), np.float32), np.zeros(0, np.int64)
    IVFFlatIndex(d, c, [none_c] * n_ivf, [none_i] * n_ivf, nprobe=1, ntotal=0).write(os.path.join(exp_dir, trained_name))
    added = os.path.join(exp_dir, added_name)
    _host_index(cent, list_off, ids, codes, 1).write(added)
    return added
