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

Above 2e5 rows the reference first reduces the rows to 10000 centres (create_index.py:63-76, under "Auto" and
"KMeans") with ``sklearn.cluster.MiniBatchKMeans(n_clusters=10000, batch_size=256 * cpu_count(),
compute_labels=False, init="random")``, saves those as ``total_fea.npy`` and indexes them.  ``minibatch_kmeans`` is
that call (sklearn 1.7.2, dense rows, unit weights) with sklearn's control flow draw for draw:

  sizes and draws     ``bs = min(batch_size, n)``; ``init_size = 3 bs``, or ``3 k`` if that is below k, at most n;
                      ``(100 n) // bs`` steps at most; one ``RandomState``: the validation rows, per init the
                      candidate rows (only if ``init_size < n``) and ``choice(m, k, replace=False, p=ones / m)``; the
                      init with the lowest inertia on the validation rows wins (strict <)
  each step           ``randint(0, n, bs)`` rows; labels and inertia against the centres before the step; per centre
                      with members ``row = centre * weight`` (an f32 product rounded on its own), ``+=`` the members
                      in batch order, ``weight += members``, ``row *= 1.f / weight``
  reassignment        when a weight is 0 or ``10 k`` rows have passed: centres with ``weight < 0.01f max`` (at most
                      half a batch, the others by ``np.argsort`` of the weights) take batch rows drawn with
                      ``choice(bs, replace=False)``, and their weights the minimum of the kept ones
  stopping            the batch inertia per row, exponentially weighted (``alpha = 2 bs / (n + 1)``) from step 1 on;
                      10 steps without a new minimum end the run

Assign, lists, update, inertia and the row scatter are kernels (``ops.minibatch_*``, csrc/minibatch.hip); the host
reads a 32-byte status block once per step and the k weights on steps that reassign.  sklearn is installed where the
fixtures are recorded: tests/golden/minibatch_*.npz hold sklearn's own centres, which the restatement
tests/minibatch_ref.py reproduces bit for bit and the device is compared with.
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


def _random_state(random_state):
    """sklearn's ``check_random_state``: None is NumPy's global RandomState (``np.random.seed`` reproduces a run)."""
    if random_state is None or random_state is np.random:
        return np.random.mtrand._rand
    if isinstance(random_state, (int, np.integer)):
        return np.random.RandomState(int(random_state))
    if isinstance(random_state, np.random.RandomState):
        return random_state
    raise TypeError(f"minibatch_kmeans: random_state must be None, an int or a numpy RandomState, "
                    f"not {type(random_state).__name__}")


def minibatch_sizes(n: int, k: int, batch_size: int, max_iter: int = 100):
    """``MiniBatchKMeans._check_params_vs_input`` with ``init_size=None``: (batch, init_size, n_steps)."""
    bs = min(int(batch_size), n)
    init_size = 3 * bs
    if init_size < k:
        init_size = 3 * k
    return bs, min(init_size, n), (max_iter * n) // bs


class MiniBatchTrainer:
    """The device state of one MiniBatchKMeans run -- rows ``x`` [n][d], centres [k][d] (two buffers that swap),
    ``weights`` f32 [k] (sklearn's ``_counts``) -- and ``step``, sklearn's ``_mini_batch_step``."""

    def __init__(self, x, cent, weights=None, reassignment_ratio=0.01):
        self.x = x
        self.k = cent.shape[0]
        self.cent = cent.contiguous().clone()
        self.other = torch.empty_like(self.cent)
        self.weights = torch.zeros(self.k, dtype=torch.float32, device=x.device) if weights is None else \
            torch.as_tensor(weights, dtype=torch.float32).to(x.device).contiguous().clone()
        self.ratio = float(reassignment_ratio)
        self.status = torch.zeros(ops.MINIBATCH_STATUS.itemsize, dtype=torch.uint8, device=x.device)
        self.any_zero = None  # of the weights after the last step; None: not known on the host

    def step(self, batch, rs, reassign, labels=None):
        """One step on the rows ``batch`` (host int array).  ``labels`` (host) overrides the device's assignment.
        Returns a dict: ``inertia`` (f64, against the centres before the step), ``labels`` (device int32), ``to``
        (the reassigned centres) and ``picked`` (the batch rows they took).  One host read (the status block), and
        the k weights as well on a step that reassigns."""
        dev = self.x.device
        xb = ops.gather_rows(self.x, torch.from_numpy(np.ascontiguousarray(batch, dtype=np.int64)).to(dev))
        bs = xb.shape[0]
        if labels is None:
            labels, _ = ops.minibatch_assign(xb, self.cent)
        else:
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
        list_off, ids, _ = ops.kmeans_lists(labels, self.k)
        new = ops.minibatch_update(xb, list_off, ids, self.cent, self.weights, out=self.other)
        ops.minibatch_inertia(xb, self.cent, labels, self.weights, status=self.status)
        to = picked = np.zeros(0, np.int64)
        if reassign and self.ratio > 0:
            w = self.weights.cpu().numpy()
            mask = w < np.float32(self.ratio) * w.max()
            if mask.sum() > 0.5 * bs:
                mask[np.argsort(w)[int(0.5 * bs):]] = False
            n_reassigns = int(mask.sum())
            if n_reassigns:
                picked = np.asarray(rs.choice(bs, replace=False, size=n_reassigns), dtype=np.int64)
                to = np.nonzero(mask)[0].astype(np.int64)
                floor = w[~mask].min()
                ops.minibatch_scatter(xb, torch.from_numpy(picked).to(dev), torch.from_numpy(to).to(dev), floor, new,
                                      self.weights)
                w[mask] = floor
            inertia, _, _ = ops.minibatch_status(self.status)
            self.any_zero = bool((w == 0).any())
        else:
            inertia, _, self.any_zero = ops.minibatch_status(self.status)
        self.cent, self.other = new, self.cent
        return {"inertia": inertia, "labels": labels, "to": to, "picked": picked}

    def inertia(self, rows):
        """The f64 inertia of the rows ``rows`` (host int array) against the current centres (one host read)."""
        xv = ops.gather_rows(self.x, torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.x.device))
        labels, _ = ops.minibatch_assign(xv, self.cent)
        return ops.minibatch_status(ops.minibatch_inertia(xv, self.cent, labels, status=self.status))[0]


def minibatch_kmeans(x_dev: torch.Tensor, n_clusters: int = 10000, batch_size=None, random_state=None, *,
                     max_iter: int = 100, max_no_improvement: int = 10, reassignment_ratio: float = 0.01,
                     n_init: int = 3, history: bool = False):
    """``sklearn.cluster.MiniBatchKMeans(n_clusters, batch_size=batch_size, compute_labels=False, init="random",
    random_state=random_state).fit(x).cluster_centers_`` (sklearn 1.7.2) on device rows ``x_dev`` [n][d] f32 ->
    centres [k][d] on the device.

    The host keeps the loop, the ``RandomState`` (every draw sklearn makes, in its order) and the reassignment
    decision; the rows, centres and weights stay on the device.  Each step reads the 32-byte status block, and the k
    weights on steps that reassign.  The assignment is the device's exact-f32 one, so a trajectory equals sklearn's
    as long as no decision falls inside the f32 tolerance (tests/minibatch_ref.py); past such a tie both are valid
    runs of the same algorithm.

    ``random_state``: None is NumPy's global ``RandomState`` (what ``check_random_state(None)`` returns, so
    ``np.random.seed(s)`` reproduces a run as in the reference); an int seeds a new one; a ``RandomState`` is used.
    ``batch_size=None`` is ``256 * multiprocessing.cpu_count()`` as create_index.py:68 passes it: the default
    depends on the host, exactly as in the reference -- pass a number for a result that does not.

    ``history=True`` returns ``(centres, hist)``: per step ``hist["batch"]``, ``["labels"]``, ``["inertia"]``,
    ``["counts"]`` (the weights after the step, an extra read per step), ``["reassigned"]`` ((centres, batch rows)
    pairs), and ``hist["n_steps"]``."""
    if x_dev.dim() != 2 or x_dev.dtype != torch.float32 or not x_dev.is_cuda:
        raise TypeError("minibatch_kmeans: a CUDA f32 [n][d] tensor")
    x = x_dev.contiguous()
    n, d = x.shape
    k = int(n_clusters)
    if k < 1 or n < k:
        raise ValueError(f"minibatch_kmeans: {n} rows cannot train {k} centres")
    if batch_size is None:
        import multiprocessing
        batch_size = 256 * multiprocessing.cpu_count()
    if int(batch_size) < 1 or n_init < 1:
        raise ValueError("minibatch_kmeans: batch_size and n_init must be at least 1")
    rs = _random_state(random_state)
    bs, init_size, n_steps = minibatch_sizes(n, k, batch_size, max_iter)
    valid = rs.randint(0, n, init_size)
    best, state = None, None
    for _ in range(n_init):
        cand = rs.randint(0, n, init_size) if init_size < n else None
        m = n if cand is None else init_size
        w = np.ones(m, np.float32)
        seeds = rs.choice(m, size=k, replace=False, p=w / w.sum())
        rows = seeds if cand is None else cand[seeds]
        trial = MiniBatchTrainer(x, ops.gather_rows(x, torch.from_numpy(np.asarray(rows, np.int64)).to(x.device)),
                                 reassignment_ratio=reassignment_ratio)
        inertia = trial.inertia(valid)
        if best is None or inertia < best:
            best, state = inertia, trial
    hist = {"batch": [], "labels": [], "inertia": [], "counts": [], "reassigned": [], "n_steps": 0}
    ewa = ewa_min = None
    no_improvement = since = 0
    any_zero = True  # the weights start at 0
    alpha = min(bs * 2.0 / (n + 1), 1)
    for i in range(n_steps):
        batch = rs.randint(0, n, bs)
        since += bs
        reassign = any_zero or since >= 10 * k
        if reassign:
            since = 0
        out = state.step(batch, rs, reassign)
        any_zero = state.any_zero
        hist["n_steps"] = i + 1
        if history:
            hist["batch"].append(batch)
            hist["labels"].append(out["labels"].cpu().numpy())
            hist["inertia"].append(out["inertia"])
            hist["counts"].append(state.weights.cpu().numpy())
            hist["reassigned"].append((out["to"], out["picked"]))
        if i == 0:
            continue
        b = out["inertia"] / bs
        ewa = b if ewa is None else ewa * (1 - alpha) + b * alpha
        if ewa_min is None or ewa < ewa_min:
            no_improvement, ewa_min = 0, ewa
        else:
            no_improvement += 1
        if max_no_improvement is not None and no_improvement >= max_no_improvement:
            break
    return (state.cent, hist) if history else state.cent


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


def create_index(exp_dir: str, version: str = "v2", index_algorithm: str = "Auto", rng=None, device="cuda", *,
                 reduce_rows=MAX_ROWS_FAISS, reduce_to: int = 10000, batch_size=None) -> str:
    """create_index.py:51-84: writes ``total_fea.npy`` and the trained / added index pair under ``exp_dir`` and
    returns the added index's path.  ``rng`` (a NumPy Generator or RandomState) shuffles the rows; None uses
    ``np.random.shuffle`` as the reference does.

    More than ``reduce_rows`` rows under "Auto" / "KMeans" are first reduced to ``reduce_to`` centres by
    ``minibatch_kmeans`` (create_index.py:63-76; ``batch_size`` as there): the centres become ``total_fea.npy`` and
    the rows of the index.  On that path ``rng`` also drives the reduction, as the reference's one global
    ``RandomState`` does, so it must be None or a ``RandomState``."""
    big_npy = load_features(exp_dir, version)
    d = 256 if version == "v1" else 768
    if big_npy.ndim != 2 or big_npy.shape[1] != d:
        raise ValueError(f"create_index: {version} features must be [N][{d}], got {big_npy.shape}")
    reduce = big_npy.shape[0] > reduce_rows and index_algorithm in ("Auto", "KMeans")
    if reduce:  # before any copy of the rows
        if torch.device(device).type != "cuda":
            raise NotImplementedError(
                f"create_index: {big_npy.shape[0]} rows > {reduce_rows:g} under index_algorithm={index_algorithm!r} "
                f"means the reference's sklearn MiniBatchKMeans reduction to {reduce_to} rows, which runs on the "
                f'device only (device={str(device)!r} is not one); index_algorithm="Faiss" (the reference\'s own '
                "option) indexes every row")
        if rng is not None and not isinstance(rng, np.random.RandomState):
            raise TypeError("create_index: the MiniBatchKMeans reduction draws from a numpy RandomState, as sklearn "
                            f"does: rng must be None or a RandomState on this path, not {type(rng).__name__}")
        if not 39 <= reduce_to <= big_npy.shape[0]:
            raise ValueError(f"create_index: reduce_to={reduce_to} must lie in [39, {big_npy.shape[0]}]")
    n_ivf = n_ivf_rule(reduce_to if reduce else big_npy.shape[0])
    if n_ivf == 0:  # faiss refuses IVF0 after the reference has written total_fea.npy; here nothing is written
        raise ValueError(f"create_index: {big_npy.shape[0]} rows give n_ivf = 0 (at least 39 rows are needed)")
    idx = np.arange(big_npy.shape[0])
    (np.random if rng is None else rng).shuffle(idx)
    big_npy = big_npy[idx]
    if reduce:
        x = minibatch_kmeans(torch.from_numpy(np.ascontiguousarray(big_npy, dtype=np.float32)).to(device), reduce_to,
                             batch_size, rng)
        big_npy = x.cpu().numpy()
    else:
        x = torch.from_numpy(np.ascontiguousarray(big_npy, dtype=np.float32)).to(device)
    np.save(os.path.join(exp_dir, "total_fea.npy"), big_npy)
    model_name = os.path.basename(os.path.normpath(exp_dir))
    trained_name, added_name = index_names(n_ivf, model_name, version)
    cent, list_off, ids, codes = build_lists(x, n_ivf)
    c = cent.cpu().numpy()
    none_c, none_i = np.zeros((0, d), np.float32), np.zeros(0, np.int64)
    IVFFlatIndex(d, c, [none_c] * n_ivf, [none_i] * n_ivf, nprobe=1, ntotal=0).write(os.path.join(exp_dir, trained_name))
    added = os.path.join(exp_dir, added_name)
    _host_index(cent, list_off, ids, codes, 1).write(added)
    return added
