"""Time of the MiniBatchKMeans reduction of create_index (csrc/minibatch.hip, rvc_amd/index_train.minibatch_kmeans)
at the reference's shape: n = 250 000 synthetic rows, d = 768, 10000 centres, batch_size = 4096, one seed.

    python scripts/minibatch_time.py [--n 250000] [--d 768] [--k 10000] [--batch 4096] [--seed 0] [--reps 7]
                                     [--out profiles/minibatch_time.txt]
    python scripts/minibatch_time.py --sklearn [--n ...]      # the comparison: sklearn itself on the CPUs, no GPU

The device run reports the wall time of the whole call (host clock, synchronised), its steps and time per step, and
the device time of each call of a step at the batch's shape (device events after warm-up, medians over --reps).  The
rows come from one NumPy RandomState, so both modes see the same matrix; --out appends the mode's lines to the file.
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=250_000)
ap.add_argument("--d", type=int, default=768)
ap.add_argument("--k", type=int, default=10_000)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sklearn", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
n, d, k = args.n, args.d, args.k


def rows():
    """f32 rows of 2000 Gaussian clusters (centres 4 N(0, 1), unit noise), the same in both modes."""
    rs = np.random.RandomState(12345)
    centres = (4.0 * rs.standard_normal((2000, d))).astype(np.float32)
    x = centres[rs.randint(0, 2000, n)]
    for i in range(0, n, 50_000):
        x[i:i + 50_000] += rs.standard_normal((min(50_000, n - i), d)).astype(np.float32)
    return np.ascontiguousarray(x)


def full_inertia(x, cent):
    """Mean squared distance of a 20000-row sample to its nearest centre (f64 on the host)."""
    s = np.asarray(x[:: max(1, n // 20_000)], np.float64)
    c = np.asarray(cent, np.float64)
    d2 = (s * s).sum(1)[:, None] - 2.0 * (s @ c.T) + (c * c).sum(1)[None, :]
    return float(np.maximum(d2, 0).min(1).mean())


x = rows()
head = f"n = {n}, d = {d}, k = {k}, batch_size = {args.batch}, seed {args.seed}"
if args.sklearn:
    import sklearn
    from sklearn.cluster import MiniBatchKMeans
    from threadpoolctl import threadpool_info
    threads = sorted({(p["user_api"], p["num_threads"]) for p in threadpool_info()})
    t0 = time.perf_counter()
    m = MiniBatchKMeans(n_clusters=k, batch_size=args.batch, compute_labels=False, init="random",
                        random_state=args.seed).fit(x)
    wall = time.perf_counter() - t0
    lines = [f"sklearn {sklearn.__version__} MiniBatchKMeans on the CPUs ({os.cpu_count()} CPUs; thread pools {threads}): "
             f"{head}",
             f"fit: {wall:.1f} s wall, {m.n_steps_} steps -> {1e3 * wall / m.n_steps_:.1f} ms per step (the three inits "
             f"included); mean squared distance of a row sample to its centre {full_inertia(x, m.cluster_centers_):.3f}"]
else:
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
    import torch

    from rvc_amd import index_train, ops

    dev = "cuda"
    xd = torch.from_numpy(x).to(dev)
    index_train.minibatch_kmeans(xd, k, args.batch, args.seed, max_iter=1, max_no_improvement=1)  # warm-up
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cent = index_train.minibatch_kmeans(xd, k, args.batch, args.seed)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    wall = float(np.median(walls))
    _, hist = index_train.minibatch_kmeans(xd, k, args.batch, args.seed, history=True)
    steps = hist["n_steps"]
    moved = sum(len(t) for t, _ in hist["reassigned"])
    lines = [f"device: {head}",
             f"minibatch_kmeans: {wall:.3f} s wall, median of {args.reps} whole calls ({min(walls):.3f} .. {max(walls):.3f}; "
             f"host clock, synchronised), {steps} steps -> {1e3 * wall / steps:.2f} ms per step (the three inits "
             f"included); {sum(len(t) > 0 for t, _ in hist['reassigned'])} steps reassigned {moved} centres; mean "
             f"squared distance of a row sample to its centre {full_inertia(x, cent.cpu().numpy()):.3f}"]

    def device_ms(fn, reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    bs = min(args.batch, n)
    batch = torch.from_numpy(np.random.RandomState(1).randint(0, n, bs).astype(np.int64)).to(dev)
    w = torch.from_numpy(hist["counts"][-1]).to(dev)
    xb = ops.gather_rows(xd, batch)
    labels, dist = ops.minibatch_assign(xb, cent)
    list_off, ids, _ = ops.kmeans_lists(labels, k)
    other = torch.empty_like(cent)
    status = torch.zeros(32, dtype=torch.uint8, device=dev)
    src = torch.arange(64, device=dev)
    dst = torch.arange(64, device=dev) * 3
    flop = 2.0 * bs * d * k
    lines.append(f"one step at batch {bs}, medians of {args.reps} calls (min .. max), device events:")
    for name, fn, note in [
            ("rvc_gather_rows (the batch)", lambda: ops.gather_rows(xd, batch), ""),
            ("rvc_minibatch_assign (prep + assign + finalize)", lambda: ops.minibatch_assign(xb, cent, labels, dist),
             f"; {flop / 1e9:.1f} GFLOP of inner products"),
            ("rvc_kmeans_lists", lambda: ops.kmeans_lists(labels, k), ""),
            ("rvc_minibatch_update (update + weights)", lambda: ops.minibatch_update(xb, list_off, ids, cent, w.clone(), other),
             "; with the clone of the k weights"),
            ("rvc_minibatch_inertia (rows + status)", lambda: ops.minibatch_inertia(xb, cent, labels, w, status), ""),
            ("rvc_minibatch_scatter (64 centres)", lambda: ops.minibatch_scatter(xb, src, dst, 1.0, other, w.clone()),
             "; with the clone of the k weights")]:
        med, lo, hi = device_ms(fn, args.reps)
        extra = f" -> {flop / med / 1e9:.1f} TFLOP/s" if "assign" in name else ""
        lines.append(f"  {name}: {med:.3f} ms ({lo:.3f} .. {hi:.3f}){note}{extra}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
