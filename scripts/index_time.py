"""Device time of the IVF training steps (csrc/kmeans.hip, rvc_amd/index_train.py) at the upper end of
create_index.py's range: N = 200 000 rows, d = 768, n_ivf = 5128.  Device events around each call after warm-up,
medians over --reps calls; the whole create_index by a host clock around the call (it ends in host copies and file
writes); and the host path it replaces, IVFFlatIndex.build's f64 assignment, on the same centroids.

    python scripts/index_time.py [--n 200000] [--d 768] [--reps 7] [--host-rows 20000] [--out profiles/index_time.txt]

The host assignment builds a dense f64 [rows][k] matrix (8.2 GB at the full size, several times that with its
temporaries), so it is timed on the first --host-rows rows and scaled by N / rows: its cost is linear in the rows.
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
import numpy as np
import torch

from rvc_amd import index_train, ops
from rvc_amd.faiss_index import IVFFlatIndex

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200_000)
ap.add_argument("--d", type=int, default=768)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-rows", type=int, default=20_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

PEAK_F32_MFMA = 157.3e12  # MI355X f32-input MFMA peak, FLOP/s
dev = "cuda"
n, d = args.n, args.d
k = index_train.n_ivf_rule(n)
g = torch.Generator(device=dev).manual_seed(0)
centres = torch.randn(k, d, device=dev, generator=g)
x = (centres[torch.randint(0, k, (n,), device=dev, generator=g)]
     + 0.3 * torch.randn(n, d, device=dev, generator=g)).contiguous()
del centres


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


lines = [f"N = {n}, d = {d}, n_ivf = {k}; medians of {args.reps} calls (min .. max), device events"]
cent = ops.gather_rows(x, torch.from_numpy(index_train.rand_perm(n, 1235)[:k].copy()).to(dev))
assign = torch.empty(n, dtype=torch.int32, device=dev)
dist = torch.empty(n, device=dev)
med, lo, hi = device_ms(lambda: ops.kmeans_assign(x, cent, assign, dist), args.reps)
flop = 2.0 * n * d * k
lines.append(f"rvc_kmeans_assign (prep + assign + finalize): {med:.2f} ms ({lo:.2f} .. {hi:.2f}); {flop / 1e12:.3f} TFLOP "
             f"of inner products -> {flop / med / 1e9:.1f} TFLOP/s = {100 * flop / (med * 1e-3) / PEAK_F32_MFMA:.1f} % of the "
             f"157.3 TF f32-MFMA peak (compute bound: {flop / PEAK_F32_MFMA * 1e3:.1f} ms at peak)")
med, lo, hi = device_ms(lambda: ops.kmeans_lists(assign, k), args.reps)
lines.append(f"rvc_kmeans_lists: {med:.3f} ms ({lo:.3f} .. {hi:.3f})")
list_off, ids, counts = ops.kmeans_lists(assign, k)
new = torch.empty_like(cent)
med, lo, hi = device_ms(lambda: ops.kmeans_update(x, list_off, ids, cent, new), args.reps)
lines.append(f"rvc_kmeans_update: {med:.3f} ms ({lo:.3f} .. {hi:.3f}); largest list {int(counts.max())} rows; reads "
             f"{n * d * 4 / 1e6:.0f} MB -> {n * d * 4 / med / 1e6:.0f} GB/s")
med, lo, hi = device_ms(lambda: ops.gather_rows(x, ids), args.reps)
lines.append(f"rvc_gather_rows (list-major codes): {med:.3f} ms ({lo:.3f} .. {hi:.3f})")
torch.cuda.synchronize()
t0 = time.perf_counter()
trained = index_train.kmeans(x, k)
torch.cuda.synchronize()
lines.append(f"kmeans (10 iterations, permutation and splits on the host): {time.perf_counter() - t0:.3f} s wall")

with tempfile.TemporaryDirectory() as tmp:
    exp = os.path.join(tmp, "voice")
    os.makedirs(os.path.join(exp, "v2_extracted" if d == 768 else "v1_extracted"))
    xh = x.cpu().numpy()
    for i in range(4):
        np.save(os.path.join(exp, "v2_extracted" if d == 768 else "v1_extracted", f"clip{i}.npy"),
                xh[i * (n // 4): (i + 1) * (n // 4) if i < 3 else n])
    t0 = time.perf_counter()
    added = index_train.create_index(exp, "v2" if d == 768 else "v1", "Faiss", rng=np.random.default_rng(0), device=dev)
    wall = time.perf_counter() - t0
    lines.append(f"create_index, whole (load 4 files, shuffle, total_fea.npy, train, add, two index files; "
                 f"{os.path.getsize(added) / 1e6:.0f} MB added index): {wall:.2f} s wall")

rows = min(args.host_rows, n)
c = trained.cpu().numpy()
t0 = time.perf_counter()
IVFFlatIndex.build(c, xh[:rows])
host = time.perf_counter() - t0
lines.append(f"host path replaced, IVFFlatIndex.build (f64 assign, one pass, {torch.get_num_threads()} threads): "
             f"{host:.2f} s on {rows} rows -> {host * n / rows:.1f} s scaled to {n} rows (linear in the rows)")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
