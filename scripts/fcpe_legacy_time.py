"""Device time of VC.f0_device for "fcpe-legacy" (rvc_amd.fcpe_legacy, csrc/performer.hip) beside "fcpe" on the same
30 s clip at 16 kHz and the same commit, synthetic weights: device events around each call after warm-up, median
and spread; then the attention kernels' share, timed as the model's own 12 rvc_performer_attention calls alone.

    python scripts/fcpe_legacy_time.py [--reps 20] [--seconds 30] [--out profiles/fcpe_legacy_time.txt] [--once]

``--once`` runs the fcpe-legacy call a few times and exits: the form to put behind a kernel-trace profiler.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
import numpy as np
import torch

from rvc_amd import synthetic
from rvc_amd.fcpe import PRECISION, FcpeAMD
from rvc_amd.fcpe_legacy import FcpeLegacyAMD
from rvc_amd.pipeline import VC, Config

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--out", default=None)
ap.add_argument("--once", action="store_true")
args = ap.parse_args()

dev = "cuda"
x = torch.from_numpy(synthetic.synthetic_audio(args.seconds, seed=4)).to(dev)
fl = FcpeLegacyAMD(synthetic.fcpe_legacy_checkpoint(n_layers=12), dev)
vc = VC(40000, Config(dev), fcpe_legacy=fl, fcpe=None if args.once else FcpeAMD(synthetic.fcpe_checkpoint(), dev))


def device_ms(fn, reps, warm=3):
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
    return np.asarray(ts)


def spread(name, ts):
    return (f"{name}: median {np.median(ts):.3f} ms, min {ts.min():.3f}, max {ts.max():.3f}, "
            f"p10-p90 {np.percentile(ts, 10):.3f}-{np.percentile(ts, 90):.3f} over {len(ts)} calls")


if args.once:
    for _ in range(3):
        vc.f0_device(x, 0, "fcpe-legacy")
    torch.cuda.synchronize()
    sys.exit(0)

T = x.numel() // 160 + 1
M = fl.layers[0]["proj"].shape[0]
lines = [f"clip: {args.seconds:g} s = {x.numel()} samples, {T} frames; {fl.n_layers} layers, {fl.C} channels, "
         f"8 heads of 64, {M} random features; dense convs at precision {PRECISION!r}"]
for method in ("fcpe-legacy", "fcpe"):
    ts = device_ms(lambda: vc.f0_device(x, 0, method), args.reps)
    lines.append(spread(f"f0_device({method!r})", ts))
    if method == "fcpe-legacy":
        whole = float(np.median(ts))
qkv = torch.randn(3 * 512, T, device=dev)
att = torch.empty(512, T, device=dev)


def attention_only():
    for L in fl.layers:
        fl.performer(qkv, L["proj"], att)


ts = device_ms(attention_only, args.reps)
lines.append(spread(f"the {fl.n_layers} rvc_performer_attention calls alone (key pass, reduction, query pass each)",
                    ts))
flop = fl.n_layers * 8 * (2 * 2 * T * M * 64 * 2)
lines.append(f"attention share of the fcpe-legacy call: {100 * np.median(ts) / whole:.1f} %; "
             f"{flop / 1e9:.2f} GFLOP of f32 MFMA in them = {flop / np.median(ts) / 1e9:.2f} TFLOP/s")
vc.check_errors()
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
