"""Device time of VC.f0_device for "fcpe" (rvc_amd.fcpe, csrc/fcpe.hip) beside "rmvpe" on the same 30 s clip at
16 kHz and the same commit, synthetic weights: device events around each call after warm-up, median and spread.

    python scripts/fcpe_time.py [--reps 20] [--seconds 30] [--out profiles/fcpe_time.txt] [--once]

``--once`` runs the fcpe call a few times and exits: the form to put behind a kernel-trace profiler.
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
from rvc_amd.pipeline import VC, Config
from rvc_amd.rmvpe import RMVPEAMD

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--out", default=None)
ap.add_argument("--once", action="store_true")
args = ap.parse_args()

dev = "cuda"
x = torch.from_numpy(synthetic.synthetic_audio(args.seconds, seed=4)).to(dev)
fc = FcpeAMD(synthetic.fcpe_checkpoint(), dev)
vc = VC(40000, Config(dev), fcpe=fc,
        rmvpe=None if args.once else RMVPEAMD(synthetic.rmvpe_state_dict(777), dev))


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


if args.once:
    for _ in range(3):
        vc.f0_device(x, 0, "fcpe")
    torch.cuda.synchronize()
    sys.exit(0)

T = x.numel() // 160 + 1
H = 2 * fc.C
lines = [f"clip: {args.seconds:g} s = {x.numel()} samples, {T} frames; {fc.n_layers} layers, {fc.C} channels; "
         f"dense convs at precision {PRECISION!r}"]
for method in ("fcpe", "rmvpe"):
    ts = device_ms(lambda: vc.f0_device(x, 0, method), args.reps)
    lines.append(f"f0_device({method!r}): median {np.median(ts):.3f} ms, min {ts.min():.3f}, max {ts.max():.3f}, "
                 f"p10-p90 {np.percentile(ts, 10):.3f}-{np.percentile(ts, 90):.3f} over {args.reps} calls")
lines.append(f"rvc_glu_dwconv_silu moves {12 * H * T / 1e6:.1f} MB per layer ({8 * H * T / 1e6:.1f} read + "
             f"{4 * H * T / 1e6:.1f} written)")
vc.check_errors()
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
