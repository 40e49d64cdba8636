"""Device time of formant shifting (rvc_amd.formant, csrc/formant.hip) on one 30 s clip at 16 kHz (device
events around the call after warm-up) beside the host time of the numpy restatement (tests/formant_ref.py)
on the same clip, and their agreement.

    python scripts/formant_time.py [--reps 20] [--seconds 30] [--out profiles/formant_time.txt] [--once]

``--once`` runs the shifter a few times and exits: the form to put behind a kernel-trace profiler.
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import formant_ref
from rvc_amd import _lib, synthetic
from rvc_amd.formant import FormantShiftAMD

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--qfrency", type=float, default=0.8)
ap.add_argument("--timbre", type=float, default=0.8)
ap.add_argument("--out", default=None)
ap.add_argument("--once", action="store_true")
args = ap.parse_args()

dev = "cuda"
x = synthetic.synthetic_audio(args.seconds, seed=4).astype(np.float32)
xd = torch.from_numpy(x).to(dev)
sh = FormantShiftAMD(16000, 1024, 32, dev)
q, d = args.qfrency * 1e-3, args.timbre


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
    return float(np.median(ts)), float(np.min(ts))


if args.once:
    for _ in range(3):
        sh(xd, q, d)
    torch.cuda.synchronize()
    sys.exit(0)

M = (len(x) - 1024) // 32 + 1
work = _lib.load().rvc_formant_work_bytes(len(x), sh._args(q, d))
lines = [f"clip: {args.seconds:g} s = {len(x)} samples, {M} frames, work {work / 1e6:.1f} MB; "
         f"formant_qfrency {args.qfrency}, formant_timbre {args.timbre}"]
med, lo = device_ms(lambda: sh(xd, q, d), args.reps)
lines.append(f"device formant shift (5 launches, work allocation included): median {med:.3f} ms, min {lo:.3f} ms "
             f"over {args.reps} calls")
t0 = time.perf_counter()
out = sh.shiftpitch(x, quefrency=q, distortion=d)
lines.append(f"device shiftpitch from / to host numpy: {(time.perf_counter() - t0) * 1e3:.1f} ms")
t0 = time.perf_counter()
ref = formant_ref.shiftpitch(x, q, d)
lines.append(f"numpy restatement on the host: {time.perf_counter() - t0:.2f} s")
lines.append(f"max |device - restatement| / spacing(f32 max |ref|): "
             f"{np.abs(out - ref).max() / np.spacing(np.float32(np.abs(ref).max())):.3f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
