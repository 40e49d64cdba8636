"""Device time of VC.f0_device on one padded 30 s clip for the swipe, pm, rmvpe and hybrid[rmvpe+swipe] f0
methods (device events around the call after warm-up), the swipe path's launch count, and the per-stage
times of swipe_strength / swipe_pick / swipe_post (device events around each).

    python scripts/swipe_time.py [--reps 50] [--out profiles/swipe_time.txt] [--once swipe]

``--once METHOD`` runs the method a few times and exits: the form to put behind a kernel-trace profiler.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rvc-maker_amd"))
import numpy as np
import torch

from rvc_amd import synthetic
from rvc_amd.pipeline import VC, Config
from rvc_amd.rmvpe import RMVPEAMD

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None)
ap.add_argument("--once", default=None)
args = ap.parse_args()

dev = "cuda"
vc = VC(48000, Config(dev), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(2), dev))
audio = torch.from_numpy(synthetic.synthetic_audio(30.0, seed=4)).float().to(dev)
xp, xp64 = vc.filt(audio, vc.t_pad, want_f64=True)
lines = [f"clip: 30 s + 2 x {vc.t_pad} padding = {xp.numel()} samples, {xp.numel() // 160 + 1} swipe frames"]


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
        vc.f0_device(xp, 0, args.once, xp64=xp64)
    torch.cuda.synchronize()
    vc.check_errors()
    sys.exit(0)

for method in ("swipe", "pm", "rmvpe", "hybrid[rmvpe+swipe]"):
    med, lo = device_ms(lambda: vc.f0_device(xp, 0, method, xp64=xp64), args.reps)
    lines.append(f"f0_device({method!r}): median {med:.3f} ms, min {lo:.3f} ms over {args.reps} calls")
vc.check_errors()

sw = vc._swipe(dev)
S = sw.strength(xp)
f0 = sw.pick(S)
for name, fn in (("swipe_strength (fft, 2 GEMMs, sum: 4 launches)", lambda: sw.strength(xp)),
                 ("swipe_pick (1 launch)", lambda: sw.pick(S)),
                 ("swipe f0_device (strength + pick + post: 6 launches)", lambda: sw.f0_device(xp, 0.0))):
    med, lo = device_ms(fn, args.reps)
    lines.append(f"{name}: median {med:.3f} ms, min {lo:.3f} ms")
# the GEMM stages' floors: flop / 78.6 TFLOP/s (f64 matrix peak) and bytes / 8 TB/s
n = xp.numel()
flop_b = flop_c = bytes_b = bytes_c = 0
for i, nc in enumerate((127, 192, 192, 192, 110)):
    nfr, nbin = n // (1024 >> i) + 2, (1024 >> i) + 1
    flop_b += 2 * 328 * nbin * nfr
    flop_c += 2 * nc * 328 * nfr
    bytes_b += 8 * (nfr * nbin + 328 * nbin + nfr * 336)
    bytes_c += 8 * (nfr * 336 + nc * 336 + nc * nfr)
for tag, fl, by in (("loudness GEMM (b)", flop_b, bytes_b), ("strength GEMM (c)", flop_c, bytes_c)):
    lines.append(f"{tag}: {fl / 1e9:.2f} GFLOP -> {fl / 78.6e12 * 1e6:.1f} us at 78.6 TFLOP/s; "
                 f"{by / 1e6:.1f} MB -> {by / 8e12 * 1e6:.1f} us at 8 TB/s")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
