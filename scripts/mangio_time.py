"""Device time of VC.f0_device for "mangio-crepe-{tiny,full}" at hop lengths 64, 128 and 160 beside "crepe-{tiny,full}"
on the same 30 s clip at 16 kHz, in one process, synthetic weights: device events around each call after warm-up, five
repeats each, every repeat listed.  At hop 160 mangio runs the frames crepe-<capacity> runs and skips its smoothing;
the stage split (input scale / network / decode + resample / post) says where any difference comes from.

    python scripts/mangio_time.py [--reps 5] [--seconds 30] [--out profiles/mangio_crepe_time.txt]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
import numpy as np
import torch

from rvc_amd import f0mix, ops, synthetic
from rvc_amd.crepe import CrepeAMD
from rvc_amd.pipeline import VC, Config

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = "cuda"
HOPS = (64, 128, 160)
CAPS = ("tiny", "full")
x = torch.from_numpy(synthetic.synthetic_audio(args.seconds, seed=4)).to(dev)
models = {c: CrepeAMD(synthetic.crepe_state_dict(1241, c), c, dev) for c in CAPS}
vc = VC(40000, Config(dev), crepe=models)
p_len = x.numel() // 160


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
    return np.asarray(ts)


def row(name, ts):
    return (f"{name:<34} median {np.median(ts):8.3f} ms  spread {ts.max() - ts.min():6.3f}  "
            f"[{', '.join(f'{t:.3f}' for t in ts)}]")


def stages(cap, hop):
    """mangio's stages on their own (each after the one before it has run): median ms."""
    m = models[cap]
    xn = f0mix.normalize(x)
    T = 1 + x.numel() // hop
    probs = m._all_probabilities(xn, T, hop)
    f0 = m.decode_mangio(probs.clone(), hop, p_len)
    out = {"scale": device_ms(lambda: f0mix.normalize(x), args.reps),
           "network": device_ms(lambda: m._all_probabilities(xn, T, hop), args.reps),
           "decode+resample": device_ms(lambda: m.decode_mangio(probs, hop, p_len), args.reps),
           "post": device_ms(lambda: ops.f0_post64(f0, p_len, 0.0), args.reps)}
    return "  " + ", ".join(f"{k} {np.median(v):.3f}" for k, v in out.items())


lines = [f"clip: {args.seconds:g} s = {x.numel()} samples; p_len {p_len}; frames per hop: "
         + ", ".join(f"{h}: {1 + x.numel() // h}" for h in HOPS) + f"; {args.reps} repeats after 2 warm-up calls; "
         "host dither draw and its upload included, as in a conversion"]
verdicts = []
for cap in CAPS:
    base = device_ms(lambda: vc.f0_device(x, 0, f"crepe-{cap}"), args.reps)
    lines.append(row(f"f0_device('crepe-{cap}')", base))
    for hop in HOPS:
        ts = device_ms(lambda: vc.f0_device(x, 0, f"mangio-crepe-{cap}", hop_length=hop), args.reps)
        lines.append(row(f"f0_device('mangio-crepe-{cap}', hop {hop})", ts))
        lines.append(stages(cap, hop))
        if hop == 160:
            limit = np.median(base) + (base.max() - base.min())
            verdicts.append(f"mangio-crepe-{cap} at hop 160: median {np.median(ts):.3f} ms against crepe-{cap} "
                            f"{np.median(base):.3f} + spread {base.max() - base.min():.3f} = {limit:.3f} ms: "
                            + ("within it" if np.median(ts) <= limit else "ABOVE it"))
lines += verdicts
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
