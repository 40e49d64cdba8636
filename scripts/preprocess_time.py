"""Wall time of PreProcessAMD.process_audio (rvc_amd.preprocess, csrc/preprocess.hip) on one long file, beside the
same chain in numpy / scipy on the CPU (tests/preprocess_ref.py), and the device time of each of the four operations.

    python scripts/preprocess_time.py [--minutes 10] [--sr 48000] [--reps 5] [--out profiles/preprocess_time.txt]

The file is synthetic speech-like audio with a silence every 15 s, written as a float32 WAV.  process_audio is timed
end to end (WAV read, upload, kernels, the RMS read-back, the plan, the slices' read-back and the WAV writes) and
its device operations again one by one between device events on the same input.
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import preprocess_ref
from rvc_amd import audio_io, synthetic
from rvc_amd import preprocess as pre

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--sr", type=int, default=48000)
ap.add_argument("--per", type=float, default=3.7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev, sr = "cuda", args.sr
spans = int(round(args.minutes * 60 / 15))
audio = synthetic.silence_layout_audio([(14.0, 1), (1.0, 0)] * spans, seed=6300, sr=sr)
work = tempfile.mkdtemp(prefix="pre_time_")
wav = os.path.join(work, "input.wav")
audio_io.write_wav_f32(wav, audio, sr)
lines = [f"file: {audio.size / sr / 60:.1f} min at {sr} Hz = {audio.size} samples, float32 WAV; per = {args.per} s, "
         f"cut_preprocess = process_effects = True, clean_dataset = False"]

pp = pre.PreProcessAMD(sr, os.path.join(work, "exp"), args.per, dev)
walls = []
for _ in range(1 + args.reps):  # the first call loads the library and fills the allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pp.process_audio(wav, 0, 0, True, True, False, 0.7)
    torch.cuda.synchronize()
    walls.append(time.perf_counter() - t0)
w = np.asarray(walls[1:])
lines.append(f"process_audio on the device: {len(out['names'])} chunks; wall median {np.median(w):.3f} s, min "
             f"{w.min():.3f}, max {w.max():.3f} over {args.reps} calls (first call {walls[0]:.3f} s); warm-up "
             f"{pp.warm} samples per {pre._lib.LFILTER_CHUNK}-sample chunk")

t0 = time.perf_counter()
loaded = audio_io.load_audio(wav, sr)
t_load = time.perf_counter() - t0
t0 = time.perf_counter()
ref = preprocess_ref.chain(loaded, sr, args.per)
t_cpu = time.perf_counter() - t0
t0 = time.perf_counter()
for k, (g, s) in enumerate(zip(ref["gt"], ref["k16"])):
    audio_io.write_wav_f32(os.path.join(work, f"gt_{k}.wav"), g, sr)
    audio_io.write_wav_f32(os.path.join(work, f"k16_{k}.wav"), s, 16000)
t_write = time.perf_counter() - t0
assert np.array_equal(ref["offsets"], out["offsets"])
lines.append(f"the same chain in scipy on the CPU (lfilter, mix, get_rms, slicer, resample_poly per chunk): "
             f"{t_cpu:.3f} s; reading the WAV {t_load:.3f} s and writing the {2 * len(ref['gt'])} slices {t_write:.3f} s "
             f"are common to both")


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
    return float(np.median(ts))


x = torch.from_numpy(loaded).to(dev)
y = pre.lfilter(x, pp.b_high, pp.a_high, pp.warm)
z, _ = pre.peak_mix(y)
chunks = [tuple(int(v) for v in c) for c in out["offsets"]]
ops = {"rvc_lfilter64": lambda: pre.lfilter(x, pp.b_high, pp.a_high, pp.warm),
       "rvc_peak_mix64": lambda: pre.peak_mix(y),
       "rvc_frame_rms64": lambda: pre.frame_rms(z, pp.slicer.win_size, pp.slicer.hop_size),
       "rvc_resample_poly64": lambda: pre.resample_poly(z, pp.up, pp.down, chunks, pp.taps())}
ms = {k: device_ms(f, args.reps) for k, f in ops.items()}
total = sum(ms.values())
lines.append(f"device time per operation (events around each call, allocation included; median of {args.reps}), "
             f"sum {total:.3f} ms:")
for k, v in ms.items():
    lines.append(f"  {k:22s} {v:9.3f} ms  {100 * v / total:5.1f} %")
n = audio.size
lines.append(f"rvc_lfilter64 runs {pp.warm + pre._lib.LFILTER_CHUNK} recurrence steps per {pre._lib.LFILTER_CHUNK} "
             f"outputs: {n * (pp.warm + pre._lib.LFILTER_CHUNK) / pre._lib.LFILTER_CHUNK * 21 / ms['rvc_lfilter64'] / 1e9:.2f} "
             f"Tflop/s of f64 (21 operations per step)")
lines.append("nothing here was predicted in advance: first measurements of a path that did not exist before")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
