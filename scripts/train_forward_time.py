"""Time of the checkpoint scorer: ``rvc_amd.train_forward.evaluate`` on N synthetic 3 s utterances on the device,
and the reference's own forward plus losses (train.py:843-848, 865-866, through the harness of
tests/golden/make_golden_train_forward.py) on the same utterances on the CPU at its best thread count.

    python scripts/train_forward_time.py --device    [--n 8] [--out FILE]   (on the MI355X)
    python scripts/train_forward_time.py --reference [--n 8] [--out FILE]   (build container only: needs the reference)

Each mode appends its lines to ``--out``; profiles/train_forward_time.txt holds both.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
from rvc_amd import synthetic  # noqa: E402

SR, VERSION, SEED = 40000, "v2", 1234


def experiment(n, seconds):
    exp = tempfile.mkdtemp(prefix="rvc_train_forward_time_")
    frames = int(seconds * SR) // synthetic.train_config(SR, VERSION)["data"]["hop_length"]
    ckpt = synthetic.write_train_experiment(exp, SR, VERSION, frames=(frames,) * n, seed=SEED)
    return exp, ckpt, frames


def device(n, seconds, reps):
    from rvc_amd import train_forward as tf
    exp, ckpt, frames = experiment(n, seconds)
    hps = json.load(open(os.path.join(exp, "config.json")))
    t0 = time.perf_counter()
    model = tf.TrainSynthAMD(torch.load(ckpt, map_location="cpu", weights_only=False), hps, "cuda")
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    tf.evaluate(exp, model, limit=2)  # warm-up: allocator, workspaces, mel basis
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tf.evaluate(exp, model)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts)
    return [f"device ({torch.cuda.get_device_name(0)}): evaluate on {n} utterances of {seconds:g} s ({frames} frames, "
            f"{SR // 1000}k {VERSION}), wav and feature files read from disk each pass",
            f"  checkpoint load, fold and upload: {load_s:.2f} s (once)",
            f"  evaluate: median {np.median(ts) * 1e3:.1f} ms per pass = "
            f"{np.median(ts) / n * 1e3:.2f} ms per utterance "
            f"(min {ts.min() * 1e3:.1f}, max {ts.max() * 1e3:.1f} ms over {reps} passes)",
            f"  loss_mel {r['loss_mel']:.4f} loss_kl {r['loss_kl']:.4f} (scored {r['scored']}, skipped {r['skipped']})"]


def reference(n, seconds):
    import make_golden as mg
    import make_golden_train_forward as gt
    from rvc_amd import audio_io, train_forward as tf
    exp, _, frames = experiment(n, seconds)
    hps = synthetic.train_config(SR, VERSION)
    work = mg.setup_harness()
    gt.stub_for_train()
    train = gt.import_train(work, hps)
    net_g = gt.build_ref_net(train, hps, synthetic.make_train_ckpt(SR, VERSION, SEED), 768)
    utts = []
    for wav, pp, cp, fp, sid in tf.read_filelist(os.path.join(exp, "filelist.txt")):
        x, _ = audio_io.read_wav(wav)
        phone, pitch, pitchf, T = tf.trim_labels(np.load(pp), np.load(cp), np.load(fp),
                                                 x.size // hps["data"]["hop_length"])
        utts.append([torch.from_numpy(x[None]), torch.from_numpy(phone[None]), torch.from_numpy(pitch[None]),
                     torch.from_numpy(pitchf[None]), torch.tensor([int(sid)])])
    lines = [f"reference on this CPU ({os.cpu_count()} logical CPUs), f32: spectrogram_torch, Synthesizer.forward in "
             f"train mode, spec_to_mel_torch, mel_spectrogram_torch, l1_loss and kl_loss on the same {n} utterances, "
             "one at a time, tensors already in memory"]
    best = None
    for threads in (1, 2, 4, 8, 16, 32):
        if threads > (os.cpu_count() or 1):
            break
        torch.set_num_threads(threads)
        with torch.no_grad():
            gt.step(train, net_g, hps, *utts[0])  # warm-up
            t0 = time.perf_counter()
            for u in utts:
                gt.step(train, net_g, hps, *u)
            dt = time.perf_counter() - t0
        lines.append(f"  {threads:2d} threads: {dt / n * 1e3:.1f} ms per utterance")
        if best is None or dt < best[1]:
            best = (threads, dt)
    lines.append(f"  best: {best[0]} threads, {best[1] / n * 1e3:.1f} ms per utterance")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = os.path.abspath(a.out) if a.out else None  # the reference harness changes the working directory
    lines = []
    if a.device:
        lines += device(a.n, a.seconds, a.reps)
    if a.reference:
        lines += reference(a.n, a.seconds)
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
