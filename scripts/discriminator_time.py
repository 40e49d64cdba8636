"""Time of the checkpoint scorer with and without a discriminator: ``rvc_amd.train_forward.evaluate`` on the 8 x 3 s
synthetic experiment of scripts/train_forward_time.py, and the reference's own ``net_d`` plus its three loss functions
(train.py:863, 286-315, through the harness of tests/golden/make_golden_discriminator.py) on segment-sized pairs on the
CPU at the thread count of profiles/r4_cpu_threads.json.

    python scripts/discriminator_time.py --device [--out FILE]      (on the MI355X)
    python scripts/discriminator_time.py --reference [--out FILE]   (build container only: needs the reference)

Each mode appends its lines to ``--out``; profiles/discriminator_time.txt holds both.
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


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def device(n, seconds, reps):
    from rvc_amd import train_forward as tf
    from rvc_amd.discriminator import DiscriminatorAMD
    exp = tempfile.mkdtemp(prefix="rvc_discriminator_time_")
    hop = synthetic.train_config(SR, VERSION)["data"]["hop_length"]
    frames = int(seconds * SR) // hop
    ckpt = synthetic.write_train_experiment(exp, SR, VERSION, frames=(frames,) * n, seed=SEED, with_d=True)
    hps = json.load(open(os.path.join(exp, "config.json")))
    model = tf.TrainSynthAMD(torch.load(ckpt, map_location="cpu", weights_only=False), hps, "cuda")
    t0 = time.perf_counter()
    disc = DiscriminatorAMD(torch.load(os.path.join(exp, "D_1.pth"), map_location="cpu", weights_only=False),
                            VERSION, "cuda")
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    tf.evaluate(exp, model, limit=2)  # warm-up: allocator, workspaces, mel basis
    tf.evaluate(exp, model, limit=2, d_checkpoint=disc)
    g = _median_ms(lambda: tf.evaluate(exp, model), reps)
    gd = _median_ms(lambda: tf.evaluate(exp, model, d_checkpoint=disc), reps)
    y = torch.randn(2, hps["train"]["segment_size"], device="cuda") * 0.2
    d_only = _median_ms(lambda: disc.losses(y[0], y[1]), reps * 4)
    r = tf.evaluate(exp, model, d_checkpoint=disc)
    return [f"device ({torch.cuda.get_device_name(0)}): evaluate on {n} utterances of {seconds:g} s ({frames} frames, "
            f"{SR // 1000}k {VERSION}), wav and feature files read from disk each pass; median (min, max) of {reps}",
            f"  D checkpoint load, fold and upload: {load_s:.2f} s (once)",
            f"  evaluate without D: {g[0]:.1f} ms per pass = {g[0] / n:.2f} ms per utterance ({g[1]:.1f}, {g[2]:.1f})",
            f"  evaluate with D:    {gd[0]:.1f} ms per pass = {gd[0] / n:.2f} ms per utterance ({gd[1]:.1f}, {gd[2]:.1f})",
            f"  DiscriminatorAMD.losses alone on a {hps['train']['segment_size']}-sample pair: {d_only[0]:.2f} ms "
            f"({d_only[1]:.2f}, {d_only[2]:.2f})",
            f"  loss_disc {r['loss_disc']:.4f} loss_gen {r['loss_gen']:.4f} loss_fm {r['loss_fm']:.4f} "
            f"loss_gen_all {r['loss_gen_all']:.4f}"]


def reference(n):
    import make_golden as mg
    import make_golden_discriminator as gd
    import make_golden_train_forward as gt
    with open(os.path.join(REPO, "profiles", "r4_cpu_threads.json")) as f:
        threads = json.load(f)["best_threads"]
    hps = synthetic.train_config(SR, VERSION)
    seg = hps["train"]["segment_size"]
    work = mg.setup_harness()
    gt.stub_for_train()
    train = gt.import_train(work, hps)
    net_d = gd.build_ref_net(train, VERSION, synthetic.make_disc_ckpt(VERSION, SEED))
    pairs = [[torch.from_numpy(s).view(1, 1, -1) for s in gd.signals(seg, SEED + i, SR)] for i in range(n)]
    threads = min(threads, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    with torch.no_grad():
        gd.step(train, net_d, *pairs[0])  # warm-up
        t0 = time.perf_counter()
        for p in pairs:
            gd.step(train, net_d, *p)
        dt = time.perf_counter() - t0
    return [f"reference on this CPU ({os.cpu_count()} logical CPUs), f32, {threads} threads (profiles/"
            f"r4_cpu_threads.json's best, capped at the CPUs there are): MultiPeriodDiscriminator({VERSION!r}) on a "
            f"{seg}-sample pair, feature_loss, discriminator_loss and generator_loss, {n} pairs one at a time",
            f"  {dt / n * 1e3:.1f} ms per pair"]


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
        lines += reference(a.n)
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
