"""Time of the discriminator's training step: ``DiscriminatorTrainerAMD.step`` on one segment-sized pair split into forward,
backward, update and the refold of the stepped weights, ``rvc_amd.train_forward.evaluate`` on the 8 x 3 s synthetic
experiment of scripts/train_forward_time.py without D, with D and with the D step, and the reference's own D step
(train.py:851-860: forward, backward, ``optim_d.step()``; through the harness of tests/golden/make_golden_disc_step.py) on
the CPU at the thread count of profiles/r4_cpu_threads.json.

    python scripts/disc_step_time.py --device [--out FILE]      (on the MI355X)
    python scripts/disc_step_time.py --reference [--out FILE]   (build container only: needs the reference)

Each mode appends its lines to ``--out``; profiles/disc_step_time.txt holds both.
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
sys.path.insert(0, os.path.join(REPO, "tests"))
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


def _fmt(t):
    return "%.2f ms (%.2f, %.2f)" % t


def device(n, seconds, reps):
    from rvc_amd import ops
    from rvc_amd import train_forward as tf
    from rvc_amd.discriminator import WEIGHT_DECAY, DiscriminatorTrainerAMD
    hps = synthetic.train_config(SR, VERSION)
    seg = hps["train"]["segment_size"]
    ck = synthetic.make_disc_ckpt(VERSION, SEED)
    ck["optimizer"] = synthetic.discriminator_optimizer_state(VERSION, SEED)
    t0 = time.perf_counter()
    tr = DiscriminatorTrainerAMD(ck, VERSION, hps["train"], "cuda")
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    y = torch.from_numpy(synthetic.synthetic_audio(seg / SR + 0.01, seed=SEED, sr=SR)[:seg]).cuda()
    y_hat = y + 0.1 * torch.from_numpy(synthetic.synthetic_audio(seg / SR + 0.01, seed=SEED + 1, sr=SR)[:seg]).cuda()
    sig = torch.stack([y, y_hat]).contiguous()
    snap = tr.snapshot()
    tr.step([(y, y_hat)])  # warm-up: workspaces
    tr.losses(y, y_hat)
    tr.restore(snap)
    state = {}

    def fwd():
        state["f"] = tr._run(sig)

    def upd():
        for name in tr.names:
            g, v, b = tr.P[name]
            r = tr.rows[name]
            ops.wn_adamw(tr.dW[name], tr.db[name], v, g, b, tr.M[name], tr.table[3 * r:3 * (r + g.numel())], tr.lr,
                         tr.betas, tr.eps, WEIGHT_DECAY, tr.step_count + 1)
        ops.grad_norm(tr.table)
    f = _median_ms(fwd, reps * 2)
    b = _median_ms(lambda: tr._backward(sig, state["f"], 1.0, False), reps * 2)
    u = _median_ms(upd, reps)
    rf = _median_ms(tr._refold, reps)
    tr.restore(snap)

    def whole():
        tr.step([(y, y_hat)])
        tr.restore(snap)
    w = _median_ms(whole, reps)
    rs = _median_ms(lambda: tr.restore(snap), reps)
    lines = [f"device ({torch.cuda.get_device_name(0)}): DiscriminatorTrainerAMD({VERSION!r}) on one {seg}-sample pair; "
             f"median (min, max) of {reps} (forward, backward: {2 * reps})",
             f"  checkpoint and optimizer state load, fold and upload: {load_s:.2f} s (once)",
             f"  forward (both signals, feature maps kept):   {_fmt(f)}",
             f"  backward (loss gradient, dW, db, dx):         {_fmt(b)}",
             f"  update (weight-norm backward, AdamW, norm):   {_fmt(u)}",
             f"  refold of the stepped weights through the host (before the next forward): {_fmt(rf)}",
             f"  step + restore, host reads included:          {_fmt(w)}   (restore alone: {_fmt(rs)})"]
    exp = tempfile.mkdtemp(prefix="rvc_disc_step_time_")
    frames = int(seconds * SR) // hps["data"]["hop_length"]
    ckpt = synthetic.write_train_experiment(exp, SR, VERSION, frames=(frames,) * n, seed=SEED, with_d=True)
    model = tf.TrainSynthAMD(torch.load(ckpt, map_location="cpu", weights_only=False), hps, "cuda")
    tf.evaluate(exp, model, limit=2)
    tf.evaluate(exp, model, limit=2, d_checkpoint=tr)
    g = _median_ms(lambda: tf.evaluate(exp, model), reps)
    gd = _median_ms(lambda: tf.evaluate(exp, model, d_checkpoint=tr), reps)
    gs = _median_ms(lambda: tf.evaluate(exp, model, d_checkpoint=tr, d_step=True), max(2, reps // 2))
    r = tf.evaluate(exp, model, d_checkpoint=tr, d_step=True)
    lines += [f"  evaluate on {n} utterances of {seconds:g} s ({frames} frames), files read from disk each pass:",
              f"    without D:        {g[0]:.1f} ms per pass ({g[1]:.1f}, {g[2]:.1f})",
              f"    with D:           {gd[0]:.1f} ms per pass ({gd[1]:.1f}, {gd[2]:.1f})",
              f"    with D and step:  {gs[0]:.1f} ms per pass = {gs[0] / n:.1f} ms per utterance ({gs[1]:.1f}, {gs[2]:.1f})",
              f"    loss_disc {r['loss_disc']:.4f} loss_gen {r['loss_gen']:.4f} loss_fm {r['loss_fm']:.4f} "
              f"grad_norm_d {r['grad_norm_d']:.3f}"]
    return lines


def reference(n):
    import make_golden as mg
    import make_golden_disc_step as gs
    import make_golden_discriminator as gd
    import make_golden_train_forward as gt
    with open(os.path.join(REPO, "profiles", "r4_cpu_threads.json")) as f:
        threads = json.load(f)["best_threads"]
    hps = synthetic.train_config(SR, VERSION)
    seg, t = hps["train"]["segment_size"], hps["train"]
    work = mg.setup_harness()
    gt.stub_for_train()
    train = gt.import_train(work, hps)
    gs.give_stub_modules_a_spec()
    net_d = gd.build_ref_net(train, VERSION, synthetic.make_disc_ckpt(VERSION, SEED))
    optim_d = torch.optim.AdamW(net_d.parameters(), t["learning_rate"], betas=t["betas"], eps=t["eps"])
    pairs = [[torch.from_numpy(s).view(1, 1, -1) for s in gd.signals(seg, SEED + i, SR)] for i in range(n + 1)]
    threads = min(threads, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    tf = tb = ts = 0.0
    for i, (y, y_hat) in enumerate(pairs):
        t0 = time.perf_counter()
        y_d_r, y_d_g, _, _ = net_d(y, y_hat.detach())
        loss, _, _ = train.discriminator_loss(y_d_r, y_d_g)
        t1 = time.perf_counter()
        optim_d.zero_grad()
        loss.backward()
        t2 = time.perf_counter()
        optim_d.step()
        t3 = time.perf_counter()
        if i:  # the first is the warm-up
            tf, tb, ts = tf + t1 - t0, tb + t2 - t1, ts + t3 - t2
    return [f"reference on this CPU ({os.cpu_count()} logical CPUs), f32, {threads} threads (profiles/r4_cpu_threads.json's "
            f"best, capped at the CPUs there are): net_d on a {seg}-sample pair, discriminator_loss, backward, "
            f"optim_d.step(), {n} pairs one at a time",
            f"  forward {tf / n * 1e3:.1f} ms, backward {tb / n * 1e3:.1f} ms, optim_d.step() {ts / n * 1e3:.1f} ms per pair"]


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
