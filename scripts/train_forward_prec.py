"""Precision of the training forward on the device against the reference's f64 stages (tests/golden/train_forward_*):
per fixture and stage the device's RMS and max deviation from the f64 yardstick, next to the reference f32's own
(the fixture's ref_dev).  tests/test_gpu_train_forward.py takes its bounds from this table (4 x the device figures,
never above 1e-4 relative RMS).

    python scripts/train_forward_prec.py --out profiles/train_forward_prec.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from rvc_amd import ops, synthetic, train_forward as tf  # noqa: E402
from train_forward_ref import fixture_ckpt  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
CASES = {"a": (40000, "v2"), "b": (48000, "v2"), "c": (32000, "v1")}
STAGES = ("spec", "m_q", "logs_q", "z", "z_p", "y_hat", "y_mel", "y_hat_mel")


def device_stages(name, dev="cuda"):
    sr, version = CASES[name]
    fx = dict(np.load(os.path.join(GOLDEN, f"train_forward_{name}.npz")))
    fx["spec_f64"] = np.load(os.path.join(GOLDEN, f"train_forward_{name}_spec.npz"))["spec_f64"]
    hps = synthetic.train_config(sr, version)
    d = hps["data"]
    model = tf.TrainSynthAMD(fixture_ckpt(fx, sr, version), hps, dev)
    t = lambda k: torch.from_numpy(fx[k]).to(dev)  # noqa: E731
    spec = tf.spectrogram(t("wav"), d["filter_length"], d["hop_length"], d["win_length"])
    ids = tf.slice_start(t("slice_u"), int(fx["T"]), int(fx["S"]))
    y_hat, ids, (z, z_p, m_p, logs_p, m_q, logs_q) = model.forward(
        t("phone"), t("pitch"), t("pitchf"), spec[0], int(fx["sid"][0]), ids_slice=ids, z_noise=t("z_noise"),
        sine_noise=t("sine_noise"), sine_phase=t("sine_phase"))
    margs = (d["filter_length"], d["n_mel_channels"], d["sample_rate"], d["mel_fmin"], d["mel_fmax"])
    mel = tf.spec_to_mel(spec, *margs)
    S, st = int(fx["S"]), int(ids.item())
    y_hat_mel = tf.mel_spectrogram(y_hat.view(1, -1), margs[0], margs[1], margs[2], d["hop_length"], d["win_length"],
                                   margs[3], margs[4])
    l1, kl = ops.slice_l1(mel, ids, y_hat_mel), ops.kl_loss(z_p, logs_q, m_p, logs_p)
    got = dict(spec=spec, m_q=m_q, logs_q=logs_q, z=z, z_p=z_p, y_hat=y_hat.view(1, 1, -1),
               y_mel=mel[:, :, st:st + S], y_hat_mel=y_hat_mel)
    got = {k: v.double().cpu().numpy() for k, v in got.items()}
    got["loss_mel"] = float(l1.item()) * hps["train"]["c_mel"]
    got["loss_kl"] = float(kl.item()) * hps["train"]["c_kl"]
    got["ids_slice"] = ids.cpu().numpy()
    return fx, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_forward_prec.txt"))
    a = ap.parse_args()
    lines = ["# training forward on the device vs the reference's f64 stages (scripts/train_forward_prec.py)",
             "# dev_* : device f32 - reference f64;  ref_* : reference f32 - reference f64 (the fixture's ref_dev)",
             "# %-4s %-10s %11s %11s %11s %11s %11s %11s" % ("case", "stage", "dev_rms", "dev_max", "dev_relrms",
                                                            "ref_rms", "ref_max", "f64_rms")]
    for name in CASES:
        fx, got = device_stages(name)
        assert np.array_equal(got["ids_slice"], fx["ids_slice"]), (got["ids_slice"], fx["ids_slice"])
        ref_dev = dict(zip([str(s) for s in fx["ref_dev_stages"]], fx["ref_dev"]))
        for k in STAGES:
            want = fx[k + "_f64"].reshape(got[k].shape)
            e = got[k] - want
            rms, mx, w = float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max()), float(np.sqrt(np.mean(want ** 2)))
            lines.append("  %-4s %-10s %11.3e %11.3e %11.3e %11.3e %11.3e %11.3e" % (
                name, k, rms, mx, rms / w, ref_dev[k][0], ref_dev[k][1], w))
        for k in ("loss_mel", "loss_kl"):
            want, r32 = float(fx[k + "_f64"]), float(fx[k + "_f32"])
            lines.append("  %-4s %-10s device %.7f  f64 %.7f  rel %.3e | reference f32 %.7f  rel %.3e" % (
                name, k, got[k], want, abs(got[k] / want - 1), r32, abs(r32 / want - 1)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
