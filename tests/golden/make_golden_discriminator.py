"""Golden vectors of the discriminator and the GAN losses: the REFERENCE itself, in f32 and in f64.

Run in the survey container only (it needs the reference tree ``make_golden.py`` points at):

    python tests/golden/make_golden_discriminator.py

What runs is ``main/inference/train.py``'s own ``MultiPeriodDiscriminator``, ``feature_loss``, ``discriminator_loss``
and ``generator_loss`` (train.py:608-674, 286-315), imported the way ``make_golden_train_forward.py`` reaches that
module, in the order of the training loop's second pass (train.py:863-869) on the seeded weights of
``rvc_amd.synthetic.make_disc_ckpt`` loaded the way ``load_checkpoint`` loads a ``D_*.pth`` (train.py:257-263).
Nothing here draws random numbers: the f64 run is the f32 module cast up on the same inputs.  The three loss functions
call ``.float()`` on what they are given, so during the f64 run ``torch.Tensor.float`` leaves f64 tensors as they are
(``KeepF64``); nothing else is changed in them.

``discriminator_<case>.npz`` holds ``y`` and ``y_hat``; every ``y_d`` of the f64 run (flattened as the reference
flattens them); per feature map, in the reference's list order, the f64 ``mean |r - g|``, the RMS of both maps and
a sample of at most 256 values of each at a fixed stride through the reference's flatten order (``fm_stride``:
flat indices 0, s, 2s, ...); all losses of both runs; and ``ref_dev``: the f32 run's deviation from the f64 run per
quantity -- for ``y_d`` and ``fmap`` the largest relative RMS and the largest absolute deviation over the list, for
the scalars the relative deviation.  The 71 M weights are not stored: ``weight_g`` is drawn, not computed, so the
checkpoint regenerates bit for bit from the seed.  ``discriminator_keys.json``: keys and shapes of the reference
modules' own ``state_dict()`` in the checkpoint's naming.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_train_forward as mgt  # noqa: E402
from rvc_amd import synthetic  # noqa: E402

OUT = mg.OUT
SAMPLE = 256
LOSSES = ("loss_disc", "loss_gen", "loss_fm")
LISTS = ("losses_gen", "losses_disc_r", "losses_disc_g")
D_SEED = 5100  # one synthetic D per version: the tests build each once
#        name version t      signal seed
CASES = [("a", "v2", 12800, 5101),  # t % p = 0, 2, 0, 4, 7, 16, 12, 35: padded and unpadded periods
         ("b", "v2", 2741, 5102),   # prime: every period pads; p = 37 ends at H = 75 -> 25 -> 9 -> 3 -> 1 -> 1
         ("c", "v1", 12800, 5103)]  # six periods


def signals(t, seed, sr=40000):
    """y: the synthetic test signal; y_hat: y plus a second seeded signal at about -20 dB."""
    y = synthetic.synthetic_audio(t / sr + 0.01, seed=seed, sr=sr)[:t]
    other = synthetic.synthetic_audio(t / sr + 0.01, seed=seed + 1, sr=sr)[:t]
    return y, (y + np.float32(0.1) * other).astype(np.float32)


def build_ref_net(train, version, ck):
    net_d = train.MultiPeriodDiscriminator(version, use_spectral_norm=False, checkpointing=False)
    sd = train.replace_keys_in_dict(train.replace_keys_in_dict(dict(ck["model"]), ".weight_v",
                                                               ".parametrizations.weight.original1"),
                                    ".weight_g", ".parametrizations.weight.original0")
    missing, unexpected = net_d.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return net_d.train().float()


class KeepF64:
    """``x.float()`` on an f64 tensor returns it unchanged, so the reference's loss functions stay in f64."""

    def __enter__(self):
        self._float = torch.Tensor.float
        keep = self._float
        torch.Tensor.float = lambda x, *a, **k: x if x.dtype == torch.float64 else keep(x, *a, **k)
        return self

    def __exit__(self, *a):
        torch.Tensor.float = self._float


def step(train, net_d, y, y_hat):
    """train.py:863, 867-868 and :854 on one pair -> outputs, feature maps and the losses."""
    y_d_r, y_d_g, fmap_r, fmap_g = net_d(y, y_hat)
    loss_disc, losses_disc_r, losses_disc_g = train.discriminator_loss(y_d_r, y_d_g)
    loss_fm = train.feature_loss(fmap_r, fmap_g)
    loss_gen, losses_gen = train.generator_loss(y_d_g)
    return dict(y_d_r=y_d_r, y_d_g=y_d_g, fmap_r=[f for d in fmap_r for f in d], fmap_g=[f for d in fmap_g for f in d],
                loss_disc=loss_disc, loss_fm=loss_fm, loss_gen=loss_gen, losses_gen=[float(l) for l in losses_gen],
                losses_disc_r=losses_disc_r, losses_disc_g=losses_disc_g)


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


def list_dev(a32, b64):
    """Largest relative RMS and largest absolute deviation of the f32 list from the f64 list."""
    rel = max(rms(a.double() - b) / rms(b) for a, b in zip(a32, b64))
    return [rel, max(float((a.double() - b).abs().max()) for a, b in zip(a32, b64))]


def gen_case(train, name, version, t, sig_seed):
    seed = D_SEED
    net_d = build_ref_net(train, version, synthetic.make_disc_ckpt(version, seed))
    y, y_hat = signals(t, sig_seed)
    ty, tg = torch.from_numpy(y).view(1, 1, -1), torch.from_numpy(y_hat).view(1, 1, -1)
    with torch.no_grad():
        r32 = step(train, net_d, ty, tg)
        net64 = net_d.double()
        with KeepF64():
            r64 = step(train, net64, ty.double(), tg.double())
        assert r64["loss_fm"].dtype == r64["loss_disc"].dtype == r64["loss_gen"].dtype == torch.float64
    n_fm = len(r64["fmap_r"])
    strides = np.array([max(1, -(-f.numel() // SAMPLE)) for f in r64["fmap_r"]], np.int64)
    sample = lambda f, s: f.reshape(-1)[::int(s)].numpy()  # noqa: E731
    sr_ = [sample(f, s) for f, s in zip(r64["fmap_r"], strides)]
    sg_ = [sample(f, s) for f, s in zip(r64["fmap_g"], strides)]
    assert all(v.size <= SAMPLE for v in sr_)
    fm_l1 = np.array([float((r - g).abs().mean()) for r, g in zip(r64["fmap_r"], r64["fmap_g"])])
    # feature_loss's own f64 value from these terms, in its order
    assert abs(2 * fm_l1.sum() / float(r64["loss_fm"]) - 1) < 1e-12
    ref_dev = {"y_d_r": list_dev(r32["y_d_r"], r64["y_d_r"]), "y_d_g": list_dev(r32["y_d_g"], r64["y_d_g"]),
               "fmap_r": list_dev(r32["fmap_r"], r64["fmap_r"]), "fmap_g": list_dev(r32["fmap_g"], r64["fmap_g"]),
               "fm_l1": [float(np.max(np.abs(np.array([float((r - g).abs().mean()) for r, g in
                                                        zip(r32["fmap_r"], r32["fmap_g"])]) / fm_l1 - 1))), 0.0]}
    for k in LOSSES:
        ref_dev[k] = [abs(float(r32[k]) / float(r64[k]) - 1), 0.0]
    for k in LISTS:
        ref_dev[k] = [float(np.max(np.abs(np.array(r32[k], np.float64) / np.array(r64[k], np.float64) - 1))), 0.0]
    names = sorted(ref_dev)
    np.savez_compressed(
        os.path.join(OUT, f"discriminator_{name}.npz"), version=version, seed=seed, sig_seed=sig_seed, t=t, y=y, y_hat=y_hat,
        y_d_sizes=np.array([v.numel() for v in r64["y_d_r"]]),
        y_d_r_f64=np.concatenate([v.reshape(-1).numpy() for v in r64["y_d_r"]]),
        y_d_g_f64=np.concatenate([v.reshape(-1).numpy() for v in r64["y_d_g"]]),
        fm_shapes=np.array([list(f.shape) + [1] * (4 - f.dim()) for f in r64["fmap_r"]]),
        fm_l1_f64=fm_l1, fm_rms_r_f64=np.array([rms(f) for f in r64["fmap_r"]]),
        fm_rms_g_f64=np.array([rms(f) for f in r64["fmap_g"]]), fm_stride=strides,
        fm_sample_sizes=np.array([v.size for v in sr_]), fm_sample_r_f64=np.concatenate(sr_),
        fm_sample_g_f64=np.concatenate(sg_),
        **{k + "_f64": np.float64(float(r64[k])) for k in LOSSES}, **{k + "_f32": np.float32(float(r32[k])) for k in LOSSES},
        **{k + "_f64": np.array(r64[k], np.float64) for k in LISTS}, **{k + "_f32": np.array(r32[k], np.float32) for k in LISTS},
        ref_dev_names=np.array(names), ref_dev=np.array([ref_dev[k] for k in names]))
    print(name, "n_fm", n_fm, {k: float(r64[k]) for k in LOSSES})
    print("   fmap rms r:", " ".join("%.2f" % rms(f) for f in r64["fmap_r"]))
    for k in names:
        print("   %-14s rel %.3e max %.3e" % (k, *ref_dev[k]))
    return net_d


def main():
    work = mg.setup_harness()
    mgt.stub_for_train()
    train = mgt.import_train(work, synthetic.train_config(40000, "v2"))
    tables = {}
    for case in CASES:
        net_d = gen_case(train, *case)
        sd = train.replace_keys_in_dict(train.replace_keys_in_dict(
            dict(net_d.state_dict()), ".parametrizations.weight.original1", ".weight_v"),
            ".parametrizations.weight.original0", ".weight_g")
        tables[case[1]] = {k: list(v.shape) for k, v in sd.items()}
    with open(os.path.join(OUT, "discriminator_keys.json"), "w") as f:
        json.dump(tables, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
