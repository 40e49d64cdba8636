"""Golden vectors of the discriminator's training step: the REFERENCE itself, in f32 and in f64.

Run in the survey container only (it needs the reference tree ``make_golden.py`` points at), never on the GPU host:

    python tests/golden/make_golden_disc_step.py

What runs is ``main/inference/train.py:851-869`` on ``net_d`` alone: the reference's ``MultiPeriodDiscriminator`` on
``(wave, y_hat.detach())``, ``discriminator_loss``, ``optim_d.zero_grad(); loss_disc.backward()``,
``clip_grad_value(net_d.parameters(), None)`` (commons.py:48-60), ``optim_d.step()`` of a
``torch.optim.AdamW(net_d.parameters(), learning_rate, betas=betas, eps=eps)`` built with train.py:766's arguments, then the
second ``net_d(wave, y_hat)`` with ``feature_loss`` and ``generator_loss``.  The weights are
``rvc_amd.synthetic.make_disc_ckpt``'s, the signals ``make_golden_discriminator.signals``', the warm optimizer state
``rvc_amd.synthetic.discriminator_optimizer_state``'s, loaded through ``optimizer.load_state_dict``.  The f64 run is the
same module and state cast up (``KeepF64`` as in ``make_golden_discriminator.py``); nothing draws random numbers.

``disc_step_<case>.npz``: ``y`` and ``y_hat`` [n][t]; per parameter tensor, in ``net_d.parameters()``' order, the f64
gradient's norm and a sample of at most 128 values at a fixed stride through its flatten order (small tensors whole) of the
f64 gradient and of the f64 value after the step (``sizes``: the sample sizes; tests/disc_step_ref.py ``sample_index``);
``grad_norm_d`` and every loss of both passes of both runs; ``ref_dev``: the f32 run's deviation from the f64 run --
``grad`` (largest relative RMS of a tensor's gradient sample, largest absolute deviation), ``grad_norms`` and the scalars
(relative deviation), ``post`` (the largest ``(|p32 - p64| - ulp(p64)) / |p64 - p_before|`` over the samples, the tolerance
form of the test).  ``disc_step_param_order.json``: names (checkpoint naming) and shapes of ``net_d.parameters()``.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_discriminator as mgd  # noqa: E402
import make_golden_train_forward as mgt  # noqa: E402
from disc_step_ref import sample_index  # noqa: E402
from rvc_amd import synthetic  # noqa: E402

OUT = mg.OUT
OPT_SEED = 5200
FIRST = ("loss_disc",)
SECOND = ("loss_gen", "loss_fm")
LISTS = ("losses_disc_r", "losses_disc_g")
#        name version t      signal seeds   warm
CASES = [("a", "v2", 12800, (5101, 5111), True),   # two pairs as one batch of 2
         ("b", "v2", 2741, (5102,), True),         # prime: every period pads, the last period maps are 1 row
         ("c", "v1", 12800, (5103,), False)]       # no optimizer state: the first step


def ckpt_name(n):
    return n.replace(".parametrizations.weight.original0", ".weight_g").replace(".parametrizations.weight.original1",
                                                                                ".weight_v")


def run(train, commons, net_d, hps, opt_state, y, y_hat):
    """train.py:851-869 on net_d: losses, gradients, grad_norm_d, the stepped parameters, the second pass' losses."""
    t = hps["train"]
    optim_d = torch.optim.AdamW(net_d.parameters(), t["learning_rate"], betas=t["betas"], eps=t["eps"])
    if opt_state is not None:
        optim_d.load_state_dict(opt_state)
    y_d_r, y_d_g, _, _ = net_d(y, y_hat.detach())
    loss_disc, losses_disc_r, losses_disc_g = train.discriminator_loss(y_d_r, y_d_g)
    optim_d.zero_grad()
    loss_disc.backward()
    grad_norm_d = commons.clip_grad_value(net_d.parameters(), None)
    grads = [p.grad.detach().clone() for p in net_d.parameters()]
    before = [p.detach().clone() for p in net_d.parameters()]
    optim_d.step()
    with torch.no_grad():
        y_d_r, y_d_g, fmap_r, fmap_g = net_d(y, y_hat)
        loss_fm = train.feature_loss(fmap_r, fmap_g)
        loss_gen, _ = train.generator_loss(y_d_g)
    return dict(loss_disc=float(loss_disc), losses_disc_r=losses_disc_r, losses_disc_g=losses_disc_g,
                grad_norm_d=float(grad_norm_d), grads=grads, before=before,
                after=[p.detach().clone() for p in net_d.parameters()], loss_fm=float(loss_fm), loss_gen=float(loss_gen),
                dtype=loss_disc.dtype)


def ulp(x):
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


def gen_case(train, commons, name, version, t, sig_seeds, warm):
    hps = synthetic.train_config(40000, version)
    ck = synthetic.make_disc_ckpt(version, mgd.D_SEED)
    sig = [mgd.signals(t, s) for s in sig_seeds]
    y = np.stack([a for a, _ in sig])
    y_hat = np.stack([b for _, b in sig])
    ty, tg = torch.from_numpy(y).unsqueeze(1), torch.from_numpy(y_hat).unsqueeze(1)
    # a fresh copy per run: load_state_dict keeps f32 tensors as they are, and the step then updates them in place
    state = lambda: synthetic.discriminator_optimizer_state(version, OPT_SEED) if warm else None  # noqa: E731
    r32 = run(train, commons, mgd.build_ref_net(train, version, ck), hps, state(), ty, tg)
    net64 = mgd.build_ref_net(train, version, ck).double()
    with mgd.KeepF64():
        r64 = run(train, commons, net64, hps, state(), ty.double(), tg.double())
    assert r64["dtype"] == torch.float64 and r64["grads"][0].dtype == torch.float64
    names = [ckpt_name(n) for n, _ in net64.named_parameters()]
    idx = [sample_index(g.numel()) for g in r64["grads"]]
    take = lambda ts: [v.reshape(-1).double().numpy()[i] for v, i in zip(ts, idx)]  # noqa: E731
    g64, g32, a64, a32, b64 = take(r64["grads"]), take(r32["grads"]), take(r64["after"]), take(r32["after"]), \
        take(r64["before"])
    norms64 = np.array([float(g.norm()) for g in r64["grads"]])
    norms32 = np.array([float(g.double().norm()) for g in r32["grads"]])
    rel = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))  # noqa: E731
    ref_dev = {"grad": [max(rel(a, b) for a, b in zip(g32, g64)), max(float(np.abs(a - b).max()) for a, b in zip(g32, g64))],
               "grad_norms": [float(np.abs(norms32 / norms64 - 1).max()), 0.0],
               "post": [max(float(np.max(np.maximum(np.abs(a - b) - ulp(b), 0) / np.abs(b - c)))
                            for a, b, c in zip(a32, a64, b64)), 0.0]}
    for k in FIRST + SECOND + ("grad_norm_d",):
        ref_dev[k] = [abs(r32[k] / r64[k] - 1), 0.0]
    for k in LISTS:
        ref_dev[k] = [float(np.max(np.abs(np.array(r32[k]) / np.array(r64[k]) - 1))), 0.0]
    dev_names = sorted(ref_dev)
    scal = FIRST + SECOND + ("grad_norm_d",)
    np.savez_compressed(
        os.path.join(OUT, f"disc_step_{name}.npz"), version=version, seed=mgd.D_SEED, opt_seed=OPT_SEED, warm=int(warm),
        step=(synthetic.OPT_STATE_STEP if warm else 0) + 1, t=t, y=y, y_hat=y_hat,
        sizes=np.array([i.size for i in idx]), grad_norms_f64=norms64, grad_f64=np.concatenate(g64),
        post_f64=np.concatenate(a64), before_f64=np.concatenate(b64),
        **{k + "_f64": np.float64(r64[k]) for k in scal}, **{k + "_f32": np.float32(r32[k]) for k in scal},
        **{k + "_f64": np.array(r64[k], np.float64) for k in LISTS}, **{k + "_f32": np.array(r32[k], np.float32) for k in LISTS},
        ref_dev_names=np.array(dev_names), ref_dev=np.array([ref_dev[k] for k in dev_names]))
    print(name, {k: r64[k] for k in scal})
    for k in dev_names:
        print("   %-14s rel %.3e max %.3e" % (k, *ref_dev[k]))
    return names, [list(p.shape) for p in net64.parameters()]


def give_stub_modules_a_spec():
    """torch.optim imports torch._dynamo, which asks every module it knows for a spec; the harness' stub modules have
    none."""
    import importlib.machinery
    for mod_name, mod in list(sys.modules.items()):
        if mod is not None and getattr(mod, "__spec__", None) is None and mod_name != "__main__":
            mod.__spec__ = importlib.machinery.ModuleSpec(mod_name, None)


def main():
    work = mg.setup_harness()
    mgt.stub_for_train()
    train = mgt.import_train(work, synthetic.train_config(40000, "v2"))
    import importlib
    give_stub_modules_a_spec()
    commons = importlib.import_module(train.clip_grad_value.__module__)
    order = {}
    for case in CASES:
        names, shapes = gen_case(train, commons, *case)
        order[case[1]] = [[n, s] for n, s in zip(names, shapes)]
    with open(os.path.join(OUT, "disc_step_param_order.json"), "w") as f:
        json.dump(order, f, indent=0)


if __name__ == "__main__":
    main()
