"""The discriminator's training step without a device: the f64 restatement tests/disc_step_ref.py against the reference's
own f64 autograd run (tests/golden/disc_step_*.npz), the checkpoint layout, the seeded optimizer state and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import disc_step_ref as R
from rvc_amd import synthetic
from rvc_amd import discriminator as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10  # f64 against f64, another summation order


@pytest.fixture(scope="module")
def restated():
    """The restated step of every fixture, computed once."""
    out = {}
    for case, version in R.CASES.items():
        fx = np.load(os.path.join(GOLDEN, f"disc_step_{case}.npz"))
        ck = R.fixture_ckpt(fx)
        state = R.state_by_key(ck["optimizer"], version) if int(fx["warm"]) else None
        lr, betas, eps = R.hyper(version)
        out[case] = (fx, ck, R.step(ck["model"], version, fx["y"], fx["y_hat"], state, int(fx["step"]), lr, betas, eps))
    return out


def close_per_tensor(got, want, sizes):
    off = 0
    for n in sizes:
        a, b = got[off:off + n], want[off:off + n]
        assert np.abs(a - b).max() <= TOL * np.abs(b).max()
        off += n
    assert off == got.size == want.size


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_reproduces_reference_f64(case, restated):
    fx, _, r = restated[case]
    close_per_tensor(R.fixture_samples(fx, r["grads"]), fx["grad_f64"], fx["sizes"])
    close_per_tensor(R.fixture_samples(fx, r["model"]), fx["post_f64"], fx["sizes"])
    norms = np.array([float(r["grads"][k].pow(2).sum().sqrt()) for k in D.discriminator_keys(str(fx["version"]))])
    np.testing.assert_allclose(norms, fx["grad_norms_f64"], rtol=TOL)
    assert abs(r["grad_norm_d"] / float(fx["grad_norm_d_f64"]) - 1) <= TOL
    assert abs(r["first"]["loss_disc"] / float(fx["loss_disc_f64"]) - 1) <= TOL
    for k in ("losses_disc_r", "losses_disc_g"):
        np.testing.assert_allclose(r["first"][k], fx[k + "_f64"], rtol=TOL)
    for k in ("loss_gen", "loss_fm"):
        assert abs(r["second"][k] / float(fx[k + "_f64"]) - 1) <= TOL


def test_checkpoint_dict_loads_into_adamw_and_the_discriminator(restated):
    fx, ck, r = restated["b"]
    order = json.load(open(os.path.join(GOLDEN, "disc_step_param_order.json")))["v2"]
    assert [n for n, _ in order] == list(D.discriminator_keys("v2"))
    assert [tuple(s) for _, s in order] == list(D.discriminator_keys("v2").values())
    lr, betas, eps = R.hyper("v2")
    out = D.checkpoint_dict("v2", r["model"], r["state"], int(fx["step"]), lr, betas, eps, 7)
    params = [torch.zeros(s) for _, s in order]
    opt = torch.optim.AdamW(params, lr, betas=betas, eps=eps)
    opt.load_state_dict(out["optimizer"])
    sd = opt.state_dict()
    assert len(sd["state"]) == len(order) and float(sd["state"][0]["step"]) == 1001
    for i in (0, 1, 2, len(order) - 1):
        assert tuple(sd["state"][i]["exp_avg"].shape) == tuple(order[i][1])
    D.check_supported(out["model"], "v2")
    assert list(out["model"]) == list(ck["model"]) and out["iteration"] == 7 and out["learning_rate"] == lr
    assert all(v.dtype == torch.float32 for v in out["model"].values())
    assert D.checkpoint_dict("v2", r["model"], {}, 0, lr, betas, eps, 1)["optimizer"]["state"] == {}


def test_optimizer_state_regenerates_bit_for_bit():
    a = synthetic.discriminator_optimizer_state("v1", 5200)
    b = synthetic.discriminator_optimizer_state("v1", 5200)
    c = synthetic.discriminator_optimizer_state("v1", 5201)
    assert len(a["state"]) == len(D.discriminator_keys("v1"))
    for i, shape in enumerate(D.discriminator_keys("v1").values()):
        for k in ("exp_avg", "exp_avg_sq"):
            assert a["state"][i][k].numpy().tobytes() == b["state"][i][k].numpy().tobytes()
            assert tuple(a["state"][i][k].shape) == shape and a["state"][i][k].dtype == torch.float32
        assert float(a["state"][i]["step"]) == synthetic.OPT_STATE_STEP
        assert bool((a["state"][i]["exp_avg_sq"] > 0).all())
    assert not torch.equal(a["state"][2]["exp_avg"], c["state"][2]["exp_avg"])
    g = a["param_groups"][0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-4, (0.8, 0.99), 1e-9, 0.01, False)


def test_refusals_by_name_without_a_device(tmp_path):
    hps = synthetic.train_config(40000, "v1")["train"]
    ck = synthetic.make_disc_ckpt("v1", 3)
    spectral = {"model": dict(ck["model"])}
    spectral["model"]["discriminators.0.convs.0.weight_orig"] = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        D.DiscriminatorTrainerAMD(spectral, "v1", hps, "cuda")
    with pytest.raises(NotImplementedError, match="fp16_run"):
        D.DiscriminatorTrainerAMD(ck, "v1", dict(hps, fp16_run=True), "cuda")
    with pytest.raises(KeyError, match="betas"):
        D.DiscriminatorTrainerAMD(ck, "v1", {"learning_rate": 1e-4, "eps": 1e-9}, "cuda")
    with pytest.raises(ValueError, match="unequal length"):
        D.check_pairs([(torch.zeros(100), torch.zeros(100)), (torch.zeros(100), torch.zeros(99))])
    with pytest.raises(ValueError, match="at least one"):
        D.check_pairs([])
    from rvc_amd import train_forward as tf
    with pytest.raises(ValueError, match="d_step needs d_checkpoint"):
        tf.evaluate(str(tmp_path), None, d_step=True)
    with pytest.raises(SystemExit):
        tf.main(["--exp", str(tmp_path), "--ckpt", "G_1.pth", "--d-step"])
