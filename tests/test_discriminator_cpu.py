"""The discriminator's host side (rvc_amd/discriminator.py, synthetic.py, train_forward.py's aggregation) and the f64
restatements of tests/discriminator_ref.py, pinned to the reference's own modules through the fixtures of
tests/golden/make_golden_discriminator.py.  No device."""
import json
import os

import numpy as np
import pytest
import torch

import discriminator_ref as ref
from rvc_amd import discriminator as dsc
from rvc_amd import synthetic, train_forward as tf
from rvc_amd.synth import fold_weight_norm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def state_dicts():
    return {v: synthetic.discriminator_state_dict(v, 5103) for v in ("v1", "v2")}


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_keys_are_the_reference_modules_own(version, state_dicts):
    with open(os.path.join(GOLDEN, "discriminator_keys.json")) as f:
        table = json.load(f)[version]
    keys = dsc.discriminator_keys(version)
    assert {k: list(s) for k, s in keys.items()} == table
    sd = state_dicts[version]
    assert list(sd) == list(keys)  # the same keys in the same order
    assert all(tuple(sd[k].shape) == s and sd[k].dtype == torch.float32 for k, s in keys.items())
    assert len(dsc.PERIODS[version]) == {"v1": 6, "v2": 8}[version]


def test_synthetic_weights_regenerate_and_are_drawn_not_derived(state_dicts):
    sd = state_dicts["v1"]
    again = synthetic.discriminator_state_dict("v1", 5103)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    other = synthetic.discriminator_state_dict("v1", 5104)
    assert not torch.equal(sd["discriminators.3.convs.2.weight_v"], other["discriminators.3.convs.2.weight_v"])
    # weight_g = gain * U(0.7, 1.3): inside the gain's band, and not ||v|| times anything exact
    g = sd["discriminators.3.convs.2.weight_g"].reshape(-1).double() / np.sqrt(2.0)
    assert 0.7 <= float(g.min()) and float(g.max()) <= 1.3 + 1e-6
    assert synthetic.make_disc_ckpt("v1", 5103)["model"].keys() == sd.keys()


def test_fold_of_4d_weights_is_g_v_over_norm(state_dicts):
    sd = state_dicts["v1"]
    names = ["discriminators.1.convs.0", "discriminators.4.convs.2", "discriminators.6.conv_post",
             "discriminators.0.convs.3"]
    W = fold_weight_norm({f"{n}.{s}": sd[f"{n}.{s}"] for n in names for s in ("bias", "weight_g", "weight_v")})
    for n in names:
        v, g = sd[n + ".weight_v"].double(), sd[n + ".weight_g"].double()
        want = g * v / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
        got = W[n + ".weight"]
        assert got.shape == v.shape and got.dtype == torch.float32
        # an f32 norm over fan_in terms and two roundings: a few 2^-24, relative to the weight's row scale
        assert float((got.double() - want).abs().max() / want.abs().max()) < 2e-6
        assert torch.equal(W[n + ".bias"], sd[n + ".bias"])


@pytest.mark.parametrize("t", [38, 74, 75, 2741])
def test_period_index_map_is_reflect_pad_and_view(t):
    y = np.random.default_rng(t).standard_normal(t).astype(np.float32)
    for p in dsc.PERIODS["v2"]:
        idx = ref.period_index(t, p)
        want = ref.period_view_torch(y, p).numpy()
        assert idx.shape == want.shape and idx.min() >= 0 and idx.max() < t
        assert np.array_equal(y[idx], want)
        assert idx.shape[0] * p == t + (p - t % p) % p
    assert ref.period_index(38, 37).shape == (2, 37) and ref.period_index(74, 37).shape == (2, 37)


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_loss_formulas_reproduce_the_fixtures_f64_losses(name, golden):
    fx = golden(f"discriminator_{name}")
    yr, yg = ref.split(fx["y_d_r_f64"], fx["y_d_sizes"]), ref.split(fx["y_d_g_f64"], fx["y_d_sizes"])
    disc_r = [np.mean((1 - v) ** 2) for v in yr]
    disc_g = [np.mean(v ** 2) for v in yg]
    gen = [np.mean((1 - v) ** 2) for v in yg]
    got = ref.losses_from_terms(fx["fm_l1_f64"], disc_r, disc_g, gen)
    for k in ref.SCALARS:
        assert abs(got[k] / float(fx[k + "_f64"]) - 1) <= 1e-12, k
    for k, v in (("losses_disc_r", disc_r), ("losses_disc_g", disc_g), ("losses_gen", gen)):
        assert np.abs(np.array(v) / fx[k + "_f64"] - 1).max() <= 1e-12, k
    n_disc = len(dsc.PERIODS[ref.CASES[name]]) + 1
    assert len(yr) == n_disc and fx["fm_l1_f64"].size == 7 + 6 * (n_disc - 1)
    # the f32 restatement of the finish kernel lands within f32 rounding of the same numbers
    f32 = ref.finish_f32(fx["fm_l1_f64"], disc_r, disc_g, gen)
    for k in ref.SCALARS:
        assert abs(f32[k] / float(fx[k + "_f64"]) - 1) <= (fx["fm_l1_f64"].size + 2) * 2.0 ** -24, k


def test_aggregate_gan_arithmetic():
    utts = [{"frames": 40, "loss_mel": 30.0, "loss_kl": 2.0, "loss_disc": 20.0, "loss_gen": 16.0, "loss_fm": 6.0},
            {"frames": 60, "loss_mel": 36.0, "loss_kl": 1.0, "loss_disc": 22.0, "loss_gen": 15.0, "loss_fm": 8.0}]
    base, gan = tf.aggregate(utts), tf.aggregate_gan(utts)
    assert base == {"loss_mel": 33.0, "loss_kl": (2.0 * 40 + 1.0 * 60) / 100}
    assert gan["loss_disc"] == 21.0 and gan["loss_gen"] == 15.5 and gan["loss_fm"] == 7.0
    assert gan["loss_gen_all"] == 15.5 + 7.0 + 33.0 + base["loss_kl"]
    assert tf.aggregate_gan([]) == {"loss_disc": None, "loss_gen": None, "loss_fm": None, "loss_gen_all": None}


def test_refusals_by_name(state_dicts):
    sd = dict(state_dicts["v1"])
    dsc.check_supported(sd, "v1")
    with pytest.raises(ValueError, match="6 period discriminators.*'v2' has 8"):
        dsc.check_supported(sd, "v2")
    with pytest.raises(ValueError, match="8 period discriminators.*'v1' has 6"):
        dsc.check_supported(state_dicts["v2"], "v1")
    sn = {k.replace("weight_v", "weight_orig").replace("weight_g", "weight_u"): v for k, v in sd.items()}
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        dsc.check_supported(sn, "v1")
    with pytest.raises(NotImplementedError, match="spectral-norm"):
        dsc.DiscriminatorAMD({"model": sn}, "v1", device="cpu")  # refused before anything is uploaded
    short = {k: v for k, v in sd.items() if k != "discriminators.2.conv_post.bias"}
    with pytest.raises(KeyError, match="discriminators.2.conv_post.bias"):
        dsc.check_supported(short, "v1")
    with pytest.raises(ValueError, match="'v3'"):
        dsc.discriminator_keys("v3")


def test_write_train_experiment_d_checkpoint_is_off_by_default(tmp_path):
    g = synthetic.write_train_experiment(str(tmp_path / "plain"), 32000, "v1", frames=(40,), seed=5)
    assert os.path.basename(g) == "G_1.pth" and not os.path.exists(tmp_path / "plain" / "D_1.pth")
    synthetic.write_train_experiment(str(tmp_path / "gan"), 32000, "v1", frames=(40,), seed=5, with_d=True)
    d = torch.load(tmp_path / "gan" / "D_1.pth", map_location="cpu", weights_only=False)
    assert list(d["model"]) == list(dsc.discriminator_keys("v1")) and d["iteration"] == 1


def test_cli_refuses_unpaired_d_checkpoints():
    with pytest.raises(SystemExit):
        tf.main(["--exp", "x", "--ckpt", "G_1.pth", "--ckpt", "G_2.pth", "--d-ckpt", "D_1.pth"])
