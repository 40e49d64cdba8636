"""The discriminator and the GAN losses on the device (csrc/discriminator.hip, rvc_amd/discriminator.py, the additions
to rvc_amd/train_forward.py): the new ops against torch CPU f64 (tests/discriminator_ref.py), the whole model on the
three fixtures of the reference's own f64 run, and the checkpoint scorer with a D beside the G."""
import json
import os

import numpy as np
import pytest
import torch

import discriminator_ref as ref
from rvc_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
# U below is the f32 unit roundoff 2^-24; the bounds are stated in 2^-23 = 2 U


def _mods():
    from rvc_amd import discriminator, ops, train_forward
    return ops, discriminator, train_forward


def _within(got, want, mag, mult):
    """|got - want| <= mult * 2^-23 * (sum of |terms| behind the output), element by element."""
    got, want, mag = got.double().cpu().numpy(), want.numpy(), mag.numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / (2.0 ** -23 * np.maximum(mag, 1e-300))
    assert ratio.max() <= mult, float(ratio.max())


# ---------------------------------------------------------------------------------------------- ops
# A sum of n products accumulated by n FMAs in any fixed order is off by at most n U sum|terms| to first order
# (Higham, Accuracy and Stability, §3.1); the bias add and the LeakyReLU product are two more roundings, and the
# kernels' slope 0.1f differs from the f64 restatement's 0.1 by 2^-26 < U: (n + 3) U = (n + 3) / 2 * 2^-23.
def _direct_mult(n_terms):
    return (n_terms + 3) / 2.0


@pytest.mark.parametrize("p", [2, 37])
@pytest.mark.parametrize("t", [38, 74, 75])
def test_period_front_op(p, t):
    """Two signals at once; p = 37 pads 36 onto 38 samples (the largest pad there is), nothing onto 74, 36 onto 75;
    at p = 37, t = 38 and 74 the view has two rows and H1 = 1."""
    ops, dsc, _ = _mods()
    rng = np.random.default_rng(100 * p + t)
    y = (rng.standard_normal((2, t)) * 0.3).astype(np.float32)
    w = (rng.standard_normal((32, 5)) * 0.8).astype(np.float32)
    b = (rng.standard_normal(32) * 0.05).astype(np.float32)
    got = ops.period_front(torch.from_numpy(y).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), p)
    H = (t + (p - t % p) % p) // p
    H1 = (H - 1) // 3 + 1
    assert got.shape == (2 * p, 32, H1) and ops.period_front_rows(t, p) == H1
    if p == 37 and t < 75:
        assert H1 == 1
    for s in range(2):
        want, mag = ref.period_front(y[s], w, b, p)
        _within(dsc.reference_order(got[s * p:(s + 1) * p], p), want, mag, _direct_mult(5))
    with pytest.raises(ValueError, match="reflect pad"):
        ops.period_front_rows(17, 37)  # a pad of 20 on 17 samples


GCONV = [(16, 64, 4), (64, 256, 16), (256, 1024, 64), (1024, 1024, 256)]


@pytest.mark.parametrize("Ci,Co,groups", GCONV)
def test_gconv_small_op(Ci, Co, groups):
    """Lin = 1: a window that is all padding but one tap; 41: one kernel width; 163 and 1001: Lout = 41 and 251, the
    stride's two remainders with a last 64-wide tile that is part full, over one and four tiles."""
    ops, _, _ = _mods()
    rng = np.random.default_rng(Ci + Co)
    w = (rng.standard_normal((Co, 4, 41)) / np.sqrt(164.0)).astype(np.float32)
    b = (rng.standard_normal(Co) * 0.05).astype(np.float32)
    wd, bd = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    for Lin in (1, 41, 163, 1001):
        x = rng.standard_normal((2, Ci, Lin)).astype(np.float32)
        got = ops.gconv_small(torch.from_numpy(x).to(DEV), wd, bd)
        want, mag = ref.gconv(x, w, b, groups)
        assert got.shape == (2, Co, (Lin - 1) // 4 + 1)
        _within(got, want, mag, _direct_mult(164))
    with pytest.raises(ValueError, match="not one of its layers"):
        ops.gconv_small(torch.zeros(1, Ci, 8, device=DEV), wd[:Co // 2].contiguous(), bd[:Co // 2])


def test_strided_batched_conv_of_a_period_layer():
    """128 -> 512, k = 5, stride 3, padding 2 at B = 3, H = 10 on the conv engine, as DiscriminatorAMD calls it.  The
    split-operand engine takes strides 1 and 2 only, so a stride-3 conv runs on the f32 MFMA engine: exact f32 FMA
    chains in the engine's own order over the n = 640 products, and the bound of the direct kernels holds for any
    order of summation."""
    ops, dsc, _ = _mods()
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((512, 128, 5)) / np.sqrt(640.0)).astype(np.float32)
    b = (rng.standard_normal(512) * 0.05).astype(np.float32)
    x = rng.standard_normal((3, 128, 10)).astype(np.float32)
    conv = ops.Conv(torch.from_numpy(w), torch.from_numpy(b), device=DEV)
    got = dsc.DiscriminatorAMD._conv(conv, torch.from_numpy(x).to(DEV), 3, 2)
    want, mag = ref.conv(x, w, b, 3, 2)
    assert got.shape == (3, 512, 4) and ops.LAST_CONV_ENGINE == 0
    _within(got, want, mag, _direct_mult(640))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_loss_reductions_and_their_fixed_order(n):
    """rvc_pair_l1 and rvc_lsgan_terms: f64 sums kept in f64, so well inside one f32 rounding of NumPy's f64 mean, and
    the same bits from run to run."""
    ops, _, _ = _mods()
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    tables = []
    for _ in range(2):
        table = ops.disc_table(2, 1, DEV)
        ops.pair_l1(ad, bd, table, 1)
        ops.lsgan_terms(ad, bd, table, 2)
        tables.append(table.cpu())
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = [0.0, np.abs(a64 - b64).mean(), ((1 - a64) ** 2).mean(), (b64 ** 2).mean(), ((1 - b64) ** 2).mean()]
    got = tables[0].numpy()
    assert got[0] == 0.0
    assert np.abs(got[1:] / np.array(want[1:]) - 1).max() <= 2.0 ** -23
    assert torch.equal(tables[0], tables[1])
    with pytest.raises(ValueError, match="slot"):
        ops.pair_l1(ad, bd, table, 5)
    with pytest.raises(ValueError, match="slots"):
        ops.lsgan_terms(ad, bd, table, 3)


def test_disc_finish_sums_in_f32_in_the_reference_order():
    ops, _, _ = _mods()
    rng = np.random.default_rng(3)
    n_fm, n_disc = 43, 7
    terms = rng.uniform(0.01, 3.0, n_fm + 3 * n_disc)
    table = torch.from_numpy(terms).to(DEV)
    ls = terms[n_fm:].reshape(n_disc, 3)
    l1, kl = np.float32(0.71234), np.float32(1.93817)
    want = ref.finish_f32(terms[:n_fm], ls[:, 0], ls[:, 1], ls[:, 2], l1, 45.0, kl, 1.0)
    got = ops.disc_finish(table, n_fm, n_disc, torch.tensor([l1], device=DEV), 45.0, torch.tensor([kl], device=DEV),
                          1.0).cpu().numpy()
    names = ("loss_disc", "loss_gen", "loss_fm", "loss_gen_all", "loss_mel", "loss_kl")
    assert {k: float(v) for k, v in zip(names, got)} == want  # bit for bit
    assert np.array_equal(got[6:], np.concatenate([ls[:, 2], ls[:, 0], ls[:, 1]]).astype(np.float32))
    bare = ops.disc_finish(table, n_fm, n_disc).cpu().numpy()
    assert np.array_equal(bare[:3], got[:3]) and np.isnan(bare[3:6]).all()
    with pytest.raises(ValueError, match="go together"):
        ops.disc_finish(table, n_fm, n_disc, l1=torch.zeros(1, device=DEV))


# ---------------------------------------------------------------------------------------------- the whole model
# profiles/discriminator_prec.txt (scripts/discriminator_prec.py on the MI355X): the device's deviation from the
# reference's f64 run per quantity -- (relative figure, max abs figure) as discriminator_ref.compare defines them, the
# largest of the three fixtures.  Each bound is 4 x the figure (room for the conv engine's split-K and tile order,
# which reorder sums), a relative figure never above the project's standing parity of 1e-4.
MEASURED = {
    "y_d_r": (2.259e-06, 4.294e-06), "y_d_g": (2.670e-06, 3.556e-06), "fm_sample_r": (2.259e-06, 6.325e-06),
    "fm_sample_g": (2.670e-06, 5.037e-06), "fm_rms_r": (7.623e-07, 0.0), "fm_rms_g": (9.769e-07, 0.0),
    "fm_l1": (1.075e-05, 0.0), "loss_disc": (1.566e-07, 0.0), "loss_gen": (2.579e-07, 0.0),
    "loss_fm": (3.111e-07, 0.0), "losses_gen": (9.368e-07, 0.0), "losses_disc_r": (8.831e-07, 0.0),
    "losses_disc_g": (4.075e-06, 0.0),
}
PARITY = 1e-4
_DISCS = {}


def _disc(fx):
    _, dsc, _ = _mods()
    key = (str(fx["version"]), int(fx["seed"]))
    if key not in _DISCS:
        _DISCS[key] = dsc.DiscriminatorAMD(ref.fixture_ckpt(fx), key[0], DEV)
    return _DISCS[key]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_model_against_reference_f64(name, golden):
    fx = golden(f"discriminator_{name}")
    disc = _disc(fx)
    assert disc.n_fm == fx["fm_l1_f64"].size and disc.n_disc == fx["y_d_sizes"].size
    got, losses = ref.compare(disc, fx, DEV)
    failures = []
    for k, (rel, mx) in sorted(got.items()):
        print(f"{name} {k}: rel {rel:.3e} max {mx:.3e}")
        if not (rel <= min(4 * MEASURED[k][0], PARITY) and mx <= 4 * MEASURED[k][1]):
            failures.append((k, rel, mx))
    assert set(got) == set(MEASURED)
    assert not failures, failures
    # the same bits from run to run, and nothing but the GAN losses without the generator's two
    y, y_hat = torch.from_numpy(fx["y"]).to(DEV), torch.from_numpy(fx["y_hat"]).to(DEV)
    assert disc.losses(y, y_hat) == losses
    assert set(losses) == {"loss_disc", "loss_gen", "loss_fm", "losses_gen", "losses_disc_r", "losses_disc_g"}


def test_model_refuses_what_it_cannot_pad(golden):
    disc = _disc(golden("discriminator_c"))
    with pytest.raises(ValueError, match="reflect pad"):
        disc.forward(torch.zeros(17, device=DEV))
    with pytest.raises(ValueError, match="samples"):
        disc.losses(torch.zeros(100, device=DEV), torch.zeros(99, device=DEV))


# ---------------------------------------------------------------------------------------------- the scorer with a D
@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """Two scored utterances (44 and 50 frames against a segment of 40) of a 32k v1 experiment with G_1.pth and
    D_1.pth, and both models built once."""
    _, dsc, tf = _mods()
    exp = str(tmp_path_factory.mktemp("exp32k_d"))
    g_path = synthetic.write_train_experiment(exp, 32000, "v1", frames=(44, 50), seed=78, with_d=True)
    d_path = os.path.join(exp, "D_1.pth")
    hps = json.load(open(os.path.join(exp, "config.json")))
    model = tf.TrainSynthAMD(torch.load(g_path, map_location="cpu", weights_only=False), hps, DEV)
    disc = dsc.DiscriminatorAMD(torch.load(d_path, map_location="cpu", weights_only=False), "v1", DEV)
    return exp, g_path, d_path, hps, model, disc


def _utterance(tf, exp, hps, index):
    wav, pp, cp, fp, sid = tf.read_filelist(os.path.join(exp, "filelist.txt"))[index]
    spec = tf._spec_of(wav, hps, DEV)
    phone, pitch, pitchf, T = tf.trim_labels(np.load(pp), np.load(cp), np.load(fp), spec.shape[-1])
    return (torch.from_numpy(phone).to(DEV), torch.from_numpy(pitch).to(DEV), torch.from_numpy(pitchf).to(DEV),
            spec[:, :T].contiguous()), tf._wave_of(wav, DEV), int(sid)


def test_step_losses_is_the_forward_plus_the_discriminator(experiment):
    _, _, tf = _mods()
    exp, _, _, hps, model, disc = experiment
    args, wave, sid = _utterance(tf, exp, hps, 1)
    got = tf.step_losses(model, disc, *args, wave, sid, hps, seed=11)
    y_hat, ids, (z, z_p, m_p, logs_p, m_q, logs_q) = model.forward(*args, sid, seed=11)
    l1, kl = tf._losses(hps, args[3], y_hat, ids, z_p, logs_q, m_p, logs_p)
    seg, st = hps["train"]["segment_size"], int(ids.item()) * hps["data"]["hop_length"]
    assert y_hat.numel() == seg
    own = disc.losses(wave[st:st + seg].contiguous(), y_hat, l1, kl, hps["train"]["c_mel"], hps["train"]["c_kl"])
    assert got == own  # bit for bit, lists included
    bare = disc.losses(wave[st:st + seg].contiguous(), y_hat)
    assert all(bare[k] == got[k] for k in bare)
    f = np.float32
    assert got["loss_gen_all"] == float(f(f(f(f(got["loss_gen"]) + f(got["loss_fm"])) + f(got["loss_mel"])) +
                                        f(got["loss_kl"])))
    gen = tf.generator_losses(model, *args, sid, hps, seed=11)
    assert (gen["loss_mel"], gen["loss_kl"]) == (got["loss_mel"], got["loss_kl"])
    assert np.isfinite([got[k] for k in ("loss_disc", "loss_gen", "loss_fm", "loss_gen_all")]).all()
    assert len(got["losses_gen"]) == len(got["losses_disc_r"]) == len(got["losses_disc_g"]) == 7


def test_evaluate_with_d_does_not_depend_on_the_limit(experiment):
    _, _, tf = _mods()
    exp, _, _, hps, model, disc = experiment
    two = tf.evaluate(exp, model, limit=2, seed=3, d_checkpoint=disc)
    one = tf.evaluate(exp, model, limit=1, seed=3, d_checkpoint=disc)
    assert two["scored"] == 2 and one["scored"] == 1 and one["utterances"][0] == two["utterances"][0]
    agg, gan = tf.aggregate(two["utterances"]), tf.aggregate_gan(two["utterances"])
    for k in ("loss_disc", "loss_gen", "loss_fm"):
        assert two[k] == sum(u[k] for u in two["utterances"]) / 2 == gan[k]
    assert two["loss_gen_all"] == two["loss_gen"] + two["loss_fm"] + two["loss_mel"] + two["loss_kl"]
    assert (two["loss_mel"], two["loss_kl"]) == (agg["loss_mel"], agg["loss_kl"])
    args, wave, sid = _utterance(tf, exp, hps, 1)
    assert tf.step_losses(model, disc, *args, wave, sid, hps, seed=3 + 1) == \
        {k: v for k, v in two["utterances"][1].items() if k not in ("index", "wav", "frames")}


def test_evaluate_without_d_is_what_it_was(experiment):
    _, _, tf = _mods()
    exp, _, _, hps, model, _ = experiment
    r = tf.evaluate(exp, model, seed=3)
    assert set(r) == {"loss_mel", "loss_kl", "utterances", "scored", "skipped"}
    for u in r["utterances"]:
        assert set(u) == {"index", "wav", "frames", "loss_mel", "loss_kl"}
        args, _, sid = _utterance(tf, exp, hps, u["index"])
        one = tf.generator_losses(model, *args, sid, hps, seed=3 + u["index"])
        assert (one["loss_mel"], one["loss_kl"]) == (u["loss_mel"], u["loss_kl"])
    agg = tf.aggregate(r["utterances"])
    assert (r["loss_mel"], r["loss_kl"]) == (agg["loss_mel"], agg["loss_kl"])


def test_cli_prints_the_new_fields_only_with_d_files(experiment, capsys):
    _, _, tf = _mods()
    exp, g_path, d_path, hps, model, disc = experiment
    tf.main(["--exp", exp, "--ckpt", g_path, "--d-ckpt", d_path, "--limit", "1", "--seed", "3"])
    with_d = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    tf.main(["--exp", exp, "--ckpt", g_path, "--limit", "1", "--seed", "3"])
    without = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(without) == {"checkpoint", "loss_mel", "loss_kl", "scored", "skipped"}
    assert set(with_d) == set(without) | {"d_checkpoint", "loss_disc", "loss_gen", "loss_fm", "loss_gen_all"}
    assert all(with_d[k] == without[k] for k in without)
    want = tf.evaluate(exp, model, limit=1, seed=3, d_checkpoint=disc)
    assert all(with_d[k] == want[k] for k in ("loss_disc", "loss_gen", "loss_fm", "loss_gen_all"))
