"""The discriminator's training step on the device (csrc/disc_backward.hip, rvc_amd.discriminator.DiscriminatorTrainerAMD)
against the f64 restatement tests/disc_step_ref.py and the reference's own f64 run in tests/golden/disc_step_*.npz.

Op level: an n-term f32 dot product is bounded per element by (n + 3) / 2 * 2^-23 * sum |terms| (DESIGN.md §19's bound: n
roundings of the FMA chain and three more for the LeakyReLU factor, the scale and the accumulate); nothing measured goes
into it.  End to end the bounds are 4 x the device's figures of profiles/disc_step_prec.txt."""
import os

import numpy as np
import pytest
import torch

import disc_step_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOPE32 = float(np.float32(0.1))  # the slope the kernels multiply by
DEV = "cuda"


def ops():
    from rvc_amd import ops as o
    return o


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def bound(n, mag):
    return (n + 3) / 2 * 2.0 ** -23 * mag + 1e-37


def twice(fn):
    """Run fn twice: the results are bit-equal (fixed order, no atomics); returns the first."""
    a = fn()
    b = fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(x, y)
    return a


def check_layer(rng, B, Ci, Co, K, stride, pad, groups, Lin, act=True, data=True):
    """conv_bwd_data and conv_bwd_weight of one layer shape against the restatement, each element within its bound."""
    o = ops()
    Lout = (Lin + 2 * pad - K) // stride + 1
    dy, y, x = rnd(rng, B, Co, Lout), rnd(rng, B, Co, Lout), rnd(rng, B, Ci, Lin)
    w = rnd(rng, Co, Ci // groups, K)
    yd = y.to(DEV) if act else None
    yr = y if act else None
    if data:
        got = twice(lambda: o.conv_bwd_data(dy.to(DEV), yd, w.to(DEV), Lin, stride, pad, groups, SLOPE32))
        want, mag = R.conv_bwd_data(dy, yr, w, Lin, stride, pad, groups, SLOPE32)
        assert got.shape == want.shape
        err = (got.cpu().double() - want).abs()
        n = (Co // groups) * -(-K // stride)
        assert bool((err <= bound(n, mag)).all()), (float(err.max()), float(bound(n, mag).max()))

    def weight():
        dW = torch.full((Co, Ci // groups, K), 7.0, device=DEV)  # stale values: a plain call overwrites them
        db = torch.full((Co,), 7.0, device=DEV)
        return o.conv_bwd_weight(dy.to(DEV), yd, x.to(DEV), dW, db, stride, pad, groups, SLOPE32)
    dW, db = twice(weight)
    wW, wb, mW, mb = R.conv_bwd_weight(dy, yr, x, K, stride, pad, groups, SLOPE32)
    n = B * Lout
    errW, errb = (dW.cpu().double() - wW).abs(), (db.cpu().double() - wb).abs()
    assert bool((errW <= bound(n, mW)).all()), (float(errW.max()), float(bound(n, mW).max()))
    assert bool((errb <= bound(n, mb)).all()), (float(errb.max()), float(bound(n, mb).max()))


# ---------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("B", [4, 74])
@pytest.mark.parametrize("ch", [(32, 128), (128, 512)])
def test_stride3_k5_every_tail(B, ch):
    """DiscriminatorP's convs: all three tail residues of Lin = 3 Lout - 2 + r, and windows of one real tap."""
    rng = np.random.default_rng(100 + B + ch[0])
    for Lin in (1, 2, 3, 4, 9, 10, 11):
        check_layer(rng, B, ch[0], ch[1], 5, 3, 2, 1, Lin)


def test_stride3_k5_1024():
    check_layer(np.random.default_rng(7), 74, 1024, 1024, 5, 3, 2, 1, 1)


@pytest.mark.parametrize("ch", [(16, 64, 4), (1024, 1024, 256)])
def test_grouped_k41(ch):
    """DiscriminatorS's grouped convs; 257 and 260 rows cross the 64-output block edge of the forward."""
    rng = np.random.default_rng(200 + ch[2])
    for Lin in (1, 3, 4, 5, 50, 257, 260):
        check_layer(rng, 2, ch[0], ch[1], 41, 4, 20, ch[2], Lin)


def test_dense_stride1_k5():
    """DiscriminatorS.convs.5 (1024 -> 1024, k 5, stride 1) at a width that is no multiple of the tile."""
    check_layer(np.random.default_rng(9), 2, 1024, 1024, 5, 1, 2, 1, 13)


@pytest.mark.parametrize("Lin", [1, 2, 27])
def test_conv_post_no_activation(Lin):
    check_layer(np.random.default_rng(300 + Lin), 4, 1024, 1, 3, 1, 1, 1, Lin, act=False)


@pytest.mark.parametrize("t", [15, 2741])
def test_first_layer_scale_dw(t):
    check_layer(np.random.default_rng(400 + t), 2, 1, 16, 15, 1, 7, 1, t, data=False)


@pytest.mark.parametrize("p,t", [(2, 74), (37, 74), (2, 2741), (37, 2741)])
def test_first_layer_period_dw(p, t):
    """dW of DiscriminatorP.convs.0 from the signal itself: the reflected samples count where the view reads them."""
    o = ops()
    rng = np.random.default_rng(500 + p + t)
    S = 2
    sig = rnd(rng, S, t)
    x = R.period_input(sig, p)  # [S p][1][H]
    H = x.shape[2]
    Lout = (H - 1) // 3 + 1
    assert Lout == o.period_front_rows(t, p)
    dy, y = rnd(rng, S * p, 32, Lout), rnd(rng, S * p, 32, Lout)

    def run():
        dW, db = torch.empty(32, 1, 5, device=DEV), torch.empty(32, device=DEV)
        return o.conv_bwd_weight(dy.to(DEV), y.to(DEV), sig.to(DEV), dW, db, 3, 2, 1, SLOPE32, period=p)
    dW, db = twice(run)
    wW, wb, mW, mb = R.conv_bwd_weight(dy, y, x, 5, 3, 2, 1, SLOPE32)
    n = S * p * Lout
    assert bool(((dW.cpu().double() - wW).abs() <= bound(n, mW)).all())
    assert bool(((db.cpu().double() - wb).abs() <= bound(n, mb)).all())


def test_fused_leaky_relu_factor_is_the_mask_product():
    """A stored output with exact zeros and negative values: taking the factor on load equals multiplying first."""
    o = ops()
    rng = np.random.default_rng(11)
    B, Ci, Co, Lin = 4, 32, 128, 10
    Lout = 4
    dy, x, w = rnd(rng, B, Co, Lout).to(DEV), rnd(rng, B, Ci, Lin).to(DEV), rnd(rng, Co, Ci, 5).to(DEV)
    y = rnd(rng, B, Co, Lout)
    y[rng.random(y.shape) < 0.3] = 0.0
    y[0, 0, 0] = -0.0
    y = y.to(DEV)
    masked = dy * torch.where(y > 0, torch.tensor(1.0, device=DEV), torch.tensor(SLOPE32, device=DEV))
    assert torch.equal(o.conv_bwd_data(dy, y, w, Lin, 3, 2, 1, SLOPE32), o.conv_bwd_data(masked, None, w, Lin, 3, 2, 1))
    a = o.conv_bwd_weight(dy, y, x, torch.empty(Co, Ci, 5, device=DEV), torch.empty(Co, device=DEV), 3, 2, 1, SLOPE32)
    b = o.conv_bwd_weight(masked, None, x, torch.empty(Co, Ci, 5, device=DEV), torch.empty(Co, device=DEV), 3, 2, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for groups, Cg, Lg in ((4, 16, 50),):  # the direct forms
        dyg, yg = rnd(rng, 2, 64, 13).to(DEV), rnd(rng, 2, 64, 13)
        yg[rng.random(yg.shape) < 0.3] = 0.0
        yg = yg.to(DEV)
        wg, xg = rnd(rng, 64, 4, 41).to(DEV), rnd(rng, 2, Cg, Lg).to(DEV)
        mg = dyg * torch.where(yg > 0, torch.tensor(1.0, device=DEV), torch.tensor(SLOPE32, device=DEV))
        assert torch.equal(o.conv_bwd_data(dyg, yg, wg, Lg, 4, 20, groups, SLOPE32),
                           o.conv_bwd_data(mg, None, wg, Lg, 4, 20, groups))
        a = o.conv_bwd_weight(dyg, yg, xg, torch.empty(64, 4, 41, device=DEV), torch.empty(64, device=DEV), 4, 20, groups,
                              SLOPE32)
        b = o.conv_bwd_weight(mg, None, xg, torch.empty(64, 4, 41, device=DEV), torch.empty(64, device=DEV), 4, 20, groups)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(32, 128, 5, 3, 2, 1, 10), (16, 64, 41, 4, 20, 4, 50)])
def test_accumulate_two_halves_is_the_batch(shape):
    """Two calls at scale 1/2, the second accumulating, against the restated batch of 2 at scale 1/2."""
    o = ops()
    Ci, Co, K, stride, pad, groups, Lin = shape
    rng = np.random.default_rng(12 + K)
    B = 6
    Lout = (Lin + 2 * pad - K) // stride + 1
    dy, y, x = rnd(rng, B, Co, Lout), rnd(rng, B, Co, Lout), rnd(rng, B, Ci, Lin)
    dW, db = torch.empty(Co, Ci // groups, K, device=DEV), torch.empty(Co, device=DEV)
    h = B // 2
    for i, sl in enumerate((slice(0, h), slice(h, B))):
        o.conv_bwd_weight(dy[sl].contiguous().to(DEV), y[sl].contiguous().to(DEV), x[sl].contiguous().to(DEV), dW, db,
                          stride, pad, groups, SLOPE32, scale=0.5, accumulate=i > 0)
    wW, wb, mW, mb = R.conv_bwd_weight(dy, y, x, K, stride, pad, groups, SLOPE32, scale=0.5)
    n = B * Lout
    assert bool(((dW.cpu().double() - wW).abs() <= bound(n, mW)).all())
    assert bool(((db.cpu().double() - wb).abs() <= bound(n, mb)).all())


def test_lsgan_grad():
    o = ops()
    rng = np.random.default_rng(13)
    for n in (1, 37, 1000):
        d = rnd(rng, 2 * n, 1, 1)
        got = twice(lambda: o.lsgan_grad(d.to(DEV), 0.5)).cpu().double().reshape(-1)
        g_r, g_g = R.lsgan_grad(d[:n], d[n:], 0.5)
        want = torch.cat([g_r, g_g]).reshape(-1)
        assert bool(((got - want).abs() <= 2.0 ** -24 * want.abs() + 1e-45).all())  # one rounding of the f64 value


def ulps(got, want64):
    """|got - want| in units of the f32 spacing at want."""
    w32 = want64.numpy().astype(np.float32)
    return np.abs(got.numpy().astype(np.float64) - want64.numpy()) / np.spacing(np.abs(w32)).astype(np.float64)


@pytest.mark.parametrize("warm", [True, False])
def test_wn_adamw(warm):
    """Given the same f32 gradients: every parameter and moment within 2 ulp of the f64 restatement rounded to f32, the
    squared norms to 1e-12; with zero state the update is lr * sign(grad) whatever the gradient's size."""
    o = ops()
    rng = np.random.default_rng(14 + warm)
    Co, shape = 37, (37, 12, 5)
    lr, betas, eps, step = 1e-4, (0.8, 0.99), 1e-9, 1001 if warm else 1
    dW = rnd(rng, *shape) * torch.from_numpy(10.0 ** rng.uniform(-3, 1, (Co, 1, 1)).astype(np.float32))
    db, v, g, b = rnd(rng, Co) * 0.1, rnd(rng, *shape) * 0.05, rnd(rng, Co).abs() + 0.5, rnd(rng, Co) * 0.02
    if warm:
        mom = [rnd(rng, *s) * 0.05 if i % 2 == 0 else rnd(rng, *s).abs() * 0.0025
               for i, s in enumerate((shape, shape, (Co,), (Co,), (Co,), (Co,)))]
    else:
        mom = [torch.zeros(s) for s in (shape, shape, (Co,), (Co,), (Co,), (Co,))]

    def run():
        st = tuple(m.clone().to(DEV) for m in mom)
        p = (v.clone().to(DEV), g.clone().to(DEV), b.clone().to(DEV))
        table = torch.zeros(3 * Co, device=DEV, dtype=torch.float64)
        o.wn_adamw(dW.to(DEV), db.to(DEV), p[0], p[1], p[2], st, table, lr, betas, eps, R.WEIGHT_DECAY, step)
        return p + st + (table, o.grad_norm(table))
    out = twice(run)
    dg, dv = R.weight_norm_bwd(dW, v, g)
    want = [R.adamw(v, dv, mom[0], mom[1], step, lr, betas, eps), R.adamw(g, dg, mom[2], mom[3], step, lr, betas, eps),
            R.adamw(b, db, mom[4], mom[5], step, lr, betas, eps)]
    got = {"v": (out[0], out[3], out[4]), "g": (out[1], out[5], out[6]), "b": (out[2], out[7], out[8])}
    for (name, triple), w in zip(got.items(), want):
        for what, a, e in zip(("p", "exp_avg", "exp_avg_sq"), triple, w):
            u = ulps(a.cpu().reshape(-1), e.reshape(-1))
            assert u.max() <= 2, (name, what, float(u.max()))
    if not warm:  # m / sqrt(s) = (1 - b1) grad / sqrt((1 - b2) grad^2), the bias corrections cancel it to sign(grad)
        moved = out[0].cpu().double() - v.double() * (1 - lr * R.WEIGHT_DECAY)
        big = dv.abs() > 1e-3  # below that eps = 1e-9 shows: the step is lr |g| / (|g| + eps)
        assert int(big.sum()) > big.numel() // 2
        assert bool(((moved + lr * torch.sign(dv)).abs()[big] <= 1e-5 * lr + np.spacing(np.float32(0.25))).all())
    total = float(dg.pow(2).sum() + dv.pow(2).sum() + R.d64(db).pow(2).sum())
    assert abs(float(out[9].sum().cpu()) / total - 1) <= 1e-12
    assert abs(float(out[10].cpu()) / R.grad_norm([dg, dv, db]) - 1) <= 1e-12


# ---------------------------------------------------------------------------------------------- end to end
# 4 x the device's figures of profiles/disc_step_prec.txt, per case; see DESIGN.md §20
BOUNDS = {
    "a": {"grad": 4 * 4.416e-04, "grad_max": 4 * 1.473e-04, "grad_norm_d": 4 * 1.013e-07, "grad_norms": 4 * 5.909e-05, "loss_disc": 4 * 1.518e-07, "loss_fm": 4 * 3.047e-07, "loss_gen": 4 * 3.201e-07, "losses_disc_g": 4 * 8.180e-07, "losses_disc_r": 4 * 1.010e-06, "post": 4 * 1.886e-02},
    "b": {"grad": 4 * 3.339e-06, "grad_max": 4 * 5.942e-06, "grad_norm_d": 4 * 1.924e-07, "grad_norms": 4 * 1.037e-06, "loss_disc": 4 * 8.959e-08, "loss_fm": 4 * 3.143e-07, "loss_gen": 4 * 2.119e-07, "losses_disc_g": 4 * 4.075e-06, "losses_disc_r": 4 * 3.377e-07, "post": 4 * 4.110e-05},
    "c": {"grad": 4 * 1.632e-06, "grad_max": 4 * 7.354e-06, "grad_norm_d": 4 * 1.071e-07, "grad_norms": 4 * 1.632e-06, "loss_disc": 4 * 1.029e-07, "loss_fm": 4 * 4.576e-08, "loss_gen": 4 * 1.155e-07, "losses_disc_g": 4 * 6.602e-07, "losses_disc_r": 4 * 8.831e-07},
}


@pytest.fixture(scope="module")
def trainers():
    """One trainer per version, rebuilt from the fixture's checkpoint by ``restore`` of its first snapshot."""
    cache = {}

    def get(fx):
        from rvc_amd import synthetic
        from rvc_amd.discriminator import DiscriminatorTrainerAMD
        key = (str(fx["version"]), int(fx["warm"]))
        if key not in cache:
            hps = synthetic.train_config(40000, key[0])["train"]
            tr = DiscriminatorTrainerAMD(R.fixture_ckpt(fx), key[0], hps, DEV)
            cache[key] = (tr, tr.snapshot())
        tr, snap = cache[key]
        tr.restore(snap)
        return tr
    return get


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_step_matches_reference_f64(case, trainers):
    fx = np.load(os.path.join(GOLDEN, f"disc_step_{case}.npz"))
    figures = R.compare(trainers(fx), fx, DEV)
    for k, v in figures.items():
        print(f"{case} {k}: {v:.3e}")
    assert case in BOUNDS, "no measured bounds for this case yet (scripts/disc_step_prec.py)"
    for k, limit in BOUNDS[case].items():
        assert figures[k] <= limit, (k, figures[k], limit)


def test_step_restore_and_save_round_trip(trainers, tmp_path):
    from rvc_amd.discriminator import DiscriminatorAMD
    fx = np.load(os.path.join(GOLDEN, "disc_step_b.npz"))
    tr = trainers(fx)
    y, y_hat = torch.from_numpy(fx["y"][0]).to(DEV), torch.from_numpy(fx["y_hat"][0]).to(DEV)
    before = tr.losses(y, y_hat)
    snap = tr.snapshot()
    tr.step([(y, y_hat)])
    stepped = tr.losses(y, y_hat)
    assert stepped != before
    path = str(tmp_path / "D_2.pth")
    tr.save(path, 2)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["iteration"] == 2 and ck["optimizer"]["state"][0]["step"] == 1001
    assert DiscriminatorAMD(ck, "v2", DEV).losses(y, y_hat) == stepped
    tr.restore(snap)
    assert tr.losses(y, y_hat) == before
    assert tr.step_count == 1000


def test_evaluate_d_step(tmp_path):
    """The scorer with the D step: loss_disc is the plain run's, loss_gen / loss_fm are those of a trainer stepped by
    hand on the same pair, and an utterance's line does not depend on the utterances before it."""
    import json
    from rvc_amd import synthetic
    from rvc_amd import train_forward as tf
    from rvc_amd.discriminator import DiscriminatorTrainerAMD
    exp = str(tmp_path / "exp")
    g_path = synthetic.write_train_experiment(exp, 32000, "v1", frames=(44, 50), seed=78, with_d=True)
    hps = json.load(open(os.path.join(exp, "config.json")))
    model = tf.TrainSynthAMD(torch.load(g_path, map_location="cpu", weights_only=False), hps, DEV)
    d_ck = torch.load(os.path.join(exp, "D_1.pth"), map_location="cpu", weights_only=False)
    tr = DiscriminatorTrainerAMD(d_ck, "v1", hps["train"], DEV)
    plain = tf.evaluate(exp, model, d_checkpoint=tr)
    again = tf.evaluate(exp, model, d_checkpoint=tr)
    stepped = tf.evaluate(exp, model, d_checkpoint=tr, d_step=True)
    assert tf.evaluate(exp, model, d_checkpoint=tr) == plain == again  # D was put back
    assert stepped["scored"] == 2
    for u, v in zip(plain["utterances"], stepped["utterances"]):
        assert v["loss_disc"] == u["loss_disc"] and v["losses_disc_r"] == u["losses_disc_r"]
        assert v["loss_mel"] == u["loss_mel"] and v["loss_kl"] == u["loss_kl"]
        assert v["loss_gen"] != u["loss_gen"] and v["grad_norm_d"] > 0
    # by hand: the second utterance's pair, a step, then the losses
    rows = tf.read_filelist(os.path.join(exp, "filelist.txt"))
    wav, phone_p, pitch_p, pitchf_p, sid = rows[1]
    spec = tf._spec_of(wav, hps, DEV)
    phone, pitch, pitchf, T = tf.trim_labels(np.load(phone_p), np.load(pitch_p), np.load(pitchf_p), spec.shape[-1])
    args = (torch.from_numpy(phone.astype(np.float32)).to(DEV), torch.from_numpy(pitch.astype(np.int64)).to(DEV),
            torch.from_numpy(pitchf.astype(np.float32)).to(DEV), spec[:, :T].contiguous())
    y_hat, ids, _ = model.forward(*args, tf.parse_sid(sid), seed=1)
    st = int(ids.item()) * model.hop
    wave = tf._wave_of(wav, DEV).reshape(-1)[st:st + y_hat.numel()].float().contiguous()
    snap = tr.snapshot()
    first = tr.step([(wave, y_hat)])
    hand = tr.losses(wave, y_hat)
    tr.restore(snap)
    v = stepped["utterances"][1]
    assert (v["loss_gen"], v["loss_fm"], v["grad_norm_d"]) == (hand["loss_gen"], hand["loss_fm"], first["grad_norm_d"])
    # the second utterance alone: the first dropped from the filelist, its seed kept
    with open(os.path.join(exp, "filelist.txt"), "w", encoding="utf-8") as f:
        f.write("|".join(rows[1]) + "\n")
    alone = tf.evaluate(exp, model, seed=1, d_checkpoint=tr, d_step=True)["utterances"][0]
    assert {k: x for k, x in alone.items() if k != "index"} == {k: x for k, x in v.items() if k != "index"}
