"""f64 restatement, without autograd, of the discriminator's training step (main/inference/train.py:851-869): the
gradient of ``discriminator_loss``, Conv1d backward-data and backward-weight with the LeakyReLU factor taken from the
stored output, the backward of ``torch._weight_norm(v, g, 0)``, ``torch.optim.AdamW``'s update and
``clip_grad_value(parameters, None)``.  tests/test_disc_step_cpu.py pins it to the reference's own f64 autograd run in
tests/golden/disc_step_*.npz; tests/test_gpu_disc_step.py and scripts/disc_step_prec.py hold the kernels of
csrc/disc_backward.hip to it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from discriminator_ref import period_view_torch

SLOPE = 0.1
WEIGHT_DECAY = 0.01  # torch.optim.AdamW's default: train.py:766 passes lr, betas and eps only
CASES = {"a": "v2", "b": "v2", "c": "v1"}
SAMPLE = 128


def d64(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double()


# ---------------------------------------------------------------------------------------------- the kernels' formulas
def lsgan_grad(d_r, d_g, scale=1.0):
    """d discriminator_loss / d (d_r, d_g) for one discriminator: means over n values each (train.py:300-301)."""
    d_r, d_g = d64(d_r), d64(d_g)
    n = d_r.numel()
    return -2.0 * (1.0 - d_r) / n * scale, 2.0 * d_g / n * scale


def dyp(dy, y, slope=SLOPE):
    """dy times LeakyReLU's derivative read from the stored output y (0 takes the slope); y None: no activation."""
    dy = d64(dy)
    if y is None:
        return dy
    one = torch.ones((), dtype=torch.float64)
    return dy * torch.where(d64(y) > 0, one, one * slope)


def conv_bwd_data(dy, y, w, Lin, stride, pad, groups=1, slope=SLOPE):
    """dx [B][Ci][Lin] = sum_co sum_k w[co][ci][k] dyp[b][co][j] at i = j stride + k - pad, and the sum of |terms|."""
    g, w = dyp(dy, y, slope), d64(w)
    extra = Lin - ((g.shape[-1] - 1) * stride - 2 * pad + w.shape[-1])
    assert 0 <= extra < stride, extra  # the rows past the last full window: Lin = (Lout - 1) stride - 2 pad + K + extra
    dx = F.conv_transpose1d(g, w, None, stride, pad, extra, groups)
    mag = F.conv_transpose1d(g.abs(), w.abs(), None, stride, pad, extra, groups)
    return dx, mag


def conv_bwd_weight(dy, y, x, K, stride, pad, groups=1, slope=SLOPE, scale=1.0):
    """dW [Co][Ci / groups][K] = scale sum_b sum_j dyp[b][co][j] x[b][ci][j stride + k - pad], db [Co] = scale sum dyp,
    and the sums of |terms| of both."""
    g, x = dyp(dy, y, slope), d64(x)
    B, Co, Lout = g.shape
    Ci = x.shape[1]
    cig, cog = Ci // groups, Co // groups
    xp = F.pad(x, (pad, pad + stride))  # the right side long enough for every strided slice below
    dW = torch.zeros(Co, cig, K, dtype=torch.float64)
    mag = torch.zeros_like(dW)
    gg = g.reshape(B, groups, cog, Lout)
    for k in range(K):
        xs = xp[:, :, k:k + stride * Lout:stride].reshape(B, groups, cig, Lout)
        dW[:, :, k] = torch.einsum("bgoj,bgcj->goc", gg, xs).reshape(Co, cig)
        mag[:, :, k] = torch.einsum("bgoj,bgcj->goc", gg.abs(), xs.abs()).reshape(Co, cig)
    return dW * scale, g.sum((0, 2)) * scale, mag * abs(scale), g.abs().sum((0, 2)) * abs(scale)


def period_input(y, p):
    """DiscriminatorP's view of the signals y [S][t] as a batch of columns [S * p][1][H] (train.py:665-666)."""
    y = d64(y)
    cols = [period_view_torch(sig, p).t() for sig in y]  # [p][H] each
    return torch.cat(cols, 0).unsqueeze(1)


def weight_norm(v, g):
    """torch._weight_norm(v, g, 0) in f64: g v / |v| per output row."""
    v, g = d64(v), d64(g)
    n = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
    return v * (g / n)


def weight_norm_bwd(dW, v, g):
    """(dg, dv) of w = g v / |v| per output row: dg = <dW, v> / |v|, dv = g / |v| (dW - v dg / |v|)."""
    dW, v, g = d64(dW), d64(v), d64(g)
    Co = v.shape[0]
    v2, dW2 = v.reshape(Co, -1), dW.reshape(Co, -1)
    n = v2.norm(dim=1, keepdim=True)
    dg = (dW2 * v2).sum(1, keepdim=True) / n
    dv = g.reshape(Co, 1) / n * (dW2 - v2 * dg / n)
    return dg.reshape(g.shape), dv.reshape(v.shape)


def adamw(p, grad, m, s, step, lr, betas, eps, weight_decay=WEIGHT_DECAY):
    """torch.optim.AdamW (amsgrad False) on one tensor in f64 -> (p, exp_avg, exp_avg_sq) after the ``step``-th update."""
    p, grad, m, s = d64(p), d64(grad), d64(m), d64(s)
    b1, b2 = betas
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * grad
    s = b2 * s + (1.0 - b2) * grad * grad
    step_size = lr / (1.0 - b1 ** step)
    denom = s.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - step_size * m / denom, m, s


def grad_norm(grads):
    """clip_grad_value(parameters, None) (commons.py:48-60): sqrt of the sum of the parameters' squared gradient norms."""
    total = 0.0
    for g in grads:
        total += float(d64(g).pow(2).sum())
    return math.sqrt(total)


# ---------------------------------------------------------------------------------------------- the whole step
def layer_table(version):
    """Per discriminator the convs as (name, stride, pad, groups, activation), in forward order."""
    from rvc_amd.discriminator import PERIODS, P_CHANNELS, P_PAD, P_STRIDE, S_CONVS
    out = [[(f"discriminators.0.convs.{j}", s, pad, g, True) for j, (_, _, _, s, g, pad) in enumerate(S_CONVS)] +
           [("discriminators.0.conv_post", 1, 1, 1, False)]]
    for i in range(1, len(PERIODS[version]) + 1):
        out.append([(f"discriminators.{i}.convs.{j}", P_STRIDE, P_PAD, 1, True) for j in range(len(P_CHANNELS))] +
                   [(f"discriminators.{i}.conv_post", 1, 1, 1, False)])
    return out


def fold(model):
    """The f64 conv weights [Co][Ci / groups][K] and biases of a ``.weight_g`` / ``.weight_v`` state dict."""
    W = {}
    for k in model:
        if k.endswith(".weight_v"):
            base = k[:-len(".weight_v")]
            w = weight_norm(model[k], model[base + ".weight_g"])
            W[base] = (w.reshape(w.shape[0], w.shape[1], w.shape[2]), d64(model[base + ".bias"]))
    return W


def forward(model, version, sigs):
    """Every discriminator on the signals sigs [S][t] in f64 -> per discriminator the layers' inputs and outputs:
    ``xs[d][l]`` [B][Ci][Lin] and ``ys[d][l]`` [B][Co][Lout], B = S for DiscriminatorS and S * p, columns as batch
    elements, for a period."""
    from rvc_amd.discriminator import PERIODS
    W = fold(model)
    sigs = d64(sigs)
    xs, ys = [], []
    for d, layers in enumerate(layer_table(version)):
        x = sigs.unsqueeze(1) if d == 0 else period_input(sigs, PERIODS[version][d - 1])
        xi, yo = [], []
        for name, stride, pad, groups, act in layers:
            w, b = W[name]
            xi.append(x)
            x = F.conv1d(x, w, b, stride, pad, 1, groups)
            if act:
                x = F.leaky_relu(x, SLOPE)
            yo.append(x)
        xs.append(xi)
        ys.append(yo)
    return xs, ys


def losses(ys, S):
    """discriminator_loss, generator_loss and feature_loss (train.py:286-315) of a forward whose first S / 2 signals
    are real and the rest generated, pair i being signals (i, S / 2 + i): the means over the whole batch."""
    out = {"losses_disc_r": [], "losses_disc_g": [], "losses_gen": []}
    fm = 0.0
    for maps in ys:
        half = maps[-1].shape[0] // 2
        d_r, d_g = maps[-1][:half], maps[-1][half:]
        out["losses_disc_r"].append(float(((1 - d_r) ** 2).mean()))
        out["losses_disc_g"].append(float((d_g ** 2).mean()))
        out["losses_gen"].append(float(((1 - d_g) ** 2).mean()))
        for f in maps:
            fm += float((f[:half] - f[half:]).abs().mean())
    out["loss_disc"] = sum(r + g for r, g in zip(out["losses_disc_r"], out["losses_disc_g"]))
    out["loss_gen"] = sum(out["losses_gen"])
    out["loss_fm"] = 2 * fm
    return out


def backward(model, version, xs, ys):
    """The gradient of ``loss_disc`` with respect to every parameter: {key: f64 tensor in the checkpoint's shape}."""
    W = fold(model)
    grads = {}
    for d, layers in enumerate(layer_table(version)):
        half = ys[d][-1].shape[0] // 2
        g_r, g_g = lsgan_grad(ys[d][-1][:half], ys[d][-1][half:])
        dy = torch.cat([g_r, g_g], 0)
        for l in range(len(layers) - 1, -1, -1):
            name, stride, pad, groups, act = layers[l]
            w, _ = W[name]
            y = ys[d][l] if act else None
            dW, db, _, _ = conv_bwd_weight(dy, y, xs[d][l], w.shape[2], stride, pad, groups)
            dg, dv = weight_norm_bwd(dW.reshape(model[name + ".weight_v"].shape), model[name + ".weight_v"],
                                     model[name + ".weight_g"])
            grads[name + ".bias"], grads[name + ".weight_g"], grads[name + ".weight_v"] = db, dg, dv
            if l:
                dy, _ = conv_bwd_data(dy, y, w, xs[d][l].shape[2], stride, pad, groups)
    return grads


def step(model, version, wave, y_hat, state, step_no, lr, betas, eps):
    """One D step on the pairs (wave[i], y_hat[i]) ([n][t] each) from ``state`` = {key: (exp_avg, exp_avg_sq)} (None:
    zeros), ``step_no`` the count after it -> gradients, grad_norm_d, the losses before, the stepped model and state
    (f64) and the second pass' losses with the stepped model."""
    sigs = torch.cat([d64(wave), d64(y_hat)], 0)
    xs, ys = forward(model, version, sigs)
    first = losses(ys, sigs.shape[0])
    grads = backward(model, version, xs, ys)
    new_model, new_state = {}, {}
    for k, g in grads.items():
        m, s = state[k] if state else (torch.zeros_like(g), torch.zeros_like(g))
        p, m, s = adamw(model[k], g, d64(m).reshape(g.shape), d64(s).reshape(g.shape), step_no, lr, betas, eps)
        new_model[k], new_state[k] = p, (m, s)
    _, ys2 = forward(new_model, version, sigs)
    return {"grads": grads, "grad_norm_d": grad_norm(grads.values()), "first": first, "model": new_model,
            "state": new_state, "second": losses(ys2, sigs.shape[0])}


# ---------------------------------------------------------------------------------------------- fixtures
def sample_index(n):
    """The flat indices a fixture stores of a tensor of n values: all of a small one, else every ceil(n / 128)-th."""
    return np.arange(0, n, max(1, -(-n // SAMPLE)))


def state_by_key(opt_state, version):
    """``optimizer.state_dict()``'s state as {checkpoint key: (exp_avg, exp_avg_sq)}: parameter i is the i-th key."""
    from rvc_amd.discriminator import discriminator_keys
    return {k: (opt_state["state"][i]["exp_avg"], opt_state["state"][i]["exp_avg_sq"])
            for i, k in enumerate(discriminator_keys(version))}


def fixture_ckpt(fx):
    """The D_*.pth dict a fixture's step started from: seeded weights and, for a warm case, the seeded AdamW state."""
    from rvc_amd import synthetic
    version = str(fx["version"])
    ck = synthetic.make_disc_ckpt(version, int(fx["seed"]))
    if int(fx["warm"]):
        ck["optimizer"] = synthetic.discriminator_optimizer_state(version, int(fx["opt_seed"]))
    return ck


def fixture_samples(fx, tensors):
    """The stored sample of every tensor of ``tensors`` ({checkpoint key: tensor}, any order) as one f64 vector in the
    fixture's order, next to ``fx["grad_f64"]`` / ``fx["post_f64"]``."""
    from rvc_amd.discriminator import discriminator_keys
    out = []
    for k, n in zip(discriminator_keys(str(fx["version"])), fx["sizes"]):
        flat = d64(tensors[k]).reshape(-1).numpy()
        idx = sample_index(flat.size)
        assert idx.size == int(n)
        out.append(flat[idx])
    return np.concatenate(out)


def hyper(version="v2"):
    from rvc_amd import synthetic
    t = synthetic.train_config(40000, version)["train"]
    return t["learning_rate"], tuple(t["betas"]), t["eps"]


# ---------------------------------------------------------------------------------------------- device vs fixture
def _ulp32(x):
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


def compare(trainer, fx, device="cuda"):
    """``trainer.step`` on a fixture's pairs, then the second pass -> {quantity: figure} against the reference's f64 run:
    ``grad`` / ``grad_max`` (largest relative RMS and absolute deviation of a tensor's gradient sample), ``grad_norms``
    (per-tensor norms, from the device's table), ``grad_norm_d``, ``loss_disc``, ``losses_disc_r`` / ``_g`` and the second
    pass' ``loss_gen`` / ``loss_fm`` (relative deviation), and for a warm case ``post``: the smallest tol with
    ``|p - p_ref| <= ulp(p_ref) + tol |p_ref - p_before|`` on every stored sample.  The device keeps the gradient of the
    folded weight; the samples of dg and dv are its weight-norm backward taken here in f64 (their norms and the update
    are the device's own)."""
    from rvc_amd.discriminator import discriminator_keys
    version = str(fx["version"])
    pairs = [(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)) for a, b in zip(fx["y"], fx["y_hat"])]
    before = trainer._model()
    first = trainer.step(pairs)
    grads, norms = {}, []
    table = trainer.table.cpu().numpy().reshape(-1, 3)
    for name in trainer.names:
        dW, db = trainer.dW[name].cpu(), trainer.db[name].cpu()
        v, g = before[name + ".weight_v"], before[name + ".weight_g"]
        dg, dv = weight_norm_bwd(dW.reshape(v.shape), v, g)
        grads[name + ".bias"], grads[name + ".weight_g"], grads[name + ".weight_v"] = db, dg, dv
    for k in discriminator_keys(version):
        name, suffix = k.rsplit(".", 1)
        r = trainer.rows[name]
        col = {"weight_g": 0, "weight_v": 1, "bias": 2}[suffix]
        norms.append(math.sqrt(table[r:r + trainer.P[name][0].numel(), col].sum()))
    got, want = fixture_samples(fx, grads), fx["grad_f64"]
    out = {"grad": 0.0, "grad_max": float(np.abs(got - want).max())}
    off = 0
    for n in fx["sizes"]:
        a, b = got[off:off + n], want[off:off + n]
        out["grad"] = max(out["grad"], float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))))
        off += n
    out["grad_norms"] = float(np.abs(np.array(norms) / fx["grad_norms_f64"] - 1).max())
    out["grad_norm_d"] = abs(first["grad_norm_d"] / float(fx["grad_norm_d_f64"]) - 1)
    out["loss_disc"] = abs(first["loss_disc"] / float(fx["loss_disc_f64"]) - 1)
    for k in ("losses_disc_r", "losses_disc_g"):
        out[k] = float(np.abs(np.array(first[k]) / fx[k + "_f64"] - 1).max())
    second = [trainer.losses(a, b) for a, b in pairs]
    for k in ("loss_gen", "loss_fm"):
        out[k] = abs(sum(s[k] for s in second) / len(second) / float(fx[k + "_f64"]) - 1)
    if int(fx["warm"]):
        p, ref, b4 = fixture_samples(fx, trainer._model()), fx["post_f64"], fx["before_f64"]
        out["post"] = float(np.max(np.maximum(np.abs(p - ref) - _ulp32(ref), 0.0) / np.abs(ref - b4)))
    return out
