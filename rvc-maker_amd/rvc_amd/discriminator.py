"""The training loop's discriminator and its GAN losses on the MI355X (main/inference/train.py).

``DiscriminatorAMD`` is ``MultiPeriodDiscriminator`` (train.py:608-674) -- one ``DiscriminatorS`` and one
``DiscriminatorP`` per period -- forward only, from the ``D_*.pth`` dict ``save_checkpoint`` writes beside every
``G_*.pth``; ``losses`` is ``discriminator_loss``, ``generator_loss`` and ``feature_loss`` (train.py:286-315) on one
(wave slice, y_hat) pair, with ``loss_gen_all`` (train.py:869) when the two generator losses are handed in.

Device layout.  ``DiscriminatorP`` pads its signal to a multiple of the period p and views it ``[H][p]``; its (k,1)
Conv2d layers never mix columns, so here column c is batch element c and every feature map is ``[p][C][H]``
(``reference_order`` gives the reference's ``[C][H][p]``).  ``rvc_period_front`` makes the first map from the signal
directly; the 32 -> 128 -> 512 -> 1024 -> 1024 convs and ``conv_post`` are batched Conv1d launches of the conv engine
with B = p.  All five period convs have stride 3, as train.py:657 builds them (upstream HiFi-GAN gives the last one
stride 1; the reference does not).  ``DiscriminatorS`` runs its k = 15, 5 and 3 convs on the engine and its four
grouped k = 41 convs on ``rvc_gconv_small``.  The real and the generated signal go through as one batch of two
(2p for a period), so each weight is read once; a feature map's two halves are then the pair ``rvc_pair_l1`` reads.
Spectral-norm checkpoints are refused.  csrc/discriminator.hip; DESIGN.md §19.
"""
from __future__ import annotations

import re

import torch

from . import ops
from .synth import fold_weight_norm

LRELU_SLOPE = 0.1
PERIODS = {"v1": (2, 3, 5, 7, 11, 17), "v2": (2, 3, 5, 7, 11, 17, 23, 37)}
# DiscriminatorS.convs (train.py:637): (Ci, Co, k, stride, groups, pad); its conv_post is (1024, 1, 3, 1, 1, 1)
S_CONVS = ((1, 16, 15, 1, 1, 7), (16, 64, 41, 4, 4, 20), (64, 256, 41, 4, 16, 20), (256, 1024, 41, 4, 64, 20),
           (1024, 1024, 41, 4, 256, 20), (1024, 1024, 5, 1, 1, 2))
S_POST = (1024, 1, 3, 1, 1, 1)
# DiscriminatorP.convs (train.py:657): (Ci, Co) at kernel (5,1), stride (3,1), padding (2,0); conv_post (1024, 1, (3,1))
P_CHANNELS = ((1, 32), (32, 128), (128, 512), (512, 1024), (1024, 1024))
P_KERNEL, P_STRIDE, P_PAD = 5, 3, 2


def discriminator_layers(version: str) -> list:
    """``(name, weight shape, groups)`` of every conv of ``MultiPeriodDiscriminator(version)`` in module order."""
    if version not in PERIODS:
        raise ValueError(f"rvc_amd: version {version!r}: the discriminator's periods are set for 'v1' and 'v2'")
    layers = []
    for j, (ci, co, k, _, g, _) in enumerate(S_CONVS):
        layers.append((f"discriminators.0.convs.{j}", (co, ci // g, k), g))
    layers.append(("discriminators.0.conv_post", (1, 1024, 3), 1))
    for i in range(1, len(PERIODS[version]) + 1):
        for j, (ci, co) in enumerate(P_CHANNELS):
            layers.append((f"discriminators.{i}.convs.{j}", (co, ci, P_KERNEL, 1), 1))
        layers.append((f"discriminators.{i}.conv_post", (1, 1024, 3, 1), 1))
    return layers


def discriminator_keys(version: str) -> dict:
    """The checkpoint keys of ``net_d`` and their shapes, in ``save_checkpoint``'s order and naming (train.py:269-271):
    per conv ``bias``, ``weight_g`` [Co][1]..., ``weight_v``."""
    keys = {}
    for name, shape, _ in discriminator_layers(version):
        keys[name + ".bias"] = (shape[0],)
        keys[name + ".weight_g"] = (shape[0],) + (1,) * (len(shape) - 1)
        keys[name + ".weight_v"] = tuple(shape)
    return keys


def check_supported(model: dict, version: str) -> None:
    """What the discriminator refuses, by name, before anything is uploaded."""
    spectral = [k for k in model if k.endswith((".weight_orig", ".weight_u"))]
    if spectral:
        raise NotImplementedError(f"rvc_amd: a spectral-norm discriminator ({spectral[0]} ...): only weight-norm "
                                  "checkpoints (use_spectral_norm = False, every shipped config) are on the device")
    want = discriminator_keys(version)
    found = {int(m.group(1)) for m in (re.match(r"discriminators\.(\d+)\.", k) for k in model) if m}
    n = len(PERIODS[version])
    if len(found) != n + 1:
        raise ValueError(f"rvc_amd: the checkpoint holds {max(len(found) - 1, 0)} period discriminators, version "
                         f"{version!r} has {n} ({list(PERIODS[version])})")
    missing = [k for k in want if k not in model]
    if missing:
        raise KeyError(f"rvc_amd: not a discriminator checkpoint: keys missing ({missing[:3]} ...)")
    bad = [k for k, s in want.items() if tuple(model[k].shape) != s]
    if bad:
        raise ValueError(f"rvc_amd: {bad[0]} has shape {tuple(model[bad[0]].shape)}, expected {want[bad[0]]}")


def reference_order(fmap: torch.Tensor, period: int = None) -> torch.Tensor:
    """One signal's feature map in the reference's order: a period map [p][C][H] -> [C][H][p]; DiscriminatorS's
    [C][L] (``period`` None) as it is.  A leading batch of one is dropped."""
    if period is None:
        return fmap.reshape(fmap.shape[-2], fmap.shape[-1])
    if fmap.dim() != 3 or fmap.shape[0] != period:
        raise ValueError(f"reference_order: expected [{period}][C][H], got {tuple(fmap.shape)}")
    return fmap.permute(1, 2, 0)


class DiscriminatorAMD:
    """``MultiPeriodDiscriminator(version)`` forward from a ``{"model": state_dict, ...}`` checkpoint dict."""

    def __init__(self, ckpt: dict, version: str = "v2", device: str = "cuda"):
        if version not in PERIODS:
            raise ValueError(f"rvc_amd: version {version!r}: the discriminator's periods are set for 'v1' and 'v2'")
        model = ckpt["model"]
        check_supported(model, version)
        self.version, self.periods, self.device = version, PERIODS[version], device
        self._build(model)

    def _build(self, model: dict) -> dict:
        """Fold the weight norm of a state dict on the host and put every conv on the device; returns the folded dict."""
        version, device = self.version, self.device
        W = fold_weight_norm({k: model[k] for k in discriminator_keys(version)})
        w = lambda name: W[name + ".weight"]  # noqa: E731
        b = lambda name: W[name + ".bias"]  # noqa: E731
        p0 = "discriminators.0."
        self.s_first = ops.Conv(w(p0 + "convs.0"), b(p0 + "convs.0"), device=device)
        self.s_grouped = [(w(p0 + f"convs.{j}").contiguous().to(device), b(p0 + f"convs.{j}").to(device))
                          for j in range(1, 5)]
        self.s_last = ops.Conv(w(p0 + "convs.5"), b(p0 + "convs.5"), device=device)
        self.s_post = ops.Conv(w(p0 + "conv_post"), b(p0 + "conv_post"), device=device)
        self.p_front, self.p_convs, self.p_post = [], [], []
        for i in range(1, len(self.periods) + 1):
            pi = f"discriminators.{i}."
            self.p_front.append((w(pi + "convs.0").reshape(32, 5).contiguous().to(device), b(pi + "convs.0").to(device)))
            self.p_convs.append([ops.Conv(w(pi + f"convs.{j}").squeeze(-1), b(pi + f"convs.{j}"), device=device)
                                 for j in range(1, 5)])
            self.p_post.append(ops.Conv(w(pi + "conv_post").squeeze(-1), b(pi + "conv_post"), device=device))
        self.n_disc = 1 + len(self.periods)
        self.n_fm = len(S_CONVS) + 1 + len(self.periods) * (len(P_CHANNELS) + 1)
        return W

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _conv(conv, x, stride, pad, act=True):
        B, _, Lin = x.shape
        Lout = (Lin + 2 * pad - conv.K) // stride + 1
        out = torch.empty(B, conv.Co, Lout, device=x.device, dtype=torch.float32)
        conv(x, stride=stride, pad=pad, out=out, out_act=ops.ACT_LRELU if act else ops.ACT_NONE,
             out_slope=LRELU_SLOPE if act else 0.0)
        return out

    def _scale(self, y):
        """DiscriminatorS.forward (train.py:641-649) on y [S][t] -> its 7 feature maps, each [S][C][L]."""
        x = self._conv(self.s_first, y.view(y.shape[0], 1, -1), 1, 7)
        fmap = [x]
        for wg, bg in self.s_grouped:
            x = ops.gconv_small(x, wg, bg, LRELU_SLOPE)
            fmap.append(x)
        x = self._conv(self.s_last, x, 1, 2)
        fmap.append(x)
        fmap.append(self._conv(self.s_post, x, 1, 1, act=False))
        return fmap

    def _period(self, i, y):
        """DiscriminatorP.forward (train.py:661-674) of period i on y [S][t] -> its 6 feature maps, each [S * p][C][H]
        (signal s in batch elements s * p .. s * p + p - 1)."""
        x = ops.period_front(y, *self.p_front[i], self.periods[i], LRELU_SLOPE)
        fmap = [x]
        for conv in self.p_convs[i]:
            x = self._conv(conv, x, P_STRIDE, P_PAD)
            fmap.append(x)
        fmap.append(self._conv(self.p_post[i], x, 1, 1, act=False))
        return fmap

    def _run(self, y):
        if y.dim() != 2 or y.dtype != torch.float32 or not y.is_cuda:
            raise ValueError("discriminator: signals must be f32 [S][t] on the device")
        y = y.contiguous()
        if y.shape[1] <= max(self.periods):
            raise ValueError(f"discriminator: {y.shape[1]} samples do not hold the reflect pad of period "
                             f"{max(self.periods)}")
        return [self._scale(y)] + [self._period(i, y) for i in range(len(self.periods))]

    def forward(self, y):
        """``d(y)`` of every discriminator (train.py:625): y [t] f32 on the device -> ``(y_d, fmap)``: per
        discriminator the ``conv_post`` output (the last feature map) and the list of its feature maps, in the device
        layout -- [1][C][L] for DiscriminatorS, [p][C][H] for a period (``reference_order``)."""
        fmaps = self._run(y.reshape(1, -1))
        return [f[-1] for f in fmaps], fmaps

    def period_of(self, i):
        """The period of discriminator i (None for DiscriminatorS, i = 0)."""
        return None if i == 0 else self.periods[i - 1]

    # ------------------------------------------------------------------ losses
    def loss_vector(self, wave_slice, y_hat, l1=None, c_mel=1.0, kl=None, c_kl=1.0):
        """The device f32 vector of ``ops.disc_finish`` for one (real, generated) pair, no host read."""
        if wave_slice.numel() != y_hat.numel():
            raise ValueError(f"losses: the wave slice has {wave_slice.numel()} samples, y_hat {y_hat.numel()}")
        fmaps = self._run(torch.stack([wave_slice.reshape(-1).float(), y_hat.reshape(-1).float()]))
        return self._loss_vector_of(fmaps, l1, c_mel, kl, c_kl)

    def _loss_vector_of(self, fmaps, l1=None, c_mel=1.0, kl=None, c_kl=1.0):
        y_hat = fmaps[0][0]
        table = ops.disc_table(self.n_fm, self.n_disc, y_hat.device)
        work, _ = ops.disc_work(y_hat.device)
        slot = 0
        for d, maps in enumerate(fmaps):
            for f in maps:
                half = f.shape[0] // 2
                ops.pair_l1(f[:half], f[half:], table, slot, work)
                slot += 1
            half = maps[-1].shape[0] // 2
            ops.lsgan_terms(maps[-1][:half], maps[-1][half:], table, self.n_fm + 3 * d, work)
        assert slot == self.n_fm
        return ops.disc_finish(table, self.n_fm, self.n_disc, l1, c_mel, kl, c_kl)

    def unpack(self, vec) -> dict:
        """``loss_vector``'s host copy as the dict ``losses`` returns."""
        v = [float(x) for x in vec]
        n, o = self.n_disc, ops.DISC_OUT_LISTS
        out = {"loss_disc": v[0], "loss_gen": v[1], "loss_fm": v[2], "losses_gen": v[o:o + n],
               "losses_disc_r": v[o + n:o + 2 * n], "losses_disc_g": v[o + 2 * n:o + 3 * n]}
        if v[3] == v[3]:  # not NaN: the generator's two losses were given
            out.update(loss_gen_all=v[3], loss_mel=v[4], loss_kl=v[5])
        return out

    def losses(self, wave_slice, y_hat, loss_mel=None, loss_kl=None, c_mel=1.0, c_kl=1.0) -> dict:
        """The GAN losses of one training step (train.py:851-869) on ``wave_slice`` and ``y_hat`` (f32 [segment_size]
        on the device) as floats: ``loss_disc``, ``losses_disc_r``, ``losses_disc_g`` (discriminator_loss), ``loss_gen``,
        ``losses_gen`` (generator_loss), ``loss_fm`` (feature_loss).  With ``loss_mel`` and ``loss_kl`` -- the device
        scalars of ``ops.slice_l1`` and ``ops.kl_loss``, weighted here by ``c_mel`` and ``c_kl`` in f32 -- also
        ``loss_mel``, ``loss_kl`` and ``loss_gen_all``.  Every mean is a fixed-order f64 sum rounded to f32; the sums
        over discriminators and feature maps are f32 in the reference's order.  One host read.

        The training loop runs ``net_d`` twice (train.py:851 and :863) with an optimizer step of D between them, so
        its ``loss_gen`` and ``loss_fm`` see D *after* that step.  A saved (G, D) pair cannot reproduce that: here both
        passes use the saved D, and are one pass (``y_hat.detach()`` changes no forward value)."""
        if (loss_mel is None) != (loss_kl is None):
            raise ValueError("losses: loss_mel and loss_kl go together")
        return self.unpack(self.loss_vector(wave_slice, y_hat, loss_mel, c_mel, loss_kl, c_kl).cpu().numpy())


# ---------------------------------------------------------------------------------------------- the training step
WEIGHT_DECAY = 0.01  # torch.optim.AdamW's default: train.py:766 passes lr, betas and eps only


def discriminator_convs(version: str) -> list:
    """Per discriminator its convs in forward order as ``(name, stride, pad, groups, activation)``."""
    out = [[(f"discriminators.0.convs.{j}", s, pad, g, True) for j, (_, _, _, s, g, pad) in enumerate(S_CONVS)] +
           [("discriminators.0.conv_post", 1, 1, 1, False)]]
    for i in range(1, len(PERIODS[version]) + 1):
        out.append([(f"discriminators.{i}.convs.{j}", P_STRIDE, P_PAD, 1, True) for j in range(len(P_CHANNELS))] +
                   [(f"discriminators.{i}.conv_post", 1, 1, 1, False)])
    return out


def check_trainable(ckpt: dict, version: str, hps_train: dict) -> None:
    """What the discriminator's step refuses, by name, before anything is uploaded."""
    check_supported(ckpt["model"], version)
    if hps_train.get("fp16_run"):
        raise NotImplementedError("rvc_amd: fp16_run / AMP training: the discriminator's step on the device is f32 "
                                  "(no autocast, no GradScaler)")
    for k in ("learning_rate", "betas", "eps"):
        if k not in hps_train:
            raise KeyError(f"rvc_amd: the experiment's config.json has no train.{k}")


def check_pairs(pairs) -> int:
    """The common length of the (wave slice, y_hat) pairs of one step."""
    if not pairs:
        raise ValueError("rvc_amd: a discriminator step needs at least one (wave slice, y_hat) pair")
    sizes = {int(t.numel()) for pair in pairs for t in pair}
    if len(sizes) != 1:
        raise ValueError(f"rvc_amd: pairs of unequal length ({sorted(sizes)}): a step takes slices of one segment_size, as "
                         "the reference's batch does")
    return sizes.pop()


def checkpoint_dict(version: str, model: dict, moments: dict, step: int, lr: float, betas, eps: float,
                    iteration: int) -> dict:
    """The dict ``save_checkpoint`` writes for ``net_d`` (train.py:269-271): ``model`` with ``.weight_g`` / ``.weight_v``
    keys in the module's order, ``optimizer`` as ``torch.optim.AdamW.state_dict()`` lays it out -- parameter i is the
    i-th key, ``net_d.parameters()``' order; ``moments`` = {key: (exp_avg, exp_avg_sq)}, empty before the first step
    -- ``iteration`` and ``learning_rate``.  The reference's ``load_checkpoint`` and ``DiscriminatorAMD`` read it."""
    from collections import OrderedDict
    keys = discriminator_keys(version)
    probe = torch.optim.AdamW([torch.zeros(1)], lr, betas=tuple(betas), eps=eps, weight_decay=WEIGHT_DECAY).state_dict()
    group = dict(probe["param_groups"][0], params=list(range(len(keys))))
    state = {}
    if moments:
        for i, (k, shape) in enumerate(keys.items()):
            m, s = moments[k]
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.float().reshape(shape),
                        "exp_avg_sq": s.float().reshape(shape)}
    return {"model": OrderedDict((k, model[k].float().reshape(shape)) for k, shape in keys.items()),
            "iteration": int(iteration), "optimizer": {"state": state, "param_groups": [group]}, "learning_rate": lr}


class DiscriminatorTrainerAMD(DiscriminatorAMD):
    """``net_d`` with its ``torch.optim.AdamW`` on the device: ``step`` is train.py:851-860 -- the forward on
    ``(wave, y_hat.detach())``, ``discriminator_loss``, its backward, ``grad_norm_d`` and the optimizer step -- after which
    ``forward`` and ``losses`` see the stepped weights, as the loop's second pass does (train.py:863-869).  No gradient
    reaches ``y_hat``; the generator's step is not here.  ``hps_train`` is the ``train`` section of the experiment's
    ``config.json``.  csrc/disc_backward.hip; DESIGN.md §20."""

    def __init__(self, ckpt: dict, version: str = "v2", hps_train: dict = None, device: str = "cuda"):
        if version not in PERIODS:
            raise ValueError(f"rvc_amd: version {version!r}: the discriminator's periods are set for 'v1' and 'v2'")
        hps_train = dict(hps_train or {})
        check_trainable(ckpt, version, hps_train)
        self.version, self.periods, self.device = version, PERIODS[version], device
        self.keys = discriminator_keys(version)
        self.convs = discriminator_convs(version)
        self.names = [c[0] for convs in self.convs for c in convs]
        opt = ckpt.get("optimizer") or {}
        groups = opt.get("param_groups") or [{}]
        self.lr = float(groups[0].get("lr", hps_train["learning_rate"]))
        self.betas = tuple(float(b) for b in hps_train["betas"])
        self.eps = float(hps_train["eps"])
        self.iteration = int(ckpt.get("iteration", 0))
        model, state = ckpt["model"], opt.get("state") or {}
        index = {k: i for i, k in enumerate(self.keys)}
        if state and len(state) != len(self.keys):
            raise ValueError(f"rvc_amd: the optimizer state holds {len(state)} parameters, net_d has {len(self.keys)}")
        self.step_count = int(float(state[0]["step"])) if state else 0
        dev = lambda t: t.detach().float().reshape(-1).contiguous().to(device)  # noqa: E731
        self.P, self.M, self.dW, self.db, self.rows = {}, {}, {}, {}, {}
        row = 0
        for name in self.names:
            self.P[name] = tuple(dev(model[name + s]) for s in (".weight_g", ".weight_v", ".bias"))
            moments = []
            for s in (".weight_v", ".weight_g", ".bias"):  # rvc_wn_adamw's order: m_v, s_v, m_g, s_g, m_b, s_b
                st = state.get(index[name + s]) if state else None
                for m in ("exp_avg", "exp_avg_sq"):
                    moments.append(dev(st[m]) if st else torch.zeros(model[name + s].numel(), device=device))
            self.M[name] = tuple(moments)
            self.dW[name] = torch.empty(self.keys[name + ".weight_v"][:3], device=device, dtype=torch.float32)
            self.db[name] = torch.empty(self.keys[name + ".bias"], device=device, dtype=torch.float32)
            self.rows[name] = row
            row += self.keys[name + ".bias"][0]
        self.table = torch.zeros(3 * row, device=device, dtype=torch.float64)
        self.work = None
        self._refold(model)

    # ------------------------------------------------------------------ weights
    def _model(self) -> dict:
        """The parameters as a host state dict in the checkpoint's keys and shapes."""
        out = {}
        for name in self.names:
            g, v, b = self.P[name]
            out[name + ".bias"] = b.cpu()
            out[name + ".weight_g"] = g.cpu().reshape(self.keys[name + ".weight_g"])
            out[name + ".weight_v"] = v.cpu().reshape(self.keys[name + ".weight_v"])
        return out

    def _refold(self, model: dict = None):
        """w = g v / |v| and the conv engine's packed images from the current parameters.  The fold runs where
        ``DiscriminatorAMD`` runs it for a checkpoint -- ``torch._weight_norm`` on the host -- so that a saved step reloads to
        the same bits; the parameters cross the host once per step (DESIGN.md §20 has the cost)."""
        W = self._build(self._model() if model is None else model)
        self.w = {name: W[name + ".weight"].reshape(self.keys[name + ".weight_v"][:3]).contiguous().to(self.device)
                  for name in self.names}
        self._dirty = False

    def _run(self, y):
        if self._dirty:
            self._refold()
        return super()._run(y)

    # ------------------------------------------------------------------ the step
    def _work(self, sig):
        if self.work is None:
            self.work = torch.empty(64 << 20, device=self.device, dtype=torch.uint8)
        return self.work

    def _backward(self, sig, fmaps, scale, accumulate):
        """Gradients of ``scale * discriminator_loss`` of one pair (sig [2][t], its feature maps) into dW / db."""
        work = self._work(sig)
        for d, convs in enumerate(self.convs):
            maps = fmaps[d]
            dy = ops.lsgan_grad(maps[-1], scale)
            for l in range(len(convs) - 1, -1, -1):
                name, stride, pad, groups, act = convs[l]
                y = maps[l] if act else None
                first = l == 0
                x = sig if first and d else sig.view(2, 1, -1) if first else maps[l - 1]
                ops.conv_bwd_weight(dy, y, x, self.dW[name], self.db[name], stride, pad, groups, LRELU_SLOPE, 1.0,
                                    accumulate, self.periods[d - 1] if first and d else 0, work)
                if not first:  # a first conv's input is the signal: no gradient in this step
                    dy = ops.conv_bwd_data(dy, y, self.w[name], x.shape[2], stride, pad, groups, LRELU_SLOPE)

    def step(self, pairs) -> dict:
        """One optimizer step of D on ``pairs`` = [(wave_slice, y_hat), ...] (f32 [segment_size] each, on the device):
        the gradient of the reference's batch of those pairs (each pair's gradient at scale 1 / len(pairs), summed),
        ``grad_norm_d`` as ``clip_grad_value(net_d.parameters(), None)`` returns it, one AdamW update.  Returns
        ``loss_disc``, ``losses_disc_r``, ``losses_disc_g`` (the batch's means) and ``grad_norm_d``."""
        check_pairs(pairs)
        n = len(pairs)
        vecs = []
        for i, (wave, y_hat) in enumerate(pairs):
            sig = torch.stack([wave.reshape(-1).float(), y_hat.detach().reshape(-1).float()]).contiguous()
            fmaps = self._run(sig)
            vecs.append(self._loss_vector_of(fmaps))
            self._backward(sig, fmaps, 1.0 / n, i > 0)
        self.step_count += 1
        for name in self.names:
            g, v, b = self.P[name]
            r = self.rows[name]
            ops.wn_adamw(self.dW[name], self.db[name], v, g, b, self.M[name], self.table[3 * r:3 * (r + g.numel())],
                         self.lr, self.betas, self.eps, WEIGHT_DECAY, self.step_count)
        norm = ops.grad_norm(self.table)
        self._dirty = True
        per = [self.unpack(v.cpu().numpy()) for v in vecs]
        out = {"loss_disc": sum(p["loss_disc"] for p in per) / n,
               "losses_disc_r": [sum(p["losses_disc_r"][i] for p in per) / n for i in range(self.n_disc)],
               "losses_disc_g": [sum(p["losses_disc_g"][i] for p in per) / n for i in range(self.n_disc)],
               "grad_norm_d": float(norm.item())}
        return out

    def gradients(self) -> dict:
        """The last step's gradients of the folded weights and biases, ``{name: (dW [Co][Ci / groups][K], db [Co])}``."""
        return {name: (self.dW[name], self.db[name]) for name in self.names}

    # ------------------------------------------------------------------ state
    def snapshot(self) -> dict:
        """D and its optimizer state, to ``restore`` later: device copies of the parameters and moments, and the folded
        weights as they are (a step replaces them, it does not write into them)."""
        if self._dirty:
            self._refold()
        fwd = {k: getattr(self, k) for k in ("s_first", "s_grouped", "s_last", "s_post", "p_front", "p_convs", "p_post",
                                             "w")}
        return {"P": {k: tuple(t.clone() for t in v) for k, v in self.P.items()},
                "M": {k: tuple(t.clone() for t in v) for k, v in self.M.items()},
                "step": self.step_count, "lr": self.lr, "iteration": self.iteration, "fwd": fwd}

    def restore(self, snap: dict) -> None:
        for k, v in snap["P"].items():
            for dst, src in zip(self.P[k], v):
                dst.copy_(src)
        for k, v in snap["M"].items():
            for dst, src in zip(self.M[k], v):
                dst.copy_(src)
        self.step_count, self.lr, self.iteration = snap["step"], snap["lr"], snap["iteration"]
        for k, v in snap["fwd"].items():
            setattr(self, k, v)
        self._dirty = False

    def state_dict(self, iteration: int = None) -> dict:
        """The dict ``save_checkpoint`` writes for ``net_d`` (``checkpoint_dict``)."""
        slot = {"weight_v": 0, "weight_g": 2, "bias": 4}
        moments = {}
        if self.step_count:
            for k in self.keys:
                name, suffix = k.rsplit(".", 1)
                m, j = self.M[name], slot[suffix]
                moments[k] = (m[j].cpu(), m[j + 1].cpu())
        return checkpoint_dict(self.version, self._model(), moments, self.step_count, self.lr, self.betas, self.eps,
                               self.iteration if iteration is None else iteration)

    def save(self, path: str, iteration: int = None) -> None:
        torch.save(self.state_dict(iteration), path)
