"""f64 restatement (torch on the CPU) of the training forward's new pieces: spectrogram_torch, spec_to_mel_torch,
slice_segments + l1_loss and kl_loss (main/inference/train.py:700-716, 845, 865, 317-325), the posterior encoder
(synthesizers.py:387-391) and the flow in the forward direction (residuals.py:87-90, 127-136; modules.py:35-51), all at
an all-ones mask.  tests/test_train_forward_cpu.py pins it to the reference's own f64 stages in the fixtures; the GPU
tests then use it at shapes the fixtures do not hold."""
import numpy as np
import torch
import torch.nn.functional as F

from rvc_amd import melbasis


def fixture_ckpt(fx, sr, version):
    """The training checkpoint a fixture was made with: ``synthetic.make_train_ckpt`` of its seed with the recorded
    ``.weight_g`` tensors put back.  Everything else in it is NumPy draws rounded to f32, the same on every host; the
    weight-norm g is ``||v|| * u`` with the norm an f32 torch reduction, whose summation order follows the host's
    vector width (one bit off on some hosts, 1e-8 in the stages)."""
    from rvc_amd import synthetic
    ck = synthetic.make_train_ckpt(sr, version, int(fx["seed"]))
    off = 0
    for k, n in zip(fx["wg_keys"], fx["wg_sizes"]):
        k, n = str(k), int(n)
        ck["model"][k] = torch.from_numpy(fx["wg_values"][off:off + n].copy()).reshape(ck["model"][k].shape)
        off += n
    assert off == fx["wg_values"].size
    return ck


def _t64(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double()


def spectrogram(y, n_fft, hop):
    """y [B][N] -> f64 [B][n_fft/2+1][F]: reflect pad (n_fft - hop) / 2, center=False, periodic Hann of n_fft -- the
    f32 torch.hann_window, which the reference's f64 run casts up (train.py:704)."""
    y = _t64(y)
    pad = (n_fft - hop) // 2
    yp = F.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    frames = yp.unfold(-1, n_fft, hop)  # [B][F][n_fft]
    win = torch.hann_window(n_fft, dtype=torch.float32).double()
    s = torch.fft.rfft(frames * win, dim=-1)
    return torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-6).transpose(1, 2).contiguous()


def mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """f32 [M][K]: librosa.filters.mel's defaults as rvc_amd.melbasis restates them."""
    return melbasis.mel_filterbank(sr, n_fft, n_mels, fmin, sr / 2.0 if fmax is None else fmax, htk=False)


def mel_log(spec, basis):
    return torch.log(torch.clamp(torch.matmul(_t64(basis), _t64(spec)), min=1e-5))


def slice_segments(x, ids, S):
    return torch.stack([x[b, :, int(ids[b]):int(ids[b]) + S] for b in range(x.shape[0])])


def slice_l1(mel, ids, yhat_mel):
    mel, yhat_mel = _t64(mel), _t64(yhat_mel)
    return float((slice_segments(mel, ids, yhat_mel.shape[-1]) - yhat_mel).abs().mean())


def kl_loss(z_p, logs_q, m_p, logs_p):
    z_p, logs_q, m_p, logs_p = (_t64(t) for t in (z_p, logs_q, m_p, logs_p))
    kl = logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * torch.exp(-2.0 * logs_p)
    return float(kl.sum() / (z_p.shape[0] * z_p.shape[-1]))


def fold64(model):
    """Checkpoint {.weight_g, .weight_v} -> f64 {.weight}, as the f64 module's parametrization computes it."""
    W = {}
    for k, v in model.items():
        if k.endswith(".weight_v"):
            base = k[:-len(".weight_v")]
            W[base + ".weight"] = torch._weight_norm(v.double(), model[base + ".weight_g"].double(), 0)
        elif not k.endswith(".weight_g"):
            W[k] = v.double()
    return W


def _conv(W, name, x, padding=0):
    return F.conv1d(x, W[name + ".weight"], W[name + ".bias"], padding=padding)


def wavenet(W, p, x, g, hidden, n_layers, k=5):
    out = torch.zeros_like(x)
    gc = _conv(W, p + "cond_layer", g)
    for i in range(n_layers):
        a = _conv(W, p + f"in_layers.{i}", x, padding=(k - 1) // 2) + gc[:, i * 2 * hidden:(i + 1) * 2 * hidden]
        acts = torch.tanh(a[:, :hidden]) * torch.sigmoid(a[:, hidden:])
        rs = _conv(W, p + f"res_skip_layers.{i}", acts)
        if i < n_layers - 1:
            x = x + rs[:, :hidden]
            out = out + rs[:, hidden:]
        else:
            out = out + rs
    return out


def speaker(W, sid):
    return W["emb_g.weight"][int(sid)][None, :, None]


def posterior(W, spec, g, noise, inter=192, hidden=192):
    """-> z, m_q, logs_q (f64 [1][inter][T])."""
    x = _conv(W, "enc_q.pre", _t64(spec).reshape(1, -1, spec.shape[-1]))
    stats = _conv(W, "enc_q.proj", wavenet(W, "enc_q.enc.", x, g, hidden, 16))
    m, logs = stats[:, :inter], stats[:, inter:]
    return m + _t64(noise).reshape(m.shape) * torch.exp(logs), m, logs


def flow_forward(W, z, g, inter=192, hidden=192):
    x = _t64(z)
    half = inter // 2
    for f in range(4):
        p = f"flow.flows.{2 * f}."
        x0, x1 = x[:, :half], x[:, half:]
        m = _conv(W, p + "post", wavenet(W, p + "enc.", _conv(W, p + "pre", x0), g, hidden, 3))
        x = torch.flip(torch.cat([x0, m + x1], 1), [1])
    return x
