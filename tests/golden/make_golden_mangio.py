"""Golden f0 tracks for mangio-crepe-* and rmvpe-legacy, from the REFERENCE's own convert.py / extract.py on the CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_mangio.py

The harness and the stubs are ``make_golden.py``'s (``setup_harness``; librosa's Viterbi is the oracle's restatement, as
for crepe.npz).  Data only: ``mangio.npz`` and ``rmvpe_legacy.npz``.

One signal, ``synthetic_audio(1.0, seed=31)[:12040]`` in f32 (p_len 75, 76 estimator frames; ``make_golden_f0_paths``'s),
handed to the reference as f64.  The conversion-side VC has x_pad = 0, so that the f0 file starts at frame 0.

``mangio.npz`` -- weights ``crepe_state_dict(1241, "tiny")``.  Per hop h in HOPS: ``probs_<h>`` [T][360] (the sigmoid
outputs at ``postprocess`` entry, before its in-place mask), ``bins_<h>`` [T] (the Viterbi's), ``dither_<h>`` [T] (every
``scipy.stats.triang.rvs`` draw, in order; numpy's generator is re-seeded before every call, so every call at one hop
draws the same values), ``f0_<h>`` (get_f0_mangio_crepe's return, f64 [75]) and ``batches_<h>``.  For hop 64 also
``vc:<variant>:coarse`` / ``:pitchf`` (get_f0 for the three variants of make_golden_f0_paths) and ``fi_f0``
(FeatureInput.get_mangio_crepe, whose input scale is torch.quantile's).

``rmvpe_legacy.npz`` -- weights ``rmvpe_state_dict(10)``: ``plain`` / ``legacy`` (get_f0_rmvpe, f64 [76]), the three get_f0
variants, ``fi_f0`` (FeatureInput.get_rmvpe(legacy=True)), and ``hybrid:coarse`` / ``hybrid:pitchf``: get_f0 of
``hybrid[mangio-crepe-tiny+rmvpe-legacy]`` at hop 64 (with mangio.npz's weights and hop-64 dither).

The script refuses to write unless the tests' conditions hold on the reference alone (``check_mangio``, ``check_legacy``);
among them, at hops 37 and 64, that no tail frame of a batch (which torch computes with the C library's powf, the rest
with its vector pow) differs between the two routines, so that the recorded track does not hang on the host's vector
width.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: mangio_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import make_golden as mg  # noqa: E402  (puts rvc-maker_amd on the path)
from make_golden_f0_paths import AUDIO_SEED, N, P_LEN, VARIANTS  # noqa: E402
from rvc_amd import synthetic  # noqa: E402
import mangio_ref  # noqa: E402

CREPE_SEED, RMVPE_SEED, NP_SEED = 1241, 10, 64
HOPS = (37, 64, 160, 512)
CHECKED_HOPS = (37, 64)
NET_BOUND = 2e-5  # the network bound of tests/test_gpu_crepe.py
HYBRID = "hybrid[mangio-crepe-tiny+rmvpe-legacy]"
EDGE_HZ = 0.1  # ten times the 1e-2 Hz bound of tests/test_gpu_rmvpe.py


class Recorder:
    """Records, per ``predict`` call, the probabilities at ``postprocess`` entry, the Viterbi's bins and the dither."""

    def __init__(self, RC):
        import scipy.stats
        self.RC, self.stats = RC, scipy.stats
        self.probs, self.bins, self.draws = [], [], []

    def __enter__(self):
        self.rvs0, self.post0, self.vit0 = self.stats.triang.rvs, self.RC.postprocess, self.RC.viterbi

        def rvs(*a, **k):
            v = self.rvs0(*a, **k)
            self.draws.append(np.asarray(v, dtype=np.float64).reshape(-1))
            return v

        def post(p, *a, **k):
            self.probs.append(p[0].t().numpy().copy())  # [T_batch][360], before the in-place mask
            return self.post0(p, *a, **k)

        def vit(logits):
            bins, pitch = self.vit0(logits)
            self.bins.append(bins[0].numpy().astype(np.int64).copy())
            return bins, pitch

        self.stats.triang.rvs, self.RC.postprocess, self.RC.viterbi = rvs, post, vit
        return self

    def __exit__(self, *a):
        self.stats.triang.rvs, self.RC.postprocess, self.RC.viterbi = self.rvs0, self.post0, self.vit0

    def take(self):
        out = (np.concatenate(self.probs), np.concatenate(self.bins), np.concatenate(self.draws),
               [len(p) for p in self.probs])
        self.probs, self.bins, self.draws = [], [], []
        return out


def check_mangio(hop, probs, bins, dither):
    """The conditions the tests lean on at one hop; a description of the first that fails, or None."""
    T = probs.shape[0]
    seg = mangio_ref.segments(T, hop)
    mine = mangio_ref.viterbi_bins(probs, seg)
    if not np.array_equal(mine, bins):
        return f"the restated decode differs in {int((mine != bins).sum())} frames"
    whole = mangio_ref.viterbi_bins(probs, [0, T])
    restart = int((whole != bins).sum())
    rng = np.random.default_rng(hop)
    flips = 0
    for _ in range(10):
        sign = rng.integers(0, 2, size=probs.shape).astype(np.float32) * 2 - 1
        flips += int((mangio_ref.viterbi_bins(probs + np.float32(NET_BOUND) * sign, seg) != bins).sum())
    print(f"  hop {hop}: T={T} segments={np.diff(seg).tolist()} bins={sorted(set(bins.tolist()))} "
          f"restart visible in {restart} frames, flips under +-{NET_BOUND}: {flips}")
    if restart == 0:
        return "one segment over the whole track gives the same bins: a missing restart would be invisible"
    if len(set(bins.tolist())) < 2:
        return "a single bin"
    if flips:
        return f"{flips} bins flip under +-{NET_BOUND}"
    # torch computes each batch's tail frames with the C library's powf and the rest with its vector pow; the device
    # (and mangio_ref's host-independent form) uses the vector routine throughout
    per_batch, vector = (mangio_ref.bins_to_hz(bins, dither, seg, vector=v) for v in (False, True))
    if not np.array_equal(per_batch, vector):
        return f"{int((per_batch != vector).sum())} tail frames differ between torch's scalar and vector pow"
    return None


def gen_mangio(conv, ext, x64):
    from main.library.predictors import CREPE as RC
    torch.save(synthetic.crepe_state_dict(CREPE_SEED, "tiny"),
               os.path.join("assets", "models", "predictors", "crepe_tiny.pth"))
    vc = conv.VC(40000, conv.config)
    vc.x_pad = 0
    out = {"x": x64.astype(np.float32), "seeds": np.array([CREPE_SEED, NP_SEED])}
    with Recorder(RC) as rec:
        for hop in HOPS:
            np.random.seed(NP_SEED)
            f0 = vc.get_f0_mangio_crepe(x64.copy(), P_LEN, hop, "tiny")
            probs, bins, dither, batches = rec.take()
            assert probs.shape == (1 + N // hop, 360) and probs.dtype == np.float32 and f0.shape == (P_LEN,)
            assert f0.dtype == np.float64 and batches == np.diff(mangio_ref.segments(len(probs), hop)).tolist()
            if hop in CHECKED_HOPS:
                why = check_mangio(hop, probs, bins, dither)
                if why:
                    raise SystemExit(f"mangio hop {hop}: {why}: try another weight or dither seed")
            assert np.array_equal(mangio_ref.f0(probs, hop, dither, P_LEN), f0)
            out.update({f"probs_{hop}": probs, f"bins_{hop}": bins, f"dither_{hop}": dither, f"f0_{hop}": f0,
                        f"batches_{hop}": np.array(batches)})
        for name, (pitch, autotune, strength, f0_file) in VARIANTS.items():
            np.random.seed(NP_SEED)
            coarse, pitchf = vc.get_f0(x64.copy(), P_LEN, pitch, "mangio-crepe-tiny", 3, 64, autotune, strength,
                                       None if f0_file is None else f0_file.copy())
            assert np.array_equal(rec.take()[2], out["dither_64"])
            out[f"vc:{name}:coarse"], out[f"vc:{name}:pitchf"] = coarse, pitchf
        np.random.seed(NP_SEED)
        out["fi_f0"] = ext.FeatureInput(device="cpu").get_mangio_crepe(x64.astype(np.float32), 64, "tiny")
        assert np.array_equal(rec.take()[2], out["dither_64"])
    assert np.array_equal(out["vc:plain:pitchf"], out["f0_64"])
    np.savez_compressed(os.path.join(mg.OUT, "mangio.npz"), **out)
    print("mangio", {k: v.shape for k, v in out.items() if v.ndim})
    return vc, out["dither_64"]


def check_legacy(plain, legacy):
    below, above = (plain > 0) & (plain < 50), plain > 1100
    kept = int(np.count_nonzero(legacy))
    edge = float(min(np.abs(plain - 50).min(), np.abs(plain - 1100).min()))
    print(f"  rmvpe-legacy: zeroed below {int(below.sum())}, above {int(above.sum())}, kept {kept}, "
          f"nearest frame {edge:.3g} Hz from a bound")
    if not np.array_equal(legacy, np.where(below | above, 0.0, plain)):
        return "legacy is not plain with the frames outside 50..1100 Hz zeroed"
    if below.sum() < 5 or above.sum() < 5:
        return "fewer than 5 frames zeroed on one side"
    if kept < 10:
        return "fewer than 10 voiced frames kept"
    if edge < EDGE_HZ:
        return f"a frame within {EDGE_HZ} Hz of a bound"
    return None


def gen_rmvpe_legacy(conv, ext, x64, vc, dither):
    torch.save(synthetic.rmvpe_state_dict(RMVPE_SEED), os.path.join("assets", "models", "predictors", "rmvpe.pt"))
    plain, legacy = vc.get_f0_rmvpe(x64.copy()), vc.get_f0_rmvpe(x64.copy(), legacy=True)
    why = check_legacy(plain, legacy)
    if why:
        raise SystemExit(f"rmvpe-legacy: {why}: try another weight seed")
    out = {"x": x64.astype(np.float32), "seeds": np.array([RMVPE_SEED, CREPE_SEED, NP_SEED]), "plain": plain,
           "legacy": legacy}
    for name, (pitch, autotune, strength, f0_file) in VARIANTS.items():
        coarse, pitchf = vc.get_f0(x64.copy(), P_LEN, pitch, "rmvpe-legacy", 3, 64, autotune, strength,
                                   None if f0_file is None else f0_file.copy())
        out[f"vc:{name}:coarse"], out[f"vc:{name}:pitchf"] = coarse, pitchf
    out["fi_f0"] = ext.FeatureInput(device="cpu").get_rmvpe(x64.copy(), legacy=True)
    assert np.array_equal(out["fi_f0"], legacy)
    np.random.seed(NP_SEED)
    out["hybrid:coarse"], out["hybrid:pitchf"] = vc.get_f0(x64.copy(), P_LEN, 0, HYBRID, 3, 64, False, 1.0, None)
    out["hybrid_dither"] = dither
    np.savez_compressed(os.path.join(mg.OUT, "rmvpe_legacy.npz"), **out)
    print("rmvpe_legacy", {k: v.shape for k, v in out.items() if v.ndim})


def main():
    x64 = synthetic.synthetic_audio(1.0, seed=AUDIO_SEED)[:N].astype(np.float32).astype(np.float64)
    mg.setup_harness()
    import main.inference.convert as conv
    import main.inference.extract as ext
    torch.set_num_threads(8)
    with torch.no_grad():
        vc, dither = gen_mangio(conv, ext, x64)
        gen_rmvpe_legacy(conv, ext, x64, vc, dither)


if __name__ == "__main__":
    main()
