"""Golden slices for dataset preprocessing, from the REFERENCE's own ``PreProcess.process_audio`` on the CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_preprocess.py

``main.inference.preprocess`` is imported through ``make_golden.setup_harness`` (the same scratch working directory
and stub modules).  Two names are replaced, both by this project's host functions, because the image has neither
soundfile nor librosa / soxr: the module's ``load_audio`` by ``rvc_amd.audio_io.load_audio`` and
``librosa.resample`` by ``rvc_amd.audio_io.resample`` (``scipy.signal.resample_poly``; parity with soxr is
therefore unpinned).  Everything else -- the filter, the normalisation, the slicer, the chunk loop, the files -- is
the reference's code.

Input: ``synthetic.silence_layout_audio(LAYOUT, seed=6100, sr=32000)`` written as a float32 WAV (the tests rebuild
it from the seed), ``per = 1.0``, ``cut_preprocess = process_effects = True``.

The same chain is run again with ``scipy.signal.sosfilt`` in place of ``lfilter``: the second-order-section form
of the same Butterworth, whose rounding noise is far below the ba form's.  The generator refuses to write unless
both chains cut the file alike and every frame's RMS is at least 1e-3 (relative) away from the slicer's threshold.
The largest difference between the two chains is the ba form's own rounding noise, and sets the tolerances:

    tol_gt  = 2 * max|lfilter chain - sosfilt chain| over the slices at sr   + 2^-24 * peak of those slices
    tol_16k = the same over the 16 kHz slices

Files (arrays only; split so that none passes 1 MiB): ``preprocess.npz`` -- ``names``, ``lengths`` [n][2]
(samples at sr, at 16 kHz), ``offsets`` [n][2] (start, length of every chunk in the processed audio), ``rms`` (the
slicer's track), ``threshold``, ``tol_gt``, ``tol_16k``, ``args`` = (sr, per, seed); ``preprocess_gt_a.npz`` /
``preprocess_gt_b.npz`` -- the slices at sr, ``gt_<k>``; ``preprocess_16k.npz`` -- ``k16_<k>``.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
from rvc_amd import audio_io, synthetic  # noqa: E402

LAYOUT = [(0.3, 0), (2.0, 1), (0.6, 0), (1.7, 1), (0.2, 0)]
SEED, SR, PER = 6100, 32000, 1.0


def run_chain(P, wav, exp_dir, sos=False):
    """The reference's process_audio -> (names, offsets [n][2], rms track, gt slices, 16 kHz slices)."""
    from scipy import signal
    seen = {"chunks": []}
    real_signal, real_rms = P.signal, P.get_rms
    if sos:
        coeffs = signal.butter(N=5, Wn=P.HIGH_PASS_CUTOFF, btype="high", fs=SR, output="sos")
        P.signal = types.SimpleNamespace(butter=signal.butter,
                                         lfilter=lambda b, a, x: signal.sosfilt(coeffs, np.asarray(x, np.float64)))

    def get_rms(*a, **k):
        seen["rms"] = real_rms(*a, **k)
        return seen["rms"]

    P.get_rms = get_rms
    try:
        pp = P.PreProcess(SR, exp_dir, PER)
        norm, seg = pp._normalize_audio, pp.process_audio_segment

        def normalize(audio):
            seen["audio"] = norm(audio)
            return seen["audio"]

        def segment(chunk, sid, idx0, idx1):
            seen["chunks"].append(chunk)
            return seg(chunk, sid, idx0, idx1)

        pp._normalize_audio, pp.process_audio_segment = normalize, segment
        pp.process_audio(wav, 0, 0, True, True, False, 0.7)
    finally:
        P.signal, P.get_rms = real_signal, real_rms
    base = seen["audio"]
    start = base.__array_interface__["data"][0]
    offsets = []
    for c in seen["chunks"]:  # every chunk is a view of the normalised audio
        assert c.base is not None and c.dtype == base.dtype
        offsets.append(((c.__array_interface__["data"][0] - start) // base.itemsize, c.shape[0]))
    names = sorted(os.listdir(pp.gt_wavs_dir), key=lambda n: int(n.split("_")[2].split(".")[0]))
    assert names == sorted(os.listdir(pp.wavs16k_dir), key=lambda n: int(n.split("_")[2].split(".")[0]))
    gt, k16 = [], []
    for n in names:
        x, sr = audio_io.read_wav(os.path.join(pp.gt_wavs_dir, n))
        assert sr == SR and x.dtype == np.float32
        gt.append(x)
        x, sr = audio_io.read_wav(os.path.join(pp.wavs16k_dir, n))
        assert sr == 16000 and x.dtype == np.float32
        k16.append(x)
    return names, np.array(offsets, np.int64), seen["rms"].squeeze(0), gt, k16, pp.slicer.threshold


def main():
    from make_golden import setup_harness
    here = os.getcwd()
    work = setup_harness()
    from main.inference import preprocess as P
    P.load_audio = lambda logger, path, sr: audio_io.load_audio(path, sr)
    sys.modules["librosa"].resample = lambda y, orig_sr, target_sr, res_type=None: audio_io.resample(y, orig_sr,
                                                                                                   target_sr)
    audio = synthetic.silence_layout_audio(LAYOUT, seed=SEED, sr=SR)
    wav = os.path.join(work, "input.wav")
    audio_io.write_wav_f32(wav, audio, SR)
    a = run_chain(P, wav, tempfile.mkdtemp(prefix="pre_ba_"))
    s = run_chain(P, wav, tempfile.mkdtemp(prefix="pre_sos_"), sos=True)
    os.chdir(here)
    names, offsets, rms, gt, k16, thr = a
    if names != s[0] or not np.array_equal(offsets, s[1]):
        raise SystemExit("the lfilter and sosfilt chains cut the file differently: try another seed")
    margin = np.abs(rms / thr - 1).min()
    print(f"{len(names)} chunks, lengths {[len(g) for g in gt]}, min RMS margin {margin:.3g}")
    if not margin >= 1e-3 or not np.abs(s[2] / thr - 1).min() >= 1e-3:
        raise SystemExit(f"a frame's RMS is within 1e-3 of the threshold ({margin:.3g}): try another seed")
    for k, (o, n) in enumerate(offsets):
        assert n == len(gt[k])

    def tol(x, y):
        d = max(np.abs(p.astype(np.float64) - q.astype(np.float64)).max() for p, q in zip(x, y))
        peak = max(np.abs(p).max() for p in x)
        print(f"  chain difference {d:.3g}, peak {peak:.3g}")
        return 2 * d + 2.0 ** -24 * float(peak)

    tol_gt, tol_16k = tol(gt, s[3]), tol(k16, s[4])
    print(f"tol_gt {tol_gt:.3g} tol_16k {tol_16k:.3g}")
    np.savez_compressed(os.path.join(HERE, "preprocess.npz"), names=np.array(names),
                        lengths=np.array([[len(g), len(k)] for g, k in zip(gt, k16)], np.int64), offsets=offsets,
                        rms=rms, threshold=np.float64(thr), tol_gt=np.float64(tol_gt), tol_16k=np.float64(tol_16k),
                        args=np.array([SR, PER, SEED], np.float64))
    half = (len(gt) + 1) // 2
    np.savez_compressed(os.path.join(HERE, "preprocess_gt_a.npz"), **{f"gt_{k}": gt[k] for k in range(half)})
    np.savez_compressed(os.path.join(HERE, "preprocess_gt_b.npz"), **{f"gt_{k}": gt[k] for k in range(half, len(gt))})
    np.savez_compressed(os.path.join(HERE, "preprocess_16k.npz"), **{f"k16_{i}": v for i, v in enumerate(k16)})


if __name__ == "__main__":
    main()
