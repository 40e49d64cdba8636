"""Golden outputs for formant shifting, from the REFERENCE's own stftpitchshift.py on the CPU.

Run where ``make_golden.py`` runs (the reference tree must exist):

    python tests/golden/make_golden_formant.py

``main/library/algorithm/stftpitchshift.py`` is loaded by path and called as ``load_audio`` calls it
(utils.py:104-108: ``StftPitchShift(1024, 32, 16000).shiftpitch(audio, factors=1,
quefrency=formant_qfrency * 1e-3, distortion=formant_timbre)``).  ``formant.npz`` holds, per case,
``out_<name>`` (the reference's f32 output) and ``par_<name>`` = (formant_qfrency, formant_timbre):
arrays only.  The inputs are not stored; they are rebuilt from ``rvc_amd.synthetic`` by seed
through ``tests/formant_ref.py:cases``, here and in the tests.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

from make_golden import OUT, REF, REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
from formant_ref import cases  # noqa: E402


def load_shifter():
    path = os.path.join(REF, "main", "library", "algorithm", "stftpitchshift.py")
    spec = importlib.util.spec_from_file_location("reference_stftpitchshift", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.StftPitchShift


def main():
    shifter = load_shifter()(1024, 32, 16000)
    out = {}
    for name, (x, qf, tb) in cases().items():
        y = shifter.shiftpitch(x, factors=1, quefrency=qf * 1e-3, distortion=tb)
        assert y.dtype == np.float32 and y.shape == x.shape and not np.isnan(y).any()
        out["out_" + name], out["par_" + name] = y, np.array([qf, tb], np.float64)
        print(name, len(x), "q =", int(qf * 1e-3 * 16000), "peak", float(np.abs(y).max()))
    np.savez_compressed(os.path.join(OUT, "formant.npz"), **out)


if __name__ == "__main__":
    main()
