"""Precision of the discriminator's training step on the device against the reference's f64 run
(tests/golden/disc_step_*): per fixture and quantity the device's figure (tests/disc_step_ref.compare) next to the
reference f32's own where the fixture records it (ref_dev).  tests/test_gpu_disc_step.py takes its bounds from this table
(4 x the device's figure of each case).

    python scripts/disc_step_prec.py --out profiles/disc_step_prec.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import disc_step_ref as ref  # noqa: E402
from rvc_amd import synthetic  # noqa: E402
from rvc_amd.discriminator import DiscriminatorTrainerAMD  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
REF_ROW = {"grad_max": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "disc_step_prec.txt"))
    a = ap.parse_args()
    lines = ["# the discriminator's step on the device vs the reference's f64 run (scripts/disc_step_prec.py)",
             "# dev: device - reference f64;  ref: reference f32 - reference f64 (the fixture's ref_dev)",
             "# grad: largest relative RMS of a tensor's gradient sample; grad_max: largest absolute deviation of one;",
             "# post: smallest tol with |p - p_ref| <= ulp(p_ref) + tol |p_ref - p_before|; the rest: relative deviation",
             "# %-4s %-14s %11s %11s" % ("case", "quantity", "dev", "ref")]
    for name, version in ref.CASES.items():
        fx = dict(np.load(os.path.join(GOLDEN, f"disc_step_{name}.npz")))
        t0 = time.time()
        tr = DiscriminatorTrainerAMD(ref.fixture_ckpt(fx), version, synthetic.train_config(40000, version)["train"], "cuda")
        torch.cuda.synchronize()
        t1 = time.time()
        got = ref.compare(tr, fx)
        ref_dev = dict(zip([str(s) for s in fx["ref_dev_names"]], fx["ref_dev"]))
        for k in sorted(got):
            r = ref_dev["grad"][1] if k == "grad_max" else ref_dev[k][0]
            lines.append("  %-4s %-14s %11.3e %11.3e" % (name, k, got[k], r))
        lines.append("# %s: trainer built in %.1f s, step + comparison %.1f s" % (name, t1 - t0, time.time() - t1))
        del tr
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
