"""Precision of the discriminator and the GAN losses on the device against the reference's f64 run
(tests/golden/discriminator_*): per fixture and quantity the device's deviation (tests/discriminator_ref.compare), next
to the reference f32's own where the fixture records it (ref_dev).  tests/test_gpu_discriminator.py takes its bounds from
this table (4 x the largest device figure of the three cases, never above 1e-4 relative).

    python scripts/discriminator_prec.py --out profiles/discriminator_prec.txt
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import discriminator_ref as ref  # noqa: E402
from rvc_amd.discriminator import DiscriminatorAMD  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
# the fixture's ref_dev row that speaks of the same quantity (whole maps there, their samples here)
REF_ROW = {"fm_sample_r": "fmap_r", "fm_sample_g": "fmap_g"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "discriminator_prec.txt"))
    a = ap.parse_args()
    lines = ["# discriminator and GAN losses on the device vs the reference's f64 run (scripts/discriminator_prec.py)",
             "# dev_* : device f32 - reference f64;  ref_* : reference f32 - reference f64 (the fixture's ref_dev)",
             "# rel: relative RMS (y_d, fm_sample: the largest over the list) or relative deviation (everything else);",
             "# max: largest absolute deviation (y_d, fm_sample)",
             "# %-4s %-14s %11s %11s %11s %11s" % ("case", "quantity", "dev_rel", "dev_max", "ref_rel", "ref_max")]
    discs, worst = {}, {}
    for name, version in ref.CASES.items():
        fx = dict(np.load(os.path.join(GOLDEN, f"discriminator_{name}.npz")))
        key = (version, int(fx["seed"]))
        if key not in discs:
            discs[key] = DiscriminatorAMD(ref.fixture_ckpt(fx), version, "cuda")
        got, _ = ref.compare(discs[key], fx)
        ref_dev = dict(zip([str(s) for s in fx["ref_dev_names"]], fx["ref_dev"]))
        for k in sorted(got):
            r = ref_dev.get(REF_ROW.get(k, k))
            lines.append("  %-4s %-14s %11.3e %11.3e %11s %11s" % (
                name, k, got[k][0], got[k][1], "-" if r is None else "%.3e" % r[0], "-" if r is None else "%.3e" % r[1]))
            worst[k] = (max(worst.get(k, (0, 0))[0], got[k][0]), max(worst.get(k, (0, 0))[1], got[k][1]))
    lines.append("# the largest of the three cases (MEASURED of tests/test_gpu_discriminator.py)")
    for k in sorted(worst):
        lines.append("  max  %-14s %11.3e %11.3e" % (k, *worst[k]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
