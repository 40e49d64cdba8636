"""Register budget of the fused ResBlock pair kernels (csrc/resblock.hip), from hipcc's kernel-resource-usage
remarks of a device-only compile with the Makefile's flags: the two instances the default path runs -- the C = 32
split-fp16 pair and the wide C = 64 one -- keep 3 waves per SIMD with nothing spilled.  A spilled value is reloaded
through vmcnt, in order behind the weight prefetch ring, so every reload waits for the prefetch just issued
(DESIGN 7)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rvc-maker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

DEFAULT_PATH = ["resblock_x6_kernelILi32ELi3ELb1ELb0EE", "resblock_x6_kernelILi64ELi3ELb1ELb1EE"]


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with its default ARCH and no EXTRA."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("rb_build") / "resblock.s"
    r = subprocess.run([HIPCC, *makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "resblock.hip"), "-o",
                        str(out), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("inst", DEFAULT_PATH)
def test_default_path_pairs_do_not_spill(remarks, inst):
    hits = [v for k, v in remarks.items() if inst in k]
    assert len(hits) == 1, sorted(remarks)
    r = hits[0]
    print(inst, r)
    assert r["VGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["Occupancy [waves/SIMD]"] == 3
