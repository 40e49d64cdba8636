"""Register budget of the MiniBatchKMeans kernels (csrc/minibatch.hip), from hipcc's kernel-resource-usage remarks of
one device-only compile with the Makefile's flags: every kernel of the file is reported, and none uses scratch or
spills a VGPR or an SGPR."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rvc-maker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ["minibatch_update_kernel", "minibatch_weights_kernel", "minibatch_rowdist_kernel",
           "minibatch_status_kernel", "minibatch_scatter_kernel"]


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
    out = tmp_path_factory.mktemp("minibatch_build") / "minibatch.s"
    r = subprocess.run([HIPCC, *makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "minibatch.hip"),
                        "-o", str(out), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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


def test_every_kernel_is_reported(remarks):
    for name in KERNELS:
        assert sum(name in k for k in remarks) == 1, (name, sorted(remarks))
    assert len(remarks) == len(KERNELS), sorted(remarks)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_and_no_spills(remarks, name):
    r = [v for k, v in remarks.items() if name in k][0]
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs Spill"] == 0
    assert r["SGPRs Spill"] == 0
