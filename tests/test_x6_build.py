"""Register budget of the split-operand conv engine (csrc/conv1d.hip conv_x6_kernel), from hipcc's kernel-resource-usage
remarks of one device-only compile with the Makefile's flags: the instances the default path runs at C >= 128 in
split-fp16 -- the 128 x 256 tile with the fast-only loaders (leaky-ReLU and plain input, <2,8,4,2,NI,3,true,false,1|2>)
and the 128 x 128 tile (<2,4,4,2,NI,3,true,false,1>), at both loader item counts NI -- keep 3 waves per SIMD with
nothing spilled and no scratch.

The 128 x 256 instances spilled 47 VGPRs (132 B of scratch per lane) before the row-base epilogue
(conv_epilogue_rows): every scratch access sat in the epilogue, and the second row-fragment pass's accumulators came
back one by one behind vmcnt(0), in order behind the first pass's 64 stores.  The count reached is 0, for
every 128 x 256 instance of the file."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rvc-maker_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# <FM, FN, WM, WN, NI, NP, F16, SA, LF> as mangled
WIDE = ["conv_x6_kernelILi2ELi8ELi4ELi2ELi%dELi3ELb1ELb0ELi%dEE" % (ni, lf) for ni in (3, 6) for lf in (1, 2)]
NARROW = ["conv_x6_kernelILi2ELi4ELi4ELi2ELi%dELi3ELb1ELb0ELi1EE" % ni for ni in (3, 6)]


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
    out = tmp_path_factory.mktemp("x6_build") / "conv1d.s"
    r = subprocess.run([HIPCC, *makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "conv1d.hip"), "-o",
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


@pytest.mark.parametrize("inst", WIDE + NARROW)
def test_default_path_tiles_do_not_spill(remarks, inst):
    hits = [v for k, v in remarks.items() if inst in k]
    assert len(hits) == 1, sorted(remarks)
    r = hits[0]
    print(inst, r)
    assert r["Occupancy [waves/SIMD]"] >= 3
    assert r["VGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0


def test_no_wide_tile_spills(remarks):
    """Every 128 x 256 instance (FN = 8: split-fp16 with the general loaders, split-bf16 at 6, 3 and 1 passes; 47 to 73
    spilled VGPRs before) at 0, still 3 waves per SIMD."""
    wide = {k: v for k, v in remarks.items() if "conv_x6_kernelILi2ELi8ELi4ELi2E" in k}
    assert len(wide) == 12, sorted(wide)
    for k, r in wide.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["Occupancy [waves/SIMD]"] >= 3, (k, r)
