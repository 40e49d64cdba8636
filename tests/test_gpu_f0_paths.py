"""Every f0 route of the conversion path (VC.f0_device: the single methods and hybrids, plain, with autotune and with
an f0 file) and of extraction (FeatureInputAMD.compute_f0) reproduces, bit for bit, what the code before f0.py gave:
tests/golden/f0_paths.npz, recorded by tests/golden/make_golden_f0_paths.py, whose case table and model set-up the test
runs as they are.  The four post kernels (rmvpe, crepe, swipe, and the f64 one of pm / fcpe / hybrids) each quantise
through rvc_common.h's f0_coarse here."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_f0_paths",
                                               os.path.join(HERE, "golden", "make_golden_f0_paths.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLD = np.load(os.path.join(HERE, "golden", "f0_paths.npz"))


@pytest.fixture(scope="module")
def paths():
    np.testing.assert_array_equal(gen.signal(), GOLD["x"])
    return gen.Paths(GOLD["dither"])


@pytest.mark.parametrize("name", gen.case_names())
def test_case_is_reproduced_bit_for_bit(paths, name):
    assert int(GOLD[f"{name}:voiced"]) >= gen.MIN_VOICED  # a voiced track: a wrong shift or override would show
    got = paths.run(name)
    assert set(got) == ({"coarse", "pitchf"} if name.startswith("vc:") else {"f0"})
    for k, v in got.items():
        want = GOLD[f"{name}:{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, (k, v.dtype, v.shape, want.dtype, want.shape)
        assert v.tobytes() == want.tobytes(), (k, int((v != want).sum()))
