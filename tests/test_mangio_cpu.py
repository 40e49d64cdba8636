"""mangio-crepe-* and rmvpe-legacy without a device: the names every holder takes, the numpy restatement
(tests/mangio_ref.py) against the reference's recorded output (tests/golden/mangio.npz, make_golden_mangio.py), the two
input scales against NumPy and torch themselves, and the new C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mangio_ref
from rvc_amd import _lib, f0, f0mix
from rvc_amd.extract import FeatureInputAMD
from rvc_amd.pipeline import VC, Config

HOPS = (37, 64, 160, 512)
MANGIO = tuple(f"mangio-crepe-{c}" for c in ("tiny", "small", "medium", "large", "full"))
NEW = MANGIO + ("rmvpe-legacy",)


def holders():
    return VC(40000, Config("cpu")), FeatureInputAMD(device="cpu")


# ------------------------------------------------------------------ names
def test_tables():
    assert tuple(f0.MANGIO_METHODS) == MANGIO and f0.MANGIO_METHODS["mangio-crepe-small"] == "small"
    assert tuple(f0.CREPE_METHODS) == tuple(m[len("mangio-"):] for m in MANGIO)  # still the five crepe-*
    assert "rmvpe-legacy" in f0.METHODS and VC.MANGIO_METHODS is f0.MANGIO_METHODS
    for name in ("rmvpe-legacy", "mangio-crepe-*"):
        assert name in f0.ON_PATH


@pytest.mark.parametrize("method", NEW)
def test_holders_accept_the_method_alone_and_as_a_member(method, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # no assets/: nothing may go to a model file, let alone a device
    for h in holders():
        h.check_f0_method(method)
        h.check_f0_method(f"hybrid[{method}+swipe]")
        assert h.f0_members(f"hybrid[pm + {method}+{method}]") == ["pm", method, method]
        assert h.rmvpe is None and h.crepe == {}
    assert f0mix.parse_hybrid(f"hybrid[{method}+rmvpe]") == [method, "rmvpe"]


def test_unknown_capacity_is_still_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    vc, fi = holders()
    xt = torch.zeros(16000)  # a host tensor: the refusal comes before anything touches a device
    for call in (lambda: vc.f0_device(xt, 0, "hybrid[mangio-crepe-huge]"),
                 lambda: vc.f0_device(xt, 0, "mangio-crepe-huge"),
                 lambda: fi.compute_f0(np.zeros(16000, np.float32), "hybrid[rmvpe+mangio-crepe-huge]"),
                 lambda: f0mix.parse_hybrid("hybrid[mangio-crepe-huge]"),
                 lambda: vc.f0_raw(xt, "rmvpe-legacy-2", 100)):
        with pytest.raises(NotImplementedError, match="huge|legacy-2") as e:
            call()
        assert "mangio-crepe-*" in str(e.value) and "rmvpe-legacy" in str(e.value)


def test_hop_length_below_one_raises():
    from rvc_amd.crepe import CrepeAMD
    m = object.__new__(CrepeAMD)  # the check comes before any model or device use
    for hop in (0, -3):
        with pytest.raises(ValueError, match="hop_length"):
            m.f0_mangio(torch.zeros(1600), hop, 10)
        with pytest.raises(ValueError, match="hop_length"):
            m.decode_mangio(torch.zeros(360, 11), hop, 10)


# ------------------------------------------------------------------ restatement vs the reference's recorded output
@pytest.mark.parametrize("hop", HOPS)
def test_restatement_matches_reference(golden, hop):
    """mangio_ref fed the recorded probabilities and dither, against the recorded bins and f0, exactly.  bins -> Hz is
    evaluated as ``predict`` evaluates it, one torch call per batch: torch sends whole vector blocks through its vector
    pow and each call's tail through the C library's powf, so this form is the reference on a host like the one that
    recorded the golden (16-lane vectors)."""
    g = golden("mangio")
    probs, dither = g[f"probs_{hop}"], g[f"dither_{hop}"]
    assert probs.shape == (1 + 12040 // hop, 360) and probs.dtype == np.float32
    assert g[f"batches_{hop}"].tolist() == np.diff(mangio_ref.segments(len(probs), hop)).tolist()
    bins, source = mangio_ref.postprocess(probs, hop, dither)
    np.testing.assert_array_equal(bins, g[f"bins_{hop}"])
    out = mangio_ref.resample(source, 75)
    assert out.dtype == np.float64
    np.testing.assert_array_equal(out, g[f"f0_{hop}"])


@pytest.mark.parametrize("hop", HOPS)
def test_vector_form_differs_only_on_batch_tails(golden, hop):
    """The host-independent form of bins -> Hz (every frame through the vector routine: what the device computes)
    against the per-batch torch form.  They may differ only on frames torch leaves to the C library -- the last
    n mod 32 of a batch of n on a 16-lane host, n mod 16 on an 8-lane one -- and there by one ulp.  At hops 37 and 64,
    where the GPU tests ask for every bit, the golden's track is the same in both forms (make_golden_mangio.py refuses
    to write it otherwise); at hop 160 one tail frame differs on the recording host, which is why that hop is held to
    a tolerance."""
    g = golden("mangio")
    bins, dither = g[f"bins_{hop}"], g[f"dither_{hop}"]
    seg = mangio_ref.segments(len(bins), hop)
    per_batch = mangio_ref.bins_to_hz(bins, dither, seg)
    vector = mangio_ref.bins_to_hz(bins, dither, seg, vector=True)
    assert per_batch.dtype == vector.dtype == np.float32
    tail = np.zeros(len(bins), bool)
    for a, b in zip(seg[:-1], seg[1:]):
        tail[b - (b - a) % 32: b] = True  # the widest tail of the two vector widths
    differ = per_batch != vector
    assert not differ[~tail].any()
    assert (np.abs(per_batch.view(np.int32) - vector.view(np.int32)) <= 1).all()
    if hop in (37, 64):
        np.testing.assert_array_equal(mangio_ref.resample(vector, 75), g[f"f0_{hop}"])


def test_pow2_vector_is_torchs_vector_path():
    """mangio_ref.pow2_vector against torch itself: equal in every bit wherever torch uses its vector routine (the
    tensor padded by two vector blocks, one thread, so that every compared element lies in a whole block), and one ulp
    from torch's scalar path on some values (one-element tensors never reach the vector routine)."""
    rng = np.random.default_rng(3)
    y = rng.uniform(1.5, 7.8, 100000).astype(np.float32)
    n0 = torch.get_num_threads()
    torch.set_num_threads(1)  # a thread's chunk has a scalar tail of its own
    try:
        padded = torch.from_numpy(np.concatenate([y, np.full(64, 2.0, np.float32)]))
        want = torch.pow(2, padded).numpy()[: len(y)]
    finally:
        torch.set_num_threads(n0)
    got = mangio_ref.pow2_vector(y)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), int((got != want).sum())
    scalar = np.array([float(torch.pow(2, torch.tensor([v]))[0]) for v in y[:4000]], np.float32)
    ulps = np.abs(scalar.view(np.int32) - got[:4000].view(np.int32))
    assert ulps.max() == 1 and 0 < (ulps > 0).mean() < 0.1


def test_golden_shows_the_batch_restart(golden):
    """Without this a decode that never restarted the Viterbi would pass: at hops 37 and 64 one segment over the whole
    track gives other bins than the reference's per-batch decode."""
    g = golden("mangio")
    for hop in (37, 64):
        probs = g[f"probs_{hop}"]
        whole = mangio_ref.viterbi_bins(probs, [0, len(probs)])
        assert (whole != g[f"bins_{hop}"]).sum() >= 100
        assert len(set(g[f"bins_{hop}"].tolist())) >= 2
    for hop in (160, 512):
        assert len(g[f"batches_{hop}"]) == 1


def test_get_f0_variants_follow_from_the_track(golden):
    """get_f0's (coarse, pitchf) for the three variants is the oracle's tail on the recorded hop-64 track."""
    g = golden("mangio")
    for name, (pitch, autotune, strength, f0_file) in mangio_ref.variants().items():
        coarse, pitchf = mangio_ref.get_f0(g["f0_64"], pitch, strength if autotune else None, f0_file)
        np.testing.assert_array_equal(coarse, g[f"vc:{name}:coarse"])
        np.testing.assert_array_equal(pitchf, g[f"vc:{name}:pitchf"])


def test_legacy_golden_is_plain_with_the_range_filter(golden):
    g = golden("rmvpe_legacy")
    plain, legacy = g["plain"], g["legacy"]
    out = (plain < 50) | (plain > 1100)
    np.testing.assert_array_equal(legacy, np.where(out, 0.0, plain))
    assert ((plain > 0) & (plain < 50)).sum() >= 5 and (plain > 1100).sum() >= 5 and np.count_nonzero(legacy) >= 10
    assert min(np.abs(plain - 50).min(), np.abs(plain - 1100).min()) > 0.1
    np.testing.assert_array_equal(g["fi_f0"], legacy)


# ------------------------------------------------------------------ the two scales
def _vectors():
    rng = np.random.default_rng(20)
    for i in range(100):
        n = int(rng.integers(2, 30000)) if i else 1
        yield (rng.standard_normal(n) * rng.uniform(0.01, 3)).astype(np.float32)


def test_scales_match_numpy_and_torch_bit_for_bit():
    differ = 0
    for x in _vectors():
        c, e = mangio_ref.scale_convert(x), mangio_ref.scale_extract(x)
        want_c = np.quantile(np.abs(x), 0.999)
        want_e = torch.quantile(torch.abs(torch.from_numpy(x)), 0.999).numpy()
        assert want_c.dtype == np.float32 and want_e.dtype == np.float32
        assert c.tobytes() == want_c.tobytes(), (x.size, c, want_c)
        assert e.tobytes() == want_e.tobytes(), (x.size, e, want_e)
        differ += c.tobytes() != e.tobytes()
    assert differ <= 10  # they agree nearly always, not always: see test_the_two_scales_are_not_the_same


def test_the_two_scales_are_not_the_same():
    """A vector on which NumPy's lerp and torch's fused one round apart (found by search over seeds)."""
    rng = np.random.default_rng(0)
    for _ in range(3000):
        n = int(rng.integers(5, 3000))
        x = (rng.standard_normal(n) * rng.uniform(0.01, 3)).astype(np.float32)
        c, e = mangio_ref.scale_convert(x), mangio_ref.scale_extract(x)
        if c.tobytes() != e.tobytes():
            assert c.tobytes() == np.quantile(np.abs(x), 0.999).tobytes()
            assert e.tobytes() == torch.quantile(torch.abs(torch.from_numpy(x)), 0.999).numpy().tobytes()
            assert abs(float(c) - float(e)) <= np.spacing(np.float32(max(c, e)))
            return
    pytest.fail("no vector found on which the two scales differ")


# ------------------------------------------------------------------ ABI
NEW_SYMBOLS = ("rvc_f0_resample_nan", "rvc_rmvpe_decode_range", "rvc_abs_quantile_as", "rvc_crepe_decode_as")


def test_new_symbols_are_declared_exported_and_bound():
    from test_abi import declared_symbols
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared_symbols() and hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rvc_rmvpe_decode_range"]) == len(_lib.SIGNATURES["rvc_rmvpe_decode"]) + 2
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include", "rvc_amd.h")).read()
    for text in ("rvc_f0_resample_nan", "rvc_rmvpe_decode_range", "mangio-crepe", "keeps these three f0 methods"):
        assert text in header


def test_null_arguments_are_einval_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: every case fails its argument check first
    inf = float("inf")
    assert lib.rvc_f0_resample_nan(None, 10, 10, one, None) == -22 and b"null" in lib.rvc_last_error()
    assert lib.rvc_f0_resample_nan(one, 10, 10, None, None) == -22
    assert lib.rvc_f0_resample_nan(one, 0, 10, one, None) == -22 and b"length" in lib.rvc_last_error()
    assert lib.rvc_f0_resample_nan(one, 10, 0, one, None) == -22
    assert lib.rvc_rmvpe_decode_range(None, 96, 76, 0.03, 50.0, 1100.0, 1.0, None, None, one, one, None) == -22
    assert lib.rvc_rmvpe_decode_range(one, 96, 76, 0.03, 50.0, 1100.0, 1.0, None, None, None, one, None) == -22
    assert lib.rvc_rmvpe_decode_range(one, 96, 76, 0.03, float("nan"), inf, 1.0, None, None, one, one, None) == -22
    assert b"NaN" in lib.rvc_last_error()
    assert lib.rvc_rmvpe_decode(None, 96, 76, 0.03, 1.0, None, None, one, one, None) == -22
    assert lib.rvc_abs_quantile_as(None, 10, 1, one, 1 << 20, one, None) == -22
    assert lib.rvc_crepe_decode_as(one, 10, 0, 360, one, 1, one, 0.0, 0.0, one, 2, one, 1 << 30, one, one, None) == -22
    assert b"bins -> Hz" in lib.rvc_last_error()
    assert lib.rvc_crepe_decode_as(None, 10, 0, 360, one, 1, one, 0.0, 0.0, one, 1, one, 1 << 30, one, one, None) == -22
    assert lib.rvc_abs_quantile_as(one, 10, 2, one, 1 << 20, one, None) == -22 and b"lerp" in lib.rvc_last_error()
