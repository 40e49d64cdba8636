"""swipe f0, the parts that need no device: the library's host-built tables against numpy / scipy, the numpy
restatement (tests/swipe_ref.py) against the reference's own f0 (tests/golden/swipe.npz, written by
tests/golden/make_golden_swipe.py), the size queries, argument checks and the hybrid[...] parser."""
import ctypes
import os

import numpy as np
import pytest

import swipe_ref
from rvc_amd import _lib, f0mix, swipe

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swipe.npz"))
NAMES = sorted(k[2:] for k in GOLD.files if k.startswith("x_"))


@pytest.fixture(scope="module")
def lib_tables():
    return swipe.host_tables()[1]


def test_small_tables_match_numpy(lib_tables):
    pc, ferbs, per = swipe_ref.tables()
    np.testing.assert_allclose(lib_tables(swipe.T_PC), pc, rtol=1e-15, atol=0)
    np.testing.assert_allclose(lib_tables(swipe.T_FERBS), ferbs, rtol=1e-15, atol=0)
    assert [len(t["idx"]) for t in per] == [127, 192, 192, 192, 110]
    cmap, cmu = lib_tables(swipe.T_CMAP).reshape(429, 2, 2), lib_tables(swipe.T_CMU)
    served = np.zeros(429, int)
    for i, t in enumerate(per):
        np.testing.assert_array_equal(lib_tables(swipe.T_IDX, i), t["idx"])
        np.testing.assert_allclose(lib_tables(swipe.T_MU, i), t["mu"], rtol=1e-15, atol=0)
        win = lib_tables(swipe.T_WIN, i)
        assert win.shape == (t["ws"] + 1,)
        np.testing.assert_allclose(win[:-1], np.hanning(t["ws"] + 2)[1:-1], rtol=0, atol=1e-15)
        np.testing.assert_allclose(win[-1], np.hanning(t["ws"] + 2)[1:-1].sum(), rtol=1e-14)
        # the per-candidate map the sum stage gathers through: the same (window, index, mu), in window order
        for l, c in enumerate(t["idx"]):
            slot = served[c]
            assert tuple(cmap[c, slot]) == (i, l) and cmu[c, slot] == lib_tables(swipe.T_MU, i)[l]
            served[c] += 1
    assert served.min() >= 1 and served.max() == 2
    assert (cmap[served == 1, 1] == -1).all()
    k = np.arange(1024)
    tw = lib_tables(swipe.T_TW)
    np.testing.assert_allclose(tw[:, 0] + 1j * tw[:, 1], np.exp(-2j * np.pi * k / 2048), rtol=0, atol=1e-15)


@pytest.mark.parametrize("i", range(5))
def test_spline_and_kernel_matrices_match_scipy(lib_tables, i):
    """W_i against scipy's not-a-knot cubic interp1d of the identity (1e-12 abs); K_i against the numpy kernels
    (1e-14 abs); the padding the GEMMs read is zero."""
    t = swipe_ref.tables()[2][i]
    W = lib_tables(swipe.T_W, i)
    assert W.shape == t["W"].shape
    assert np.abs(W - t["W"]).max() <= 1e-12
    K = lib_tables(swipe.T_K, i)
    assert K.shape == t["K"].shape
    assert np.abs(K - t["K"]).max() <= 1e-14
    assert not lib_tables(swipe.T_W, i, padded=True)[:, W.shape[1]:].any()
    assert not lib_tables(swipe.T_K, i, padded=True)[:, K.shape[1]:].any()
    # the copies the kernels read, in MFMA operand order: [row tile][K / 16][lane][u] =
    # M[16 tile + (lane & 15)][4 (4 k16 + u) + (lane >> 4)] over the zero-padded matrix
    lane, u = np.arange(64)[:, None], np.arange(4)[None, :]
    for plain, packed in ((swipe.T_W, swipe.T_WP), (swipe.T_K, swipe.T_KP)):
        M = lib_tables(plain, i, padded=True)
        rows = -(-M.shape[0] // 16) * 16
        M = np.vstack([M, np.zeros((rows - M.shape[0], M.shape[1]))])
        Kd = M.shape[1]
        got = lib_tables(packed, i).reshape(rows // 16, Kd // 16, 64, 4)
        for tile in (0, rows // 16 - 1):
            for k16 in (0, Kd // 16 - 1):
                want = M[16 * tile + (lane & 15), 4 * (4 * k16 + u) + (lane >> 4)]
                np.testing.assert_array_equal(got[tile, k16], want)
        assert np.sort(got.ravel()).tobytes() == np.sort(M.ravel()).tobytes()  # a permutation of the matrix


def test_pick_grids_match_numpy(lib_tables):
    pc = swipe_ref.tables()[0]
    px, gx, gf = lib_tables(swipe.T_PX), lib_tables(swipe.T_GRIDX), lib_tables(swipe.T_GRIDF0)
    for i in (1, 2, 200, 427):
        tc = 1 / pc[i - 1:i + 2]
        ntc = (tc / tc[1] - 1) * 2 * np.pi
        np.testing.assert_allclose(px[i], ntc[[0, 2]], rtol=1e-12)
        lo = np.log2(pc[i - 1])
        grid = 2 ** np.arange(lo, np.log2(pc[i + 1]) + 1 / 12 / 64, 1 / 12 / 64)[:17]
        np.testing.assert_allclose(gx[i], ((1 / grid) / tc[1] - 1) * 2 * np.pi, rtol=0, atol=1e-14)
        np.testing.assert_array_equal(gf[i], (2 ** (lo + np.arange(17) / 12 / 64)).astype(np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference_f0(name):
    """tests/swipe_ref.py (f64 matrix form) gives the reference's f0 on every frame of every fixture."""
    x, want = GOLD["x_" + name], GOLD["f0_" + name]
    got = swipe_ref.f0(x)
    assert got.dtype == np.float32 and got.shape == want.shape == (len(x) // 160 + 1,)
    np.testing.assert_array_equal(got, want)
    if name in ("noise", "silence"):
        assert not want.any()


def test_frames_and_work_queries():
    lib = _lib.load()
    for n in (400, 16000, 160000 + 37, 480000):
        assert lib.rvc_swipe_frames(n) == n // 160 + 1
        assert lib.rvc_swipe_work_bytes(n) > 0
    assert lib.rvc_swipe_frames(0) == -1 and lib.rvc_swipe_work_bytes(0) == -1
    assert lib.rvc_swipe_tables_bytes() > 0


def test_entry_points_reject_null_arguments():
    lib = _lib.load()
    dims = (ctypes.c_int64 * 3)()
    assert lib.rvc_swipe_tables(None, 1 << 30) == -22
    assert b"null" in lib.rvc_last_error()
    small = np.zeros(16, np.uint8)
    assert lib.rvc_swipe_tables(ctypes.c_void_p(small.ctypes.data), small.nbytes) == -22
    assert lib.rvc_swipe_table_dims(swipe.T_W, 0, None) == -22
    assert lib.rvc_swipe_table_dims(99, 0, dims) == -22
    assert lib.rvc_swipe_table_dims(swipe.T_W, 5, dims) == -22
    assert lib.rvc_swipe_strength(None, 16000, None, None, 0, None, None) == -22
    assert lib.rvc_swipe_pick(None, 10, None, None, None) == -22
    assert lib.rvc_swipe_post(None, 10, 1.0, None, None, None, None) == -22
    assert lib.rvc_abs_quantile(None, 10, None, 0, None, None) == -22
    assert lib.rvc_abs_quantile_work_bytes() > 0
    assert lib.rvc_div_scalar(None, 10, None, None, None) == -22
    assert lib.rvc_f0_mix(None, 1, 10, None, None) == -22
    one = (_lib.F0Track * 1)()
    out = np.zeros(4)
    assert lib.rvc_f0_mix(one, 1, 4, ctypes.c_void_p(out.ctypes.data), None) == -22  # an empty track
    assert lib.rvc_f0_mix(one, 9, 4, ctypes.c_void_p(out.ctypes.data), None) == -22
    assert b"tracks" in lib.rvc_last_error()


def test_hybrid_parser():
    assert f0mix.parse_hybrid("hybrid[rmvpe+swipe]") == ["rmvpe", "swipe"]
    assert f0mix.parse_hybrid("hybrid[ pm + crepe-tiny +pm ]") == ["pm", "crepe-tiny", "pm"]
    assert f0mix.parse_hybrid("hybrid[swipe]") == ["swipe"]
    assert f0mix.is_hybrid("hybrid[swipe]") and not f0mix.is_hybrid("swipe")
    with pytest.raises(NotImplementedError, match="harvest"):
        f0mix.parse_hybrid("hybrid[rmvpe+harvest]")
    with pytest.raises(NotImplementedError, match="fcpe"):
        f0mix.parse_hybrid("hybrid[fcpe+swipe]")
    with pytest.raises(ValueError):
        f0mix.parse_hybrid("hybrid")
