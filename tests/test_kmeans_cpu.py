"""CPU-side checks of the IVF training path (csrc/kmeans.hip's argument validation, rvc_amd/index_train.py's host
control and tests/kmeans_ref.py's restatement): no GPU is touched."""
import ctypes

import numpy as np
import pytest

import kmeans_ref as kr
from rvc_amd import _lib, index_train
from rvc_amd.faiss_index import IVFFlatIndex, read_index

P = ctypes.c_void_p(4096)  # a non-null, aligned address: validation fails before anything is read


def last_error():
    return _lib.load().rvc_last_error().decode()


def test_assign_rejects_bad_arguments():
    lib = _lib.load()
    need = lib.rvc_kmeans_assign_work_bytes(100, 8, 4)
    assert need > 0
    assert lib.rvc_kmeans_assign(None, 100, 8, P, 4, P, need, P, P, None) == -22 and "null" in last_error()
    assert lib.rvc_kmeans_assign(P, 100, 8, P, 4, P, need, None, P, None) == -22 and "null" in last_error()
    assert lib.rvc_kmeans_assign(P, 100, 12, P, 4, P, need, P, P, None) == -22 and "d=12" in last_error()
    assert lib.rvc_kmeans_assign(P, 100, 2048, P, 4, P, 1 << 30, P, P, None) == -22 and "d=2048" in last_error()
    assert lib.rvc_kmeans_assign(P, 100, 8, P, 0, P, need, P, P, None) == -22 and "k=0" in last_error()
    assert lib.rvc_kmeans_assign(P, 3, 8, P, 4, P, need, P, P, None) == -22 and "n=3 k=4" in last_error()
    assert lib.rvc_kmeans_assign(P, 100, 8, P, 4, P, need - 1, P, P, None) == -22 and "workspace" in last_error()
    assert lib.rvc_kmeans_assign(ctypes.c_void_p(4100), 100, 8, P, 4, P, need, P, P, None) == -22
    assert "aligned" in last_error()
    assert lib.rvc_kmeans_assign_work_bytes(100, 12, 4) == -1 and lib.rvc_kmeans_assign_work_bytes(0, 8, 1) == -1


def test_lists_update_gather_reject_bad_arguments():
    lib = _lib.load()
    need = lib.rvc_kmeans_lists_work_bytes(100, 4)
    assert need > 0 and lib.rvc_kmeans_lists_work_bytes(100, 0) == -1
    assert lib.rvc_kmeans_lists(None, 100, 4, P, need, P, P, P, None) == -22 and "null" in last_error()
    assert lib.rvc_kmeans_lists(P, 100, 0, P, need, P, P, P, None) == -22 and "k=0" in last_error()
    assert lib.rvc_kmeans_lists(P, 0, 4, P, need, P, P, P, None) == -22 and "n=0" in last_error()
    assert lib.rvc_kmeans_lists(P, 100, 4, P, need - 1, P, P, P, None) == -22 and "workspace" in last_error()
    Q = ctypes.c_void_p(8192)
    assert lib.rvc_kmeans_update(P, 100, 8, P, P, 4, P, None, None) == -22 and "null" in last_error()
    assert lib.rvc_kmeans_update(P, 100, 12, P, P, 4, P, Q, None) == -22 and "d=12" in last_error()
    assert lib.rvc_kmeans_update(P, 100, 8, P, P, 0, P, Q, None) == -22 and "k=0" in last_error()
    assert lib.rvc_kmeans_update(P, 100, 8, P, P, 4, P, P, None) == -22 and "alias" in last_error()
    assert lib.rvc_gather_rows(P, 8, None, 4, Q, None) == -22 and "null" in last_error()
    assert lib.rvc_gather_rows(P, 12, P, 4, Q, None) == -22 and "d=12" in last_error()
    assert lib.rvc_gather_rows(P, 8, P, 0, Q, None) == -22 and "m=0" in last_error()


def test_n_ivf_rule_and_file_names():
    # create_index.py:66: min(int(16 sqrt N), N // 39)
    assert index_train.n_ivf_rule(38) == 0 and index_train.n_ivf_rule(39) == 1
    assert index_train.n_ivf_rule(2000) == 51 and index_train.n_ivf_rule(6000) == 153
    assert index_train.n_ivf_rule(200_000) == 5128 and index_train.n_ivf_rule(100_000) == 2564
    assert index_train.n_ivf_rule(1_000_000) == 16000  # the square-root branch
    assert index_train.index_names(51, "voice", "v2") == ("trained_IVF51_Flat_nprobe_1_voice_v2.index",
                                                          "added_IVF51_Flat_nprobe_1_voice_v2.index")


def test_mt19937_stream_is_the_standard_one():
    # the C++ standard's check value: the 10000th output of a default-constructed std::mt19937 (seed 5489)
    assert int(kr.mt_raw(5489, 10000)[-1]) == 4123659995
    assert int(index_train.mt19937_raw(5489, 10000)[-1]) == 4123659995


@pytest.mark.parametrize("n,seed", [(1, 3), (2, 1235), (7, 1235), (1000, 1235), (5000, 9)])
def test_rand_perm_against_random_raw(n, seed):
    perm = index_train.rand_perm(n, seed)
    assert sorted(perm.tolist()) == list(range(n))
    np.testing.assert_array_equal(perm, kr.rand_perm(n, seed))
    raw = np.random.RandomState(seed)._bit_generator.random_raw(max(n - 1, 1))
    want = np.arange(n)
    for i in range(n - 1):  # the definition, spelled out once more
        j = i + int(raw[i]) % (n - i)
        want[[i, j]] = want[[j, i]]
    np.testing.assert_array_equal(perm, want)


def test_split_plan_matches_restatement():
    counts = np.array([40, 0, 3, 0, 1, 0, 56], np.float32)
    n = int(counts.sum())
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((7, 8)).astype(np.float32)
    ref = cent.copy()
    assert kr.split(ref, counts, n) == 3
    h = counts.copy()
    plan = index_train.split_plan(h, n)
    assert [ci for ci, _ in plan] == [1, 3, 5]
    even = np.arange(8) % 2 == 0
    up = np.where(even, np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)).astype(np.float32)
    dn = np.where(even, np.float32(1 - 1 / 1024), np.float32(1 + 1 / 1024)).astype(np.float32)
    for ci, cj in plan:
        src = cent[cj].copy()
        cent[ci], cent[cj] = src * up, src * dn
    np.testing.assert_array_equal(cent, ref)
    assert h.sum() == n and (h > 0).all()
    assert index_train.split_plan(np.array([3, 4, 5], np.float32), 12) == []


def test_restated_lloyd_step_does_not_raise_the_objective():
    x = kr.clustered(1200, 24, 20, seed=4)
    cent = x[kr.rand_perm(len(x), 1235)[:20]].copy()
    prev = np.inf
    for _ in range(6):
        cent, assign, obj, nsplit = kr.lloyd_step(x, cent)
        assert nsplit == 0  # split-free: Lloyd's monotonicity applies
        assert obj <= prev * (1 + 1e-12)
        prev = obj
    assert kr.objective(x, cent, kr.dist64(x, cent).argmin(1)) <= prev * (1 + 1e-6)  # f32 means: rounding only


def test_trained_and_added_pair_round_trips(tmp_path):
    x = kr.clustered(300, 256, 7, seed=1)
    cent = x[:7].copy()
    off, ids = kr.lists(kr.dist64(x, cent).argmin(1), 7)
    cut = off[1:-1]
    added = IVFFlatIndex(256, cent, np.split(x[ids], cut), np.split(ids, cut), nprobe=1, ntotal=300)
    trained = IVFFlatIndex(256, cent, [np.zeros((0, 256), np.float32)] * 7, [np.zeros(0, np.int64)] * 7, ntotal=0)
    names = index_train.index_names(7, "m", "v1")
    trained.write(str(tmp_path / names[0]))
    added.write(str(tmp_path / names[1]))
    t, a = read_index(str(tmp_path / names[0])), read_index(str(tmp_path / names[1]))
    assert (t.ntotal, t.nlist, t.nprobe, t.d) == (0, 7, 1, 256) and all(len(i) == 0 for i in t.ids)
    np.testing.assert_array_equal(t.centroids, cent)
    assert (a.ntotal, a.nlist, a.nprobe) == (300, 7, 1)
    np.testing.assert_array_equal(a.centroids, cent)
    for li in range(7):
        np.testing.assert_array_equal(a.ids[li], added.ids[li])
        np.testing.assert_array_equal(a.codes[li], added.codes[li])
    np.testing.assert_array_equal(a.reconstruct_n(0, 300), x)


def test_create_index_refuses_the_minibatch_reduction(tmp_path, monkeypatch):
    """N > 2e5 under "Auto" / "KMeans" is the reference's MiniBatchKMeans reduction: refused by name, before any
    row is copied (the loader is patched with a broadcast view: nothing of that size is allocated)."""
    big = np.broadcast_to(np.zeros((1, 768), np.float32), (200_001, 768))
    monkeypatch.setattr(index_train, "load_features", lambda exp_dir, version: big)
    for algo in ("Auto", "KMeans"):
        with pytest.raises(NotImplementedError, match="MiniBatchKMeans") as e:
            index_train.create_index(str(tmp_path), "v2", algo, device="cpu")
        assert 'index_algorithm="Faiss"' in str(e.value)
    assert not list(tmp_path.iterdir())


def test_create_index_rejects_too_few_rows_and_wrong_width(tmp_path, monkeypatch):
    monkeypatch.setattr(index_train, "load_features", lambda exp_dir, version: np.zeros((38, 768), np.float32))
    with pytest.raises(ValueError, match="n_ivf = 0"):
        index_train.create_index(str(tmp_path), "v2", device="cpu")
    with pytest.raises(ValueError, match="256"):
        index_train.create_index(str(tmp_path), "v1", device="cpu")
    assert not list(tmp_path.iterdir())  # refused before total_fea.npy is written


def test_kmeans_rejects_host_tensors():
    import torch
    with pytest.raises(TypeError):
        index_train.kmeans(torch.zeros(10, 8), 2)
