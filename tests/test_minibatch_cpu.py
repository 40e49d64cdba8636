"""CPU-side checks of the MiniBatchKMeans reduction (csrc/minibatch.hip's argument validation, rvc_amd/index_train.py's
host rules, tests/minibatch_ref.py's restatement against the fixtures recorded from sklearn, and against sklearn live
where it is installed): no GPU is touched."""
import ctypes

import numpy as np
import pytest

import minibatch_ref as mr
from rvc_amd import _lib, index_train

P = ctypes.c_void_p(4096)  # a non-null, aligned address: validation fails before anything is read


def last_error():
    return _lib.load().rvc_last_error().decode()


@pytest.fixture(scope="module", params=sorted(mr.CASES))
def case(request):
    fx = mr.load_fixture(request.param)
    n, d, k, batch_size = mr.CASES[request.param]
    assert fx["x"].shape == (n, d) and fx["x"].dtype == np.float32
    assert (int(fx["n_clusters"]), int(fx["batch_size"])) == (k, batch_size)
    cent, hist = mr.fit(fx["x"], k, batch_size, int(fx["seed"]))
    return request.param, fx, cent, hist


def test_fixture_rows_are_the_stated_blobs(case):
    name, fx, _, _ = case
    n, d, _, _ = mr.CASES[name]
    np.testing.assert_array_equal(fx["x"], mr.blobs(n, d, mr.DATA_SEED[name]))
    assert str(fx["sklearn_version"]) and str(fx["numpy_version"])


def test_restatement_equals_the_fixture(case):
    """Centres bit for bit with sklearn's, equal n_steps, and the recorded history step by step."""
    name, fx, cent, hist = case
    np.testing.assert_array_equal(cent.view(np.uint32), fx["sk_centres"].view(np.uint32))
    assert hist["n_steps"] == int(fx["sk_n_steps"]) == len(fx["inertia"])
    np.testing.assert_array_equal(hist["init"].view(np.uint32), fx["init"].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(hist["batch"]), fx["batch"])
    np.testing.assert_array_equal(np.asarray(hist["labels"]), fx["labels"])
    np.testing.assert_array_equal(np.asarray(hist["inertia"]), fx["inertia"])
    np.testing.assert_array_equal(np.asarray(hist["reassign"]), fx["reassign"])
    np.testing.assert_array_equal(np.concatenate(hist["to"]), fx["to"])
    np.testing.assert_array_equal(np.concatenate(hist["picked"]), fx["picked"])
    np.testing.assert_array_equal([len(t) for t in hist["to"]], np.diff(fx["to_off"]))
    assert hist["min_ewa_gap"] > 1e-6  # what the maker selected the seed for
    assert bool(fx["free_run_exact"]) == (min(hist["gap_tol"]) >= 4.0)


def test_fixtures_cover_what_they_are_for():
    a, b, c = (mr.load_fixture(name) for name in "ABC")
    assert b["batch"].shape[1] == 2000  # B: the batch clamped to n, no init subsample
    assert mr.sizes(2000, 10, 4096) == (2000, 2000, 100)
    assert mr.CASES["C"][2] > mr.CASES["C"][3] and len(c["to"]) >= 100  # C: k > batch, hundreds of reassignments
    assert len(a["to"]) >= 1
    assert bool(b["free_run_exact"])  # the free-running GPU test needs one such case
    q = mr.load_fixture("Q")
    assert q["sk_inertia"].shape == (8,) and (q["sk_inertia"] > 0).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_equals_sklearn_live(name):
    pytest.importorskip("sklearn")
    from sklearn.cluster import MiniBatchKMeans
    fx = mr.load_fixture(name)
    n, d, k, batch_size = mr.CASES[name]
    sk = MiniBatchKMeans(n_clusters=k, batch_size=batch_size, compute_labels=False, init="random",
                         random_state=int(fx["seed"])).fit(fx["x"])
    cent, hist = mr.fit(fx["x"], k, batch_size, int(fx["seed"]))
    np.testing.assert_array_equal(cent.view(np.uint32), sk.cluster_centers_.view(np.uint32))
    assert hist["n_steps"] == sk.n_steps_


def test_update_is_sequential_f32_with_the_product_rounded_on_its_own():
    """A hand-made centre whose product centre * weight is inexact: an fma with the first add would differ."""
    cent, w, xb = mr.fma_case()
    new, nw = mr.update(xb, [0, 0], cent, w)
    # f32(1/3) * 3 = 1 + 2^-25 exactly, which rounds to 1; + 0.75 * 2^-24 stays 1.  One rounding of the exact sum
    # 1 + 1.25 * 2^-24 would give 1 + 2^-23 instead.
    assert np.float32(np.float64(cent[0, 0]) * 3.0 + np.float64(xb[0, 0])) == np.float32(1.0 + 2.0 ** -23)
    assert nw[0] == 5 and (new[0] == np.float32(1.0) * (np.float32(1) / np.float32(5))).all()
    assert (new[1] == cent[1]).all() and nw[1] == 0  # no member: copied


def test_sizes_follow_sklearn():
    assert index_train.minibatch_sizes(3000, 40, 256) == mr.sizes(3000, 40, 256) == (256, 768, 1171)
    assert index_train.minibatch_sizes(20000, 200, 64) == mr.sizes(20000, 200, 64) == (64, 600, 31250)
    assert index_train.minibatch_sizes(250000, 10000, 2048) == (2048, 30000, 12207)


def test_random_state_rules():
    assert index_train._random_state(None) is np.random.mtrand._rand
    rs = np.random.RandomState(3)
    assert index_train._random_state(rs) is rs
    assert index_train._random_state(7).randint(0, 1000) == np.random.RandomState(7).randint(0, 1000)
    with pytest.raises(TypeError, match="RandomState"):
        index_train._random_state(np.random.default_rng(0))


def test_minibatch_kmeans_rejects_host_tensors():
    import torch
    with pytest.raises(TypeError, match="CUDA"):
        index_train.minibatch_kmeans(torch.zeros(100, 8), 4, 32, 0)


def test_n_ivf_of_the_reduced_rows():
    assert index_train.n_ivf_rule(10000) == 256
    assert index_train.index_names(256, "voice", "v2")[1] == "added_IVF256_Flat_nprobe_1_voice_v2.index"


def test_create_index_reduction_refuses_a_host_device(tmp_path, monkeypatch):
    """Above reduce_rows the reduction runs on the device only: device="cpu" is refused by name before any copy, at
    the reference's threshold and at a lowered one."""
    big = np.broadcast_to(np.zeros((1, 768), np.float32), (200_001, 768))
    monkeypatch.setattr(index_train, "load_features", lambda exp_dir, version: big)
    with pytest.raises(NotImplementedError, match="MiniBatchKMeans") as e:
        index_train.create_index(str(tmp_path), "v2", "Auto", device="cpu")
    assert 'index_algorithm="Faiss"' in str(e.value) and "on the device only" in str(e.value)
    monkeypatch.setattr(index_train, "load_features", lambda exp_dir, version: big[:3000])
    with pytest.raises(NotImplementedError, match="on the device only"):
        index_train.create_index(str(tmp_path), "v2", "KMeans", device="cpu", reduce_rows=1000, reduce_to=400)
    assert not list(tmp_path.iterdir())


def test_create_index_reduction_takes_a_randomstate_only(tmp_path, monkeypatch):
    """The reduction draws from the RandomState that shuffles: a Generator is a TypeError naming RandomState, raised
    before anything is copied or written (the device is never reached)."""
    big = np.broadcast_to(np.zeros((1, 256), np.float32), (3000, 256))
    monkeypatch.setattr(index_train, "load_features", lambda exp_dir, version: big)
    with pytest.raises(TypeError, match="RandomState"):
        index_train.create_index(str(tmp_path), "v1", rng=np.random.default_rng(0), reduce_rows=1000, reduce_to=400)
    with pytest.raises(ValueError, match="reduce_to"):
        index_train.create_index(str(tmp_path), "v1", rng=np.random.RandomState(0), reduce_rows=1000, reduce_to=38)
    assert not list(tmp_path.iterdir())


def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    assert lib.rvc_minibatch_status_bytes() == 32 and index_train.ops.MINIBATCH_STATUS.itemsize == 32
    need = lib.rvc_kmeans_assign_work_bytes(3, 8, 4)
    assert need > 0
    assert lib.rvc_minibatch_assign(None, 3, 8, P, 4, P, need, P, P, None) == -22 and "null" in last_error()
    assert lib.rvc_minibatch_assign(P, 3, 12, P, 4, P, need, P, P, None) == -22 and "d=12" in last_error()
    assert lib.rvc_minibatch_assign(P, 0, 8, P, 4, P, need, P, P, None) == -22 and "n=0" in last_error()
    assert lib.rvc_minibatch_assign(P, 3, 8, P, 4, P, need - 1, P, P, None) == -22 and "workspace" in last_error()
    assert lib.rvc_minibatch_update(P, 64, 8, P, P, 4, P, None, P, None) == -22 and "null" in last_error()
    assert lib.rvc_minibatch_update(P, 64, 20, P, P, 4, P, P, ctypes.c_void_p(8192), None) == -22
    assert "d=20" in last_error()
    assert lib.rvc_minibatch_update(P, 64, 8, P, P, 0, P, P, ctypes.c_void_p(8192), None) == -22 and "k=0" in last_error()
    assert lib.rvc_minibatch_update(P, 64, 8, P, P, 4, P, P, P, None) == -22 and "alias" in last_error()
    assert lib.rvc_minibatch_update(P, 64, 8, P, P, 4, ctypes.c_void_p(4100), P, P, None) == -22
    assert "aligned" in last_error()
    assert lib.rvc_minibatch_inertia_work_bytes(64) == 512 and lib.rvc_minibatch_inertia_work_bytes(0) == -1
    assert lib.rvc_minibatch_inertia(P, 64, 8, P, 4, None, P, P, 512, P, None) == -22 and "null" in last_error()
    assert lib.rvc_minibatch_inertia(P, 64, 8, P, 4, P, None, P, 511, P, None) == -22 and "workspace" in last_error()
    assert lib.rvc_minibatch_inertia(P, 64, 8, P, 4, P, None, P, 512, ctypes.c_void_p(4100), None) == -22
    assert "aligned" in last_error()
    assert lib.rvc_minibatch_scatter(P, 64, 8, None, P, 2, 1.0, P, 4, P, None) == -22 and "null" in last_error()
    assert lib.rvc_minibatch_scatter(P, 64, 8, P, P, 5, 1.0, P, 4, P, None) == -22 and "m=5" in last_error()
    assert lib.rvc_minibatch_scatter(P, 64, 8, P, P, 0, 1.0, P, 4, P, None) == -22 and "m=0" in last_error()
