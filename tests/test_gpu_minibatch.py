"""The MiniBatchKMeans reduction on the device (csrc/minibatch.hip, rvc_amd/index_train.py) against the NumPy
restatement tests/minibatch_ref.py and the fixtures recorded from sklearn (tests/golden/minibatch_*.npz): the update
bit for bit, the f64 inertia, the assignment with more centres than rows, the scatter, one step at the real widths,
the trainer teacher-forced per step and free-running, the quality of its centres, and create_index end to end."""
import os

import numpy as np
import pytest
import torch

import kmeans_ref as kr
import minibatch_ref as mr
from rvc_amd.faiss_index import read_index

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (batch, d, k, every row in one centre)
SHAPES = [(1000, 24, 257, False), (1003, 768, 12, False), (1003, 8, 5, True), (64, 768, 300, False)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_step(n, d, k, one_centre, seed=0):
    """(batch rows, centres, weights, labels): some centres of weight 0, some without a member (a weight-0 one
    among them, and one with members), integer weights up to 2^20."""
    rng = np.random.default_rng(seed + n + d + k)
    xb = kr.clustered(n, d, 20, seed=seed + d)
    cent = (xb[rng.integers(0, n, k)] + 0.05 * rng.standard_normal((k, d))).astype(np.float32)
    w = rng.integers(1, 1 << 20, k).astype(np.float32)
    w[rng.integers(0, k, max(2, k // 4))] = 0
    w[0], w[1], w[k - 1] = 0, 1 << 20, 0
    if one_centre:
        labels = np.full(n, 1, np.int32)
    else:
        used = np.setdiff1d(np.arange(k), [k - 1, k // 2])  # k - 1 (weight 0) and k // 2 get no member
        labels = used[rng.integers(0, len(used), n)].astype(np.int32)
        labels[:3] = 0  # members in a weight-0 centre
    return xb, cent, w, labels


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}k{s[2]}")
def step_case(request):
    n, d, k, one = request.param
    xb, cent, w, labels = make_step(n, d, k, one)
    new, new_w = mr.update(xb, labels, cent, w)
    return xb, cent, w, labels, new, new_w


def test_update_bit_for_bit(step_case):
    from rvc_amd import ops
    xb, cent, w, labels, new, new_w = step_case
    k = cent.shape[0]
    assert (w == 0).any() and w.max() == 1 << 20 and len(np.unique(labels)) < k
    wd = dev(w)
    off, ids, _ = ops.kmeans_lists(dev(labels), k)
    got = ops.minibatch_update(dev(xb), off, ids, dev(cent), wd)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(new))
    np.testing.assert_array_equal(bits(wd.cpu().numpy()), bits(new_w))
    idle = np.setdiff1d(np.arange(k), labels)
    np.testing.assert_array_equal(bits(new[idle]), bits(cent[idle]))  # no member: copied


def test_update_rounds_the_product_on_its_own():
    """The case on which an fma of centre * weight with the first add gives another result."""
    from rvc_amd import ops
    cent, w, xb = mr.fma_case()
    labels = np.zeros(2, np.int32)
    new, new_w = mr.update(xb, labels, cent, w)
    wd = dev(w)
    off, ids, _ = ops.kmeans_lists(dev(labels), 2)
    got = ops.minibatch_update(dev(xb), off, ids, dev(cent), wd).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(new))
    assert got[0, 0] == np.float32(1.0) * (np.float32(1) / np.float32(5))
    np.testing.assert_array_equal(wd.cpu().numpy(), new_w)


def test_inertia_f64_and_status(step_case):
    from rvc_amd import ops
    xb, cent, w, labels, _, _ = step_case
    xd, cd, ld, wd = dev(xb), dev(cent), dev(labels), dev(w)
    s1 = ops.minibatch_inertia(xd, cd, ld, wd).cpu().numpy().copy()
    s2 = ops.minibatch_inertia(xd, cd, ld, wd).cpu().numpy().copy()
    np.testing.assert_array_equal(s1, s2)  # two runs: identical bits
    inertia, wmax, any_zero = ops.minibatch_status(torch.from_numpy(s1).to(DEV))
    want = mr.inertia(xb, cent, labels)
    print(f"inertia {inertia!r} against {want!r}: relative {abs(inertia - want) / want:.2e}")
    np.testing.assert_allclose(inertia, want, rtol=1e-12, atol=0)
    assert wmax == w.max() and any_zero
    w2 = np.where(w == 0, np.float32(3), w)
    inertia2, wmax2, any_zero2 = ops.minibatch_status(ops.minibatch_inertia(xd, cd, ld, dev(w2)))
    assert inertia2 == inertia and wmax2 == w.max() and not any_zero2
    assert ops.minibatch_status(ops.minibatch_inertia(xd, cd, ld))[1:] == (0, False)  # no weights given


@pytest.mark.parametrize("n,d,k", [(64, 16, 200), (128, 768, 300)])
def test_assign_with_more_centres_than_rows(n, d, k):
    """Centre j repeated at j + 128 (and j + 256): equal bits, so every row must take the lowest copy; the rest is
    kmeans_ref's acceptance rule.  rvc_kmeans_assign itself still refuses k > n."""
    from rvc_amd import ops
    rng = np.random.default_rng(n + k)
    x = kr.clustered(n, d, 20, seed=n)
    cent = (x[rng.integers(0, n, k)] + 0.05 * rng.standard_normal((k, d))).astype(np.float32)
    cent[:n // 2] = x[:n // 2]  # exact hits
    cent[128:256] = cent[:len(cent[128:256])]
    cent[256:] = cent[:len(cent[256:])]
    a1, d1 = ops.minibatch_assign(dev(x), dev(cent))
    a2, d2 = ops.minibatch_assign(dev(x), dev(cent))
    a1, d1 = a1.cpu().numpy(), d1.cpu().numpy()
    differ = kr.check_assign(x, cent, a1, d1)
    print(f"n={n} d={d} k={k}: {len(differ)} rows differ from the f64 argmin")
    assert a1.max() < 128
    np.testing.assert_array_equal(a1[:n // 2], np.arange(n // 2))
    np.testing.assert_array_equal(a1, a2.cpu().numpy())
    np.testing.assert_array_equal(bits(d1), bits(d2.cpu().numpy()))
    with pytest.raises(RuntimeError, match="1 <= k <= n"):
        ops.kmeans_assign(dev(x), dev(cent))


def test_scatter_rows_and_weights():
    from rvc_amd import ops
    n, d, k = 50, 24, 37
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    cent = rng.standard_normal((k, d)).astype(np.float32)
    w = rng.integers(0, 100, k).astype(np.float32)
    src = np.array([7, 7, 0, n - 1, 7], np.int64)  # repeated sources
    dst = np.array([0, k - 1, 5, 6, 20], np.int64)  # the first and the last centre
    cd, wd = dev(cent), dev(w)
    ops.minibatch_scatter(dev(xb), dev(src), dev(dst), 2.5, cd, wd)
    want_c, want_w = cent.copy(), w.copy()
    want_c[dst], want_w[dst] = xb[src], np.float32(2.5)
    np.testing.assert_array_equal(bits(cd.cpu().numpy()), bits(want_c))
    np.testing.assert_array_equal(wd.cpu().numpy(), want_w)


def test_one_step_at_the_real_widths():
    """d = 768, 10000 centres (rows plus noise), a batch of 2048: the device's labels pass the acceptance rule, and
    given those labels the update equals the restatement bit for bit."""
    from rvc_amd import ops
    n, d, k, bs = 4000, 768, 10000, 2048
    rng = np.random.default_rng(9)
    x = kr.clustered(n, d, 60, seed=17)
    cent = (x[rng.integers(0, n, k)] + 0.05 * rng.standard_normal((k, d))).astype(np.float32)
    w = rng.integers(0, 50, k).astype(np.float32)
    batch = rng.integers(0, n, bs)
    xb = x[batch]
    xd, cd, wd = ops.gather_rows(dev(x), dev(batch.astype(np.int64))), dev(cent), dev(w)
    np.testing.assert_array_equal(xd.cpu().numpy(), xb)
    labels, dist = ops.minibatch_assign(xd, cd)
    lab = labels.cpu().numpy()
    differ = kr.check_assign(xb, cent, lab, dist.cpu().numpy())
    print(f"{len(differ)} of {bs} rows differ from the f64 argmin")
    off, ids, _ = ops.kmeans_lists(labels, k)
    got = ops.minibatch_update(xd, off, ids, cd, wd)
    inertia = ops.minibatch_status(ops.minibatch_inertia(xd, cd, labels, wd))[0]
    new, new_w = mr.update(xb, lab, cent, w)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(new))
    np.testing.assert_array_equal(bits(wd.cpu().numpy()), bits(new_w))
    np.testing.assert_allclose(inertia, mr.inertia(xb, cent, lab), rtol=1e-12, atol=0)


class Forced:
    """Stands in for the RandomState of a teacher-forced step: hands out the recorded choice."""

    def __init__(self, picked):
        self.picked = picked

    def choice(self, n, replace, size):
        assert not replace and size == len(self.picked) and (self.picked < n).all()
        return self.picked


@pytest.mark.parametrize("name", ["A", "C"])
def test_trainer_teacher_forced_per_step(name):
    """State from the restatement (equal to the fixture: test_minibatch_cpu.py) before each step: the device's own
    labels pass the acceptance rule; with the fixture's labels the centres and weights after the step, reassigned
    ones included, have the restatement's bits.  The first 40 steps and every reassigning one of the first 200."""
    from rvc_amd import index_train, ops
    fx = mr.load_fixture(name)
    n, d, k, batch_size = mr.CASES[name]
    x = fx["x"]
    flags = fx["reassign"][:200]
    steps = sorted(set(range(min(40, len(flags)))) | set(np.nonzero(flags)[0].tolist()))
    _, hist = mr.fit(x, k, batch_size, int(fx["seed"]), stop_after=200, states=steps)
    xd = dev(x)
    moved = differ_rows = 0
    for i in steps:
        before, w_before, after, w_after = hist["state"][i]
        batch, want = fx["batch"][i], fx["labels"][i].astype(np.int32)
        np.testing.assert_array_equal(want, hist["labels"][i])
        xb = x[batch]
        own, dist = ops.minibatch_assign(dev(xb), dev(before))
        differ_rows += len(kr.check_assign(xb, before, own.cpu().numpy(), dist.cpu().numpy()))
        trainer = index_train.MiniBatchTrainer(xd, dev(before), w_before)
        out = trainer.step(batch, Forced(hist["picked"][i]), bool(flags[i]), labels=want)
        np.testing.assert_array_equal(out["to"], hist["to"][i], err_msg=f"step {i}")
        np.testing.assert_array_equal(bits(trainer.cent.cpu().numpy()), bits(after), err_msg=f"step {i}")
        np.testing.assert_array_equal(bits(trainer.weights.cpu().numpy()), bits(w_after), err_msg=f"step {i}")
        np.testing.assert_allclose(out["inertia"], fx["inertia"][i], rtol=1e-12, atol=0)
        assert trainer.any_zero == bool((w_after == 0).any())
        moved += len(hist["to"][i])
    print(f"case {name}: {len(steps)} steps, {int(flags.sum())} reassigning, {moved} centres reassigned, "
          f"{differ_rows} rows off the f64 argmin")
    assert moved >= (100 if name == "C" else 1)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_trainer_free_running(name):
    """Two runs with one seed give identical bits; on a fixture whose every decision clears 4 tolerances
    (free_run_exact) the centres have sklearn's bits and n_steps is sklearn's."""
    from rvc_amd import index_train
    fx = mr.load_fixture(name)
    n, d, k, batch_size = mr.CASES[name]
    xd = dev(fx["x"])
    seed = int(fx["seed"])
    cent, hist = index_train.minibatch_kmeans(xd, k, batch_size, seed, history=True)
    again = index_train.minibatch_kmeans(xd, k, batch_size, np.random.RandomState(seed))
    got = cent.cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(again.cpu().numpy()))
    steps = hist["n_steps"]
    assert got.shape == (k, d) and np.isfinite(got).all()
    assert steps == len(hist["batch"]) == len(hist["labels"]) == len(hist["inertia"]) == len(hist["counts"]) == \
        len(hist["reassigned"]) and hist["counts"][-1].shape == (k,)
    print(f"case {name}: {steps} steps on the device, {int(fx['sk_n_steps'])} in sklearn")
    if bool(fx["free_run_exact"]):
        assert steps == int(fx["sk_n_steps"])
        np.testing.assert_array_equal(bits(got), bits(fx["sk_centres"]))
        np.testing.assert_array_equal(np.asarray(hist["batch"]), fx["batch"])
        np.testing.assert_array_equal(np.asarray(hist["labels"]), fx["labels"])
        np.testing.assert_allclose(hist["inertia"], fx["inertia"], rtol=1e-12, atol=0)


def test_global_random_state_is_the_default():
    """random_state=None draws from NumPy's global RandomState, as sklearn's check_random_state(None) does."""
    from rvc_amd import index_train
    fx = mr.load_fixture("B")
    n, d, k, batch_size = mr.CASES["B"]
    np.random.seed(int(fx["seed"]))
    got = index_train.minibatch_kmeans(dev(fx["x"]), k, batch_size).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(fx["sk_centres"]))


def test_quality_against_sklearn():
    """Case Q, seeds 0..7: the mean full-data f64 inertia of the device's centres is no higher than sklearn's mean
    plus sklearn's own max - min spread over those seeds (the trajectories legitimately part at ties, so the margin
    is one spread)."""
    from rvc_amd import index_train
    q = mr.load_fixture("Q")
    n, d, k, batch_size = mr.QUALITY
    x = mr.blobs(n, d, int(q["data_seed"]))
    xd = dev(x)
    ours = [mr.full_inertia(x, index_train.minibatch_kmeans(xd, k, batch_size, int(s)).cpu().numpy())
            for s in q["seeds"]]
    sk = q["sk_inertia"]
    spread = sk.max() - sk.min()
    print(f"device mean {np.mean(ours):.2f} (min {min(ours):.2f}, max {max(ours):.2f}); sklearn mean {sk.mean():.2f}, "
          f"spread {spread:.2f}")
    assert np.mean(ours) <= sk.mean() + spread


def test_create_index_reduces_above_the_threshold(tmp_path):
    """3000 rows of v1 width with reduce_rows = 1000, reduce_to = 400: total_fea.npy is the 400 centres of
    minibatch_kmeans on the shuffled rows with the same RandomState, and they are what the IVF10 index holds."""
    from rvc_amd import index_train
    exp = tmp_path / "voice"
    os.makedirs(exp / "v1_extracted")
    x = kr.clustered(3000, 256, 60, seed=41)
    for i in range(3):
        np.save(exp / "v1_extracted" / f"clip{i}.npy", x[1000 * i: 1000 * (i + 1)])
    added = index_train.create_index(str(exp), "v1", rng=np.random.RandomState(5), device=DEV, reduce_rows=1000,
                                     reduce_to=400, batch_size=256)
    assert index_train.n_ivf_rule(400) == 10
    assert os.path.basename(added) == "added_IVF10_Flat_nprobe_1_voice_v1.index"
    assert os.path.exists(exp / "trained_IVF10_Flat_nprobe_1_voice_v1.index")
    total = np.load(exp / "total_fea.npy")
    assert total.shape == (400, 256) and total.dtype == np.float32
    rs = np.random.RandomState(5)
    order = np.arange(3000)
    rs.shuffle(order)
    want = index_train.minibatch_kmeans(dev(x[order]), 400, 256, rs).cpu().numpy()
    np.testing.assert_array_equal(bits(total), bits(want))
    idx = read_index(added)
    assert (idx.nlist, idx.ntotal) == (10, 400)
    np.testing.assert_array_equal(idx.reconstruct_n(0, 400), total)
    with pytest.raises(TypeError, match="RandomState"):
        index_train.create_index(str(exp), "v1", rng=np.random.default_rng(5), device=DEV, reduce_rows=1000,
                                 reduce_to=400, batch_size=256)
