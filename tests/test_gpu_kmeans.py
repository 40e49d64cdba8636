"""IVF training on the device (csrc/kmeans.hip, rvc_amd/index_train.py) against the NumPy restatement
tests/kmeans_ref.py: assignment within the derived f32 tolerance of the f64 argmin, lists equal to a stable sort,
centroid updates and splits bit for bit, the trainer teacher-forced per iteration, and create_index end to end.

The assign kernel's launch plan at these sizes (128-row blocks, 128-centroid tiles, the centroid axis split over
grid.y while fewer than 256 row blocks exist): k <= 128 is one tile and no split; n = 1000 with k = 129 / 257 is
2 / 3 tiles, one per block of the split; n = 16384 with k = 300 is 3 tiles over 2 blocks, so one block crosses a
tile boundary and the other starts at tile 2."""
import os

import numpy as np
import pytest
import torch

import kmeans_ref as kr
from rvc_amd.faiss_index import IVFFlatIndex, read_index

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(d, n, k) for d in (8, 24, 256, 768) for n in (1, 127, 129, 1000) for k in (1, 2, 33, 129, 257) if n >= k]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make(d, n, k, seed=0):
    x = kr.clustered(n, d, max(1, min(k, 40)), seed=seed + d + n)
    if n >= 10:
        x[-5:] = x[:5]  # duplicated rows
    rng = np.random.default_rng(seed + k)
    cent = x[rng.choice(n, k, replace=False)].copy()  # rows themselves: exact hits, dist at the clamp
    cent[k // 2:] += (0.05 * rng.standard_normal((k - k // 2, d))).astype(np.float32)
    return x, cent


@pytest.mark.parametrize("d,n,k", SHAPES)
def test_assign_within_tolerance_of_f64(d, n, k):
    from rvc_amd import ops
    x, cent = make(d, n, k)
    xd, cd = dev(x), dev(cent)
    a1, d1 = ops.kmeans_assign(xd, cd)
    a1, d1 = a1.cpu().numpy(), d1.cpu().numpy()
    a2, d2 = ops.kmeans_assign(xd, cd)
    differ = kr.check_assign(x, cent, a1, d1)
    print(f"d={d} n={n} k={k}: {len(differ)} rows differ from the f64 argmin")
    assert (d1 >= 0).all()
    np.testing.assert_array_equal(a1, a2.cpu().numpy())  # two runs: identical bits
    np.testing.assert_array_equal(d1.view(np.uint32), d2.cpu().numpy().view(np.uint32))
    if n >= 10:  # duplicated rows: equal results
        np.testing.assert_array_equal(a1[-5:], a1[:5])
        np.testing.assert_array_equal(d1[-5:].view(np.uint32), d1[:5].view(np.uint32))


@pytest.mark.parametrize("n,d,k", [(1000, 24, 300), (16384, 8, 300), (129, 256, 129 + 0)])
def test_exact_ties_resolve_to_the_lowest_centroid(n, d, k):
    """Centroid j repeated at j + 128 (the next tile: another block of the split at n = 1000, the same block at
    n = 16384) and at j + 256 (a block of its own in both): equal bits, so every row must take the lowest copy."""
    from rvc_amd import ops
    x = kr.clustered(n, d, 30, seed=11)
    rng = np.random.default_rng(5)
    cent = x[rng.choice(n, k, replace=False)].copy()
    copies, first = [], np.arange(k)
    for j in range(0, min(44, k - 128)):
        cent[j + 128] = cent[j]
        copies.append(j + 128)
        if j + 256 < k:
            cent[j + 256] = cent[j]
            copies.append(j + 256)
    assert copies
    first[copies] = np.asarray(copies) % 128
    a, dist = ops.kmeans_assign(dev(x), dev(cent))
    a = a.cpu().numpy()
    assert not np.isin(a, copies).any()
    # the f64 matrix product does not give equal columns equal bits, so its argmin is taken to the first copy
    want = first[kr.dist64(x, cent).argmin(1)]
    assert np.isin(want, np.arange(44)).sum() > 0  # rows do land on the repeated centroids
    assert (a != want).sum() <= 0.005 * n
    kr.check_assign(x, cent, a, dist.cpu().numpy(), cap=1.0)  # the tolerance rule and dist; the cap is the line above


@pytest.mark.parametrize("n,k,mode", [(1000, 257, "random"), (5000, 257, "sparse"), (5000, 33, "random"),
                                      (4099, 257, "one"), (1, 1, "one"), (70000, 70000, "perm")])
def test_lists_equal_a_stable_sort(n, k, mode):
    """k = 257 takes two radix passes, k = 33 one, k = 70000 three; n = 5000 spans three chunks; "sparse" leaves most
    lists empty and "one" puts every row in one list."""
    from rvc_amd import ops
    rng = np.random.default_rng(n + k)
    if mode == "random":
        assign = rng.integers(0, k, n)
        assign[assign % 16 == 5] = 0  # lists 5, 21, ... stay empty
    elif mode == "sparse":
        assign = rng.choice(np.array([0, 3, 128, 255, 256]), n)
    elif mode == "perm":
        assign = rng.permutation(n)
    else:
        assign = np.full(n, k // 2)
    assign = assign.astype(np.int32)
    off, ids, counts = ops.kmeans_lists(dev(assign), k)
    woff, wids = kr.lists(assign, k)
    np.testing.assert_array_equal(off.cpu().numpy(), woff)
    np.testing.assert_array_equal(ids.cpu().numpy(), wids)
    np.testing.assert_array_equal(counts.cpu().numpy(), np.diff(woff))
    assert mode == "perm" or n == 1 or (np.diff(woff) == 0).any()


@pytest.mark.parametrize("n,d,k,mode", [(1000, 24, 257, "random"), (1003, 768, 12, "random"), (1003, 8, 5, "one"),
                                        (3000, 256, 60, "random")])
def test_update_equals_the_ordered_f32_sum_bit_for_bit(n, d, k, mode):
    from rvc_amd import ops
    x = kr.clustered(n, d, 20, seed=3)
    rng = np.random.default_rng(n)
    assign = (rng.integers(0, k, n) if mode == "random" else np.full(n, 2)).astype(np.int32)
    assign[assign == 3] = 4  # list 3 stays empty
    prev = rng.standard_normal((k, d)).astype(np.float32)
    off, ids, _ = ops.kmeans_lists(dev(assign), k)
    got = ops.kmeans_update(dev(x), off, ids, dev(prev)).cpu().numpy()
    want, counts = kr.update(x, assign, k, prev)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    empty = np.nonzero(counts == 0)[0]
    assert len(empty)
    np.testing.assert_array_equal(got[empty], prev[empty])  # empty lists keep the previous centroid


def test_gather_rows():
    from rvc_amd import ops
    x = kr.clustered(300, 24, 5, seed=2)
    ids = np.random.default_rng(0).integers(0, 300, 77)
    np.testing.assert_array_equal(ops.gather_rows(dev(x), dev(ids)).cpu().numpy(), x[ids])


def teacher_forced(x, k, hist, niter, seed=1234, cap=0.005):
    n = x.shape[0]
    assert len(hist["centroids"]) == niter + 1 and len(hist["assign"]) == niter == len(hist["objective"])
    splits = []
    for t in range(niter):
        cent, assign = hist["centroids"][t], hist["assign"][t]
        kr.check_assign(x, cent, assign, cap=cap)
        want, counts = kr.update(x, assign, k, cent)
        splits.append(kr.split(want, counts, n, seed))
        np.testing.assert_array_equal(hist["centroids"][t + 1].view(np.uint32), want.view(np.uint32))
        assert abs(hist["objective"][t] - kr.objective(x, cent, assign)) <= kr.tolerance(x, cent).sum()
    return splits


@pytest.mark.parametrize("n,d,k", [(3000, 256, 60), (500, 768, 12)])
def test_trainer_teacher_forced(n, d, k):
    from rvc_amd import index_train
    x = kr.clustered(n, d, k, seed=21)
    cent, hist = index_train.kmeans(dev(x), k, history=True)
    np.testing.assert_array_equal(hist["centroids"][0], x[kr.rand_perm(n, 1235)[:k]])  # x[perm[:k]], seed + 1
    teacher_forced(x, k, hist, 10)
    np.testing.assert_array_equal(cent.cpu().numpy(), hist["centroids"][-1])
    again = index_train.kmeans(dev(x), k)  # the same seed twice
    np.testing.assert_array_equal(again.cpu().numpy().view(np.uint32), hist["centroids"][-1].view(np.uint32))
    other, h2 = index_train.kmeans(dev(x), k, niter=2, init=x[:k], history=True)  # an explicit init overrides it
    np.testing.assert_array_equal(h2["centroids"][0], x[:k])
    teacher_forced(x, k, h2, 2)


def test_trainer_splits_empty_clusters():
    """All rows identical, k = 4: every iteration sends all rows to one centroid and splits three times.  The four
    centroids are copies of one point perturbed by 1 +- 1/1024 on alternate dimensions, at equal distances from it in
    real arithmetic, so which of them wins is inside the tolerance and the cap on rows that differ from the f64
    argmin does not apply (the rows are one row): the tolerance rule itself is still checked."""
    from rvc_amd import index_train
    row = np.random.default_rng(8).standard_normal(16).astype(np.float32)
    x = np.ascontiguousarray(np.tile(row, (64, 1)))
    cent, hist = index_train.kmeans(dev(x), 4, niter=4, history=True)
    for a in hist["assign"]:
        assert (a == a[0]).all()  # duplicated rows: equal results
    assert teacher_forced(x, 4, hist, 4, cap=1.0) == [3, 3, 3, 3]


def test_trainer_degenerate_sizes():
    from rvc_amd import index_train
    x = kr.clustered(12, 8, 3, seed=1)
    np.testing.assert_array_equal(index_train.kmeans(dev(x), 12).cpu().numpy(), x)  # n == k returns the rows
    with pytest.raises(ValueError):
        index_train.kmeans(dev(x), 13)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """create_index over four synthetic v2_extracted files (2000 rows, n_ivf = 51), run once for the module."""
    from rvc_amd import index_train
    exp = tmp_path_factory.mktemp("logs") / "voice"
    os.makedirs(exp / "v2_extracted")
    x = kr.clustered(2000, 768, 60, seed=31)
    for i in range(4):
        np.save(exp / "v2_extracted" / f"clip{i}.npy", x[500 * i: 500 * (i + 1)])
    added = index_train.create_index(str(exp), "v2", rng=np.random.default_rng(2), device=DEV)
    return exp, x, added


def test_create_index_writes_the_three_files(built):
    from rvc_amd import index_train
    from rvc_amd.retrieval import IVFFlatDevice
    exp, x, added = built
    assert index_train.n_ivf_rule(2000) == 51
    assert os.path.basename(added) == "added_IVF51_Flat_nprobe_1_voice_v2.index"
    trained = read_index(str(exp / "trained_IVF51_Flat_nprobe_1_voice_v2.index"))
    total = np.load(exp / "total_fea.npy")
    order = np.arange(2000)
    np.random.default_rng(2).shuffle(order)
    np.testing.assert_array_equal(total, x[order])  # sorted files, concatenated, shuffled with the given rng
    idx = read_index(added)
    assert (idx.nlist, idx.ntotal, idx.nprobe, trained.ntotal, trained.nlist) == (51, 2000, 1, 0, 51)
    np.testing.assert_array_equal(trained.centroids, idx.centroids)
    np.testing.assert_array_equal(idx.reconstruct_n(0, 2000), total)
    for ids in idx.ids:
        assert (np.diff(ids) > 0).all()  # ascending inside each list, as a sequential add leaves them
    # the same index without the file round trip
    cent, off, ids, codes = index_train.build_lists(dev(total), 51)
    a, b = IVFFlatDevice.from_file(added, DEV), IVFFlatDevice.from_lists(cent, off, ids, codes, dev(total))
    for name in ("centT", "list_off", "codes", "ids", "big"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.d, a.nlist, a.nprobe, a.ntotal) == (b.d, b.nlist, b.nprobe, b.ntotal)
    # against the host's f64 assignment to the same centroids: equal lists off the near ties
    assign = np.empty(2000, np.int64)
    for li, m in enumerate(idx.ids):
        assign[m] = li
    flagged = kr.check_assign(total, idx.centroids, assign)
    host = IVFFlatIndex.build(idx.centroids, total)
    for li in range(51):
        np.testing.assert_array_equal(np.setdiff1d(idx.ids[li], flagged), np.setdiff1d(host.ids[li], flagged))
    # a search of the built index finds stored rows as their own nearest neighbours
    D, I = b.search_cf(dev(total[:64].T.copy()), k=8)
    assert (I[:, 0].cpu().numpy() == np.arange(64)).sum() >= 60  # nprobe 1: all but near ties of the coarse step


def test_pipeline_runs_with_the_created_index(built, tmp_path):
    """VC.pipeline(file_index=added, index_rate=0.75) runs, and equals the run with the host-built index
    (IVFFlatIndex.build over the same centroids) when no row is flagged as a near tie."""
    from rvc_amd import synthetic
    from rvc_amd.contentvec import ContentVecAMD
    from rvc_amd.pipeline import VC, Config
    from rvc_amd.rmvpe import RMVPEAMD
    from rvc_amd.synth import SynthesizerAMD
    exp, x, added = built
    sr, version, seed = 40000, "v2", 71
    net_g = SynthesizerAMD(synthetic.make_synth_ckpt(sr, version, seed=seed), DEV)
    hub = ContentVecAMD(synthetic.make_contentvec_ckpt(seed + 1), DEV)
    vc = VC(sr, Config(DEV), rmvpe=RMVPEAMD(synthetic.rmvpe_state_dict(seed + 2), DEV))
    audio = synthetic.synthetic_audio(3.0, seed=5)
    noises = {}

    def noise(seg, kind, shape):
        if (seg, kind) not in noises:
            noises[(seg, kind)] = torch.randn(*shape, generator=torch.Generator().manual_seed(11 * seg + len(kind)))
        return noises[(seg, kind)].to(DEV)

    vc.noise_fn = noise

    def run(path):
        return np.asarray(vc.pipeline(hub, net_g, 0, audio.copy(), 0, "rmvpe", str(path), 0.75, 1, 3, 1, version, 0.33,
                                      64, False, 1, ".pth", ".pt"))

    out = run(added)
    plain = run("")
    assert out.shape == plain.shape and np.isfinite(out.astype(np.float64)).all() and not np.array_equal(out, plain)
    idx, total = read_index(added), np.load(exp / "total_fea.npy")
    assign = np.empty(2000, np.int64)
    for li, m in enumerate(idx.ids):
        assign[m] = li
    flagged = kr.check_assign(total, idx.centroids, assign)
    print(f"{len(flagged)} rows flagged as near ties")
    if len(flagged) == 0:
        host_path = tmp_path / "added_IVF51_Flat_nprobe_1_host_v2.index"
        IVFFlatIndex.build(idx.centroids, total).write(str(host_path))
        np.testing.assert_array_equal(run(host_path), out)
