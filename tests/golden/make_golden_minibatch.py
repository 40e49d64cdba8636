"""Records tests/golden/minibatch_*.npz from sklearn itself (needs scikit-learn; the tests read the files only).

    python tests/golden/make_golden_minibatch.py

Cases A, B, C (tests/minibatch_ref.py: CASES): the rows, the seed, sklearn's ``cluster_centers_`` and ``n_steps_`` and
the restatement's per-step history.  For each case the first seed in 0..63 is taken for which (i) the restatement
equals sklearn bit for bit with equal ``n_steps_`` and (ii) every comparison of the stopping rule is decided by more
than 1e-6 relative.  A case whose every step also leaves at least 4 x ``kmeans_ref.tolerance`` between a row's best
and next different distance is marked ``free_run_exact``: the device's f32 assignment cannot part from it.  A case
without that property is teacher-forced only, and the maker says so.  Case Q: sklearn's eight full-data f64 inertias
at seeds 0..7 only.

Rows of more than 1 MiB are stored in parts (minibatch_<case>_x1.npz, ...), which ``minibatch_ref.load_fixture`` joins.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import MiniBatchKMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import minibatch_ref as mr  # noqa: E402

PART_ROWS_BYTES = 640 * 1024


def sk_fit(x, k, batch_size, seed):
    return MiniBatchKMeans(n_clusters=k, batch_size=batch_size, compute_labels=False, init="random",
                           random_state=seed).fit(x)


def flat(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return off, (np.concatenate(parts) if len(parts) else np.zeros(0, np.int64)).astype(np.int32)


def record(name):
    n, d, k, batch_size = mr.CASES[name]
    x = mr.blobs(n, d, mr.DATA_SEED[name])
    chosen = None
    for seed in range(64):
        sk = sk_fit(x, k, batch_size, seed)
        cent, hist = mr.fit(x, k, batch_size, seed)
        same = np.array_equal(cent.view(np.uint32), sk.cluster_centers_.view(np.uint32)) and \
            hist["n_steps"] == sk.n_steps_
        exact = min(hist["gap_tol"]) >= 4.0
        print(f"case {name} seed {seed}: equal to sklearn {same}, n_steps {hist['n_steps']} / {sk.n_steps_}, "
              f"ewa gap {hist['min_ewa_gap']:.2e}, decision gap {min(hist['gap']):.2e} = "
              f"{min(hist['gap_tol']):.2f} tolerances, {sum(len(t) for t in hist['to'])} reassigned")
        if same and hist["min_ewa_gap"] > 1e-6:
            chosen = (seed, sk, hist, exact)
            break
    if chosen is None:
        print(f"case {name}: no seed in 0..63 qualifies; no fixture")
        return
    seed, sk, hist, exact = chosen
    if not exact:
        print(f"case {name}: no qualifying seed keeps 4 tolerances at every step; teacher-forced only")
    to_off, to = flat(hist["to"])
    _, picked = flat(hist["picked"])
    rows = max(1, PART_ROWS_BYTES // (4 * d))
    parts = [x[i:i + rows] for i in range(0, n, rows)]
    np.savez_compressed(
        os.path.join(HERE, f"minibatch_{name}.npz"), x=parts[0], seed=seed, n_clusters=k, batch_size=batch_size,
        sk_centres=sk.cluster_centers_, sk_n_steps=sk.n_steps_, init=hist["init"],
        batch=np.asarray(hist["batch"], np.int32), labels=np.asarray(hist["labels"], np.int16),
        inertia=np.asarray(hist["inertia"], np.float64), reassign=np.asarray(hist["reassign"], bool), to_off=to_off,
        to=to, picked=picked, gap=np.asarray(hist["gap"]), gap_tol=np.asarray(hist["gap_tol"]),
        min_ewa_gap=hist["min_ewa_gap"], free_run_exact=exact, sklearn_version=sklearn.__version__,
        numpy_version=np.__version__)
    for p, part in enumerate(parts[1:], 1):
        np.savez_compressed(os.path.join(HERE, f"minibatch_{name}_x{p}.npz"), x=part)
    print(f"case {name}: seed {seed}, {hist['n_steps']} steps, free_run_exact {exact}, {len(parts)} file(s)")


def record_quality():
    n, d, k, batch_size = mr.QUALITY
    x = mr.blobs(n, d, mr.DATA_SEED["Q"])
    inertia = [mr.full_inertia(x, sk_fit(x, k, batch_size, s).cluster_centers_) for s in mr.QUALITY_SEEDS]
    print("case Q: sklearn full-data inertias", inertia)
    np.savez_compressed(os.path.join(HERE, "minibatch_Q.npz"), sk_inertia=np.asarray(inertia, np.float64),
                        seeds=np.asarray(mr.QUALITY_SEEDS), data_seed=mr.DATA_SEED["Q"],
                        sklearn_version=sklearn.__version__, numpy_version=np.__version__)


if __name__ == "__main__":
    for case in mr.CASES:
        record(case)
    record_quality()
