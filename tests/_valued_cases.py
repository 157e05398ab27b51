"""The minibatch streams of the valued tests (tests/test_values_cpu.py runs the checker alone over
them and asserts that every one of its sums is exact; tests/test_gpu_values.py compares the GPU
with it on the same streams)."""
import numpy as np

from oracle import pyoracle as O
from tests import _valued_checker as V
from xflow_amd import capi

KS = (1, 4, 7, 16, 64, 80)
OPTS = ("ftrl", "sgd")
STEPS = 3


def _values(rng, lens):
    """magnitudes 2^-4 ... 4 with eight significant bits, one in ten an exact zero; one row in
    four holds negative values only, the others none: the per-factor row sums S[r,f] then never
    cancel to something tiny, whose square would sit far below the other squares of the row's T
    sum (the CPU test is the proof that every sum is exact, sum by sum)"""
    n = int(np.sum(lens))
    mant = rng.randint(128, 256, size=n).astype(np.float32) / np.float32(128.0)   # [1, 2)
    x = mant * np.exp2(rng.randint(-4, 2, size=n)).astype(np.float32)
    x *= np.repeat(np.where(rng.rand(len(lens)) < 0.25, -1.0, 1.0), lens).astype(np.float32)
    x[rng.rand(n) < 0.1] = 0.0
    return x.astype(np.float32)


def _keytab(K):
    return np.array([capi.hash_str(str(i)) for i in range(K)], dtype=np.uint64)


def ragged(seed, R=300, K=1500, longest=40):
    """ragged rows, some empty; row 1 holds one key twice with two different values"""
    rng = np.random.RandomState(seed)
    tab = _keytab(K)
    lens = rng.randint(0, longest + 1, size=R)
    lens[rng.rand(R) < 0.1] = 0
    lens[1] = 3
    rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    n = int(rowptr[-1])
    keys = tab[rng.randint(0, K, size=n)]
    vals = _values(rng, lens)
    a = int(rowptr[1])      # row 1: key A with 0.75, a small positive value, key A with -1.5
    keys[a + 2] = keys[a]
    vals[a:a + 3] = np.array([0.75, 0.09375, -1.5], np.float32)
    labels = rng.randint(0, 2, size=R).astype(np.int32)
    return rowptr, keys, vals, labels


def zipf(seed, R, per_row, K):
    """Zipf(1.1) keys: the head keys own more than XF_HEAVY_SEG occurrences"""
    rng = np.random.RandomState(seed)
    tab = _keytab(K)
    p = 1.0 / np.arange(1, K + 1) ** 1.1
    p /= p.sum()
    lens = rng.randint(per_row // 2, per_row + per_row // 2 + 1, size=R)
    rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    n = int(rowptr[-1])
    keys = tab[rng.choice(K, size=n, p=p)]
    return rowptr, keys, _values(rng, lens), rng.randint(0, 2, size=R).astype(np.int32)


def stream(case, seed=0):
    """STEPS minibatches (rowptr, keys, values, labels) whose keys overlap from step to step"""
    if case == "ragged":
        return [ragged(seed + i) for i in range(STEPS)]
    if case == "zipf_heavy":        # head keys beyond XF_HEAVY_SEG, every one in one chunk
        return [zipf(seed + i, 400, 14, 3000) for i in range(STEPS)]
    if case == "zipf_chunks":       # the head key spans several chunks of XF_TILE_NNZ
        return [zipf(seed + i, 2500, 20, 5000) for i in range(STEPS)]
    raise KeyError(case)


CASES = ("ragged", "zipf_heavy", "zipf_chunks")


def heavy_profile(mb):
    """(keys beyond XF_HEAVY_SEG occurrences, occurrences of the most frequent key)"""
    cnt = np.unique(mb[1], return_counts=True)[1]
    return int((cnt > capi.HEAVY_SEG).sum()), int(cnt.max())


def old_state(keys, opt, k, table="v", seed=11):
    """A table "many steps old" for every key a stream can hold: (keys, weights, n, z) sorted by
    key, to import into the oracle's store and the GPU table alike (the w table: k = 1,
    weights in [2^-7, 2^-5); the v table: factors in [2^-9, 2^-7)).  The weights sit in one band of
    magnitude and the state is such that a step moves them by a small fraction of themselves —
    FTRL: n = 10^4 and the z of that weight (ftrl.h:66-73 with the default alpha 0.05, beta 1,
    lambda1 5e-5, lambda2 10: w = -(z + l1) / 2030 for z < 0); SGD: the weight alone, lr 0.001 —
    so they stay there.  With |x| in [2^-4, 4) the squares fp32((v x)^2) of a row then span
    2^-26 ... 2^-10 and are multiples of 2^-49: thousands of them add exactly in fp64, where the
    squares of fresh hash-normal factors (any magnitude down to 0), or weights fresh from zero
    (lr g, g of any magnitude), do not; and the second-order term stays below 1, so that no loss
    is tiny beside the others a heavy key sums."""
    rng = np.random.RandomState(seed + (1000 if table == "w" else k))
    keys = np.sort(np.asarray(keys, np.uint64))
    lo = 2.0 ** -7 if table == "w" else 2.0 ** -9
    v = (rng.uniform(1.0, 4.0, size=(len(keys), k)) * lo).astype(np.float32)
    if opt == "sgd":
        return keys, v, None, None
    n = np.full_like(v, 1e4)
    z = (-(v.astype(np.float64) * 2030.0) - 5e-5).astype(np.float32)
    return keys, v, n, z


def stream_keys(mbs):
    return np.unique(np.concatenate([m[1] for m in mbs]))


def stores(model, opt, k, mbs=None, seed=7):
    """the oracle's stores (w zero-init, v hash-normal); with a stream given they hold the old
    state of the stream's keys"""
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    ws = O.Store(o, 1)
    vs = O.Store(o, k, O.INIT_HASHNORM, 0.0, seed) if model == "fm" else None
    if mbs is not None:
        ws.import_(*old_state(stream_keys(mbs), opt, 1, "w"))
        if vs is not None:
            vs.import_(*old_state(stream_keys(mbs), opt, k))
    return ws, vs


def run_checker(model, opt, k, mbs, audit):
    """the checker over a stream: -> per step (ukeys, wu, loss, gw), the stores, the last
    minibatch's predictions"""
    ws, vs = stores(model, opt, k, mbs)
    steps = []
    for rowptr, keys, vals, labels in mbs:
        if model == "fm":
            steps.append(V.fm_step(ws, vs, rowptr, keys, vals, labels, audit))
        else:
            steps.append(V.lr_step(ws, rowptr, keys, vals, labels, audit))
    rowptr, keys, vals, labels = mbs[-1]
    if model == "fm":
        pctr = V.fm_predict(ws, vs, rowptr, keys, vals, labels, audit)
    else:
        pctr = V.lr_predict(ws, rowptr, keys, vals, labels, audit)
    return steps, ws, vs, pctr


# the worker end to end on the golden sample files, two epochs, from fresh tables: (model,
# optimizer, k).  FM runs SGD with k = 4: there every sum of the checker is exact; under FTRL a
# first step leaves factors of any magnitude (w = -(z -+ l1) / (...) with z near l1) and the
# sums of their squares are not (k = 4: 10 of 2400 row sums and 49 of 600 sums over the factors
# depend on the order of their addends) — an input that cannot meet the condition, so not one
# this checker may judge; tests/test_gpu_values.py adds (1, "ftrl", 4) under the interval rule of
# tests/_interval.py.
E2E = ((0, "ftrl", 1), (0, "sgd", 1), (1, "sgd", 4))
E2E_EPOCHS = 2


def run_checker_files(model, opt, k, train_path, test_path, audit):
    """-> the stores after training, (labels, pctr) of the test file, its metrics"""
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    ws = O.Store(o, 1)
    vs = O.Store(o, k, O.INIT_HASHNORM, 0.0, 0) if model == 1 else None   # the worker's seed: 0
    V.train_worker(model, ws, vs, train_path, E2E_EPOCHS, audit)
    # predict's blocks: 4 MiB for LR (lr_worker.cc:80), 2 MiB for FM (fm_worker.cc:106)
    lab, p = V.predict_file(model, ws, vs, test_path, audit, (4 << 20) if model == 0 else (2 << 20))
    return ws, vs, lab, p, O.auc_logloss(lab, p)
