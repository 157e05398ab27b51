"""Value binning (xf_bin.hip, the worker's bin=F:n,...) on a real MI355X.  Every comparison is ==
against the numpy / Python-int restatement tests/_bin_checker.py: the counts against
numpy.bincount, the LUTs, the rewritten keys and values (floats as their bits), the worker against
the same blocks driven from Python through capi.Bin and the trainer."""
import os
import shutil

import numpy as np
import pytest

from xflow_amd import capi

from . import _bin_checker as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%s: %d of %d differ; first (at, got, want): %s" % (
            what, i.size, a.size, [(j, a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


TILE, G, MAXGRID, _ = capi.Bin.shape()                     # (host code: no GPU is touched)
NNZS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * MAXGRID * TILE + 777]


def spec_of(n):
    """n listed fields, scattered ids (two of them collide in the slot table's home), bins varied"""
    return [(7 * p + (1 << 20) * (p % 3), 2 + (p * 37) % 254) for p in range(n)]


def values(rng, n):
    """counts and prices: small integers piled on a few codes, general floats, negatives, zeros"""
    v = rng.randint(0, 20, size=n).astype(np.float32)
    g = rng.rand(n)
    v = np.where(g < 0.3, np.exp(rng.randn(n) * 4).astype(np.float32), v)
    v = np.where(g < 0.05, -v, v)
    return np.where(g > 0.97, np.float32(-0.0), v).astype(np.float32)


CASES = ["n1", "nG", "nG1", "n64", "one_cell", "none_listed", "nans"]


def minibatch(case, nnz):
    rng = np.random.RandomState(nnz % 1000 + 17 * CASES.index(case))
    n = {"n1": 1, "nG": G, "nG1": G + 1, "n64": 64}.get(case, 3)
    spec = spec_of(n)
    listed = np.array([f for f, _ in spec], np.int32)
    # listed fields with unlisted ones mixed in (neighbours of listed ids among them)
    unlisted = np.concatenate([listed + 1, np.array([3, 5, 2**31 - 1], np.int32)])
    pool = unlisted if case == "none_listed" else np.concatenate([listed, unlisted])
    fgid = pool[rng.randint(0, len(pool), size=nnz)].astype(np.int32)
    vals = values(rng, nnz)
    if case == "one_cell":                     # the combine path and the counter bound
        fgid[:], vals[:] = listed[-1], 3.0
    elif case == "nans":
        bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32)
        at = rng.rand(nnz) < 0.2
        vals = np.where(at, bits[rng.randint(0, 4, size=nnz)].view(np.float32), vals)
    keys = rng.randint(0, 1 << 62, size=nnz).astype(np.uint64)
    lens = rng.multinomial(nnz, np.ones(9) / 9) if nnz else np.zeros(3, np.int64)
    rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    return spec, rowptr, keys, fgid, vals


@pytest.mark.parametrize("nnz", NNZS)
@pytest.mark.parametrize("case", CASES)
def test_count_fit_and_apply(case, nnz):
    spec, rowptr, keys, fgid, vals = minibatch(case, nnz)
    st = capi.Bin(spec)
    at = capi.Bin.launches()
    st.count(fgid, vals)
    cnt = B.counts(spec, fgid, vals)
    same(st.counts(), cnt, "counts")
    assert capi.Bin.launches() == at + (1 if nnz else 0)
    if case == "one_cell":
        assert cnt.sum() == cnt.max() == nnz
    if case == "nans" and nnz > 64:
        assert cnt[:, 4095].sum() > 0
    st.fit()
    luts = B.fit(spec, cnt)
    same(st.lut(), luts, "luts")
    with pytest.raises(capi.XFError, match=r"xf_bin_count: the stage is fitted"):
        st.count(fgid, vals)
    got = st.apply(rowptr, keys, fgid, vals)
    wk, wv, binned = B.apply(spec, luts, keys, fgid, vals)
    same(got[0], rowptr.astype(np.uint32), "rowptr")
    same(got[1], wk, "keys")
    same(got[2], fgid, "fgid")
    same(got[3], wv, "values")
    un = ~np.isin(fgid, [f for f, _ in spec])
    same(got[1][un], keys[un], "unlisted keys")
    same(got[3][un], vals[un], "unlisted values")
    assert st.stats() == (nnz, binned)
    # (a handful of nonzeros may all be unlisted by chance; from 63 on every case's draw lists some)
    assert binned == 0 if case == "none_listed" else (binned > 0 or nnz < 63)


def test_two_counts_add_and_the_order_of_calls():
    spec, rowptr, keys, fgid, vals = minibatch("nG1", 3 * TILE + 5)
    st = capi.Bin(spec)
    with pytest.raises(capi.XFError, match=r"xf_bin_apply: the stage is not fitted"):
        st.apply(rowptr, keys, fgid, vals)
    st.count(fgid, vals)
    st.count(fgid, vals, rowptr=rowptr, row_begin=2, row_end=6)    # a row slice
    a, e = int(rowptr[2]), int(rowptr[6])
    same(st.counts(), B.counts(spec, fgid, vals) + B.counts(spec, fgid[a:e], vals[a:e]), "totals")
    st.fit()
    with pytest.raises(capi.XFError, match=r"xf_bin_fit: the stage is fitted already"):
        st.fit()


def test_device_entry_and_host_entry_on_a_row_slice(tmp_path):
    spec, rowptr, keys, fgid, vals = minibatch("nG1", 5 * TILE + 3)
    labels = np.arange(len(rowptr) - 1, dtype=np.int32)
    st = capi.Bin(spec)
    st.count(fgid, vals)
    st.fit()
    got = st.apply(rowptr, keys, fgid, vals, labels=labels, row_begin=2, row_end=7)
    a, e = int(rowptr[2]), int(rowptr[7])
    wk, wv, binned = B.apply(spec, st.lut(), keys[a:e], fgid[a:e], vals[a:e])
    same(got[0], (rowptr[2:8] - rowptr[2]).astype(np.uint32), "rowptr")
    same(got[1], wk, "keys")
    same(got[2], fgid[a:e], "fgid")
    same(got[3], wv, "values")
    same(got[4], labels[2:7], "labels")
    # the device entry of another object, loaded from the first one's file, on the first one's
    # uploaded slice: the same outputs, and the inputs are not written
    path = str(tmp_path / "m.bins")
    st.save(path)
    dev = capi.Bin(spec)
    dev.load(path)
    same(dev.lut(), st.lut(), "loaded luts")
    d = st.apply_dev(rowptr, keys, fgid, vals, row_begin=2, row_end=7)
    up = capi.Cross("300*301")               # (a cross none of whose fields occur: an uploader)
    u = up.apply_dev(rowptr[2:8] - rowptr[2], keys[a:e], fgid[a:e], values=vals[a:e])
    dl = capi.RowNorm.download
    dk, dv = dev.bin_dev(u.d_keys, u.d_fgid, u.d_vals, u.NNZ)
    same(dl(dk, u.NNZ, np.uint64), dl(d.d_keys, d.NNZ, np.uint64), "device entry keys")
    same(dl(dv, u.NNZ, np.float32), dl(d.d_vals, d.NNZ, np.float32), "device entry values")
    same(dl(u.d_keys, u.NNZ, np.uint64), keys[a:e], "input keys")
    same(dl(u.d_fgid, u.NNZ, np.int32), fgid[a:e], "input fgid")
    same(dl(u.d_vals, u.NNZ, np.float32), vals[a:e], "input values")
    assert dev.stats() == (e - a, binned) and st.stats() == (2 * (e - a), 2 * binned)
    with pytest.raises(capi.XFError, match=r"was fitted for bin=.*, not for bin=5:9"):
        capi.Bin("5:9").load(path)


# ------------------------------------------------------------------ the worker end to end
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WSPEC = "2:4,17:8"
STAGES = {"bins": {}, "bins_cross_norm": dict(cross="2*17,3*4", row_norm="l2")}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("bin")
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "train-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    return d


def driven(data, extra):
    """the same blocks driven from Python: capi.Bin counts every training block and fits, then
    every block goes Bin -> (cross -> norm) -> the trainer's valued compile on the trainer's stream;
    two epochs (the second replays the kept minibatches), then the test blocks are scored"""
    st = capi.Sharded(model="lr", capacity=1 << 14)
    st.w.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))     # (the worker's init push)
    bn = capi.Bin(WSPEC)
    x = capi.Cross(extra["cross"]) if extra else None
    rn = capi.RowNorm() if extra else None
    train = list(capi.read_blocks(str(data / "train-00000"), 2 << 20, values=True))
    for rp, keys, fg, labels, vals in train:
        bn.count(fg, vals)
    bn.fit()

    def compiled(rp, keys, fg, labels, vals):
        d = bn.apply_dev(rp, keys, fg, vals, labels=labels, stream=st.stream())
        dk, dr, nnz, dv = d.d_keys, d.d_rowptr, d.NNZ, d.d_vals
        if extra:
            dk, dr, nnz, _, dv = x.cross_dev(dk, dr, d.R, nnz, d.d_fgid, d_vals=dv, want_fgid=False,
                                             stream=st.stream())
            dv, _ = rn.norm_dev(dv, dr, d.R, nnz, stream=st.stream(), want_sumsq=False)
        return st.compile_valued_dev(dk, dv, dr, d.d_labels, d.R, nnz)
    mbs = [compiled(*blk) for blk in train]
    for _ in range(2):
        for b in mbs:
            st.step(b)
            st.check()
    labs, ps = [], []
    for blk in capi.read_blocks(str(data / "test-00000"), 4 << 20, values=True):
        ps.append(st.predict(compiled(*blk)))
        labs.append(blk[3])
    return st, np.concatenate(labs), np.concatenate(ps), bn


def run_worker(data, tag, **params):
    pred = str(data / ("pred_%s.txt" % tag))
    p = dict(model=0, epochs=2, capacity=1 << 14, feature_values="on", bin=WSPEC, pred_path=pred)
    p.update(params)
    x = capi.XFlow(str(data / "train"), str(data / "test"), **p)
    x.train()
    return x, pred


@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
@pytest.mark.parametrize("stages", sorted(STAGES))
def test_worker_against_the_same_blocks_driven_from_python(data, stages, ingest):
    st, lab, p, bn = driven(data, STAGES[stages])
    x, pred = run_worker(data, stages + ingest, ingest=ingest, **STAGES[stages])
    wh, _ = x.tables()
    for a, e in zip(capi.Table.from_handle(wh, 1, capi.OPT_FTRL).export(), st.w.export()):
        same(a, e, "table")
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b)
                                                  for a, b in zip(p, lab)]
    seen, binned = bn.stats()
    assert binned > 0 and (x.metric("bin_nonzeros"), x.metric("bin_binned")) == (seen, binned)
    assert x.metric("bin_fit_rows") == x.metric("rows_trained") / 2 > 100


def test_save_then_load_predicts_the_same_bytes(data, tmp_path):
    model = str(tmp_path / "model")
    x, pred = run_worker(data, "save", ingest="host", model_out=model)
    assert os.path.exists(model + ".bins")
    y, pred_y = run_worker(data, "load", ingest="host", model_in=model, epochs=0)
    assert open(pred_y, "rb").read() == open(pred, "rb").read() and os.path.getsize(pred) > 500
    assert y.metric("bin_fit_rows") == 0                           # (nothing is fitted after a load)
    with pytest.raises(capi.XFError, match=r"was fitted for bin=2:4,17:8, not for bin=2:5,17:8"):
        run_worker(data, "other", ingest="host", model_in=model, epochs=0, bin="2:5,17:8")


@pytest.mark.parametrize("want", [1, 5000])
def test_bin_fit_rows_stops_after_whole_blocks(data, tmp_path, want):
    """fifty copies of the training file are three 1 MiB blocks: the fit reads whole blocks until
    it has `want` rows, and the saved LUTs are those of exactly these blocks"""
    text = open(str(data / "train-00000"), "rb").read()
    os.makedirs(str(tmp_path / "d"))
    with open(str(tmp_path / "d" / "train-00000"), "wb") as f:
        f.write(text * 50)
    shutil.copy(str(data / "test-00000"), str(tmp_path / "d" / "test-00000"))
    blocks = list(capi.read_blocks(str(tmp_path / "d" / "train-00000"), 1 << 20, values=True))
    rows = np.cumsum([len(b[3]) for b in blocks])
    k = int(np.searchsorted(rows, want)) + 1                      # the fewest blocks with >= want rows
    assert len(blocks) == 3 and k == (1 if want == 1 else 2)
    model = str(tmp_path / "model")
    x = capi.XFlow(str(tmp_path / "d" / "train"), str(tmp_path / "d" / "test"), model=0, epochs=1,
                   capacity=1 << 14, feature_values="on", bin=WSPEC, bin_fit_rows=want,
                   block_size_mb=1, model_out=model, pred_path=str(tmp_path / "pred.txt"))
    x.train()
    assert x.metric("bin_fit_rows") == rows[k - 1] >= want and rows[k - 1] < rows[-1]
    ref, got = capi.Bin(WSPEC), capi.Bin(WSPEC)
    for rp, keys, fg, labels, vals in blocks[:k]:
        ref.count(fg, vals)
    ref.fit()
    got.load(model + ".bins")
    same(got.lut(), ref.lut(), "luts of the first blocks")


REFUSALS = [
    (dict(feature_values="off"), r"bin=2:4,17:8 needs feature_values=on"),
    (dict(core_num=2), r"bin=2:4,17:8 needs core_num=1, not core_num=2"),
    (dict(key_build="host"), r"bin=2:4,17:8 together with key_build=host"),
    (dict(parity="reference_order"), r"bin=2:4,17:8 together with parity=reference_order"),
    (dict(ingest="gpu"), r"bin=2:4,17:8 together with ingest=gpu"),
    (dict(world=2), r"bin=2:4,17:8 runs on one worker only \(world 2\)"),
    (dict(bin="2:4,2:8"), r"xf_bin_parse: the field of '2:8' is listed twice"),
]


@pytest.mark.parametrize("params,msg", REFUSALS, ids=["feature_values", "core_num", "key_build",
                                                      "parity", "ingest", "world", "spec"])
def test_refusals_by_name(data, params, msg):
    p = dict(feature_values="on", bin=WSPEC)
    p.update(params)
    with pytest.raises(capi.XFError, match=msg):
        capi.XFlow(str(data / "train"), str(data / "test"), **p).train()
