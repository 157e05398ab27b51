"""Row normalisation (xf_rownorm.hip, the worker's row_norm=l2) on a real MI355X.  The reference of
the stage is the host definition xf_rownorm_row, which tests/test_rownorm_cpu.py pins to the numpy
restatement tests/_rownorm_checker.py and that to a plain loop.  Every comparison is exact: integer
arrays, float arrays as their bits, the rows' sums of squares with == (a NaN matching a NaN).

* the stage: values and sums on minibatches chosen where the kernel can go wrong, one after the
  other on ONE object, sizes growing and then shrinking; the statistics; the launch counter;
* the host entry on a row slice against the device entry; descending offsets;
* valued LR (cell kernels and the generic path), canonical and field-aware FM, FTRL and SGD,
  stepped on the stage's device arrays, against each mode's exact checker fed the host-normalised
  values — on minibatches by the power-of-two recipe, whose normalised values are exact;
* the worker end to end: row_norm=l2 on a file with values 1 and 2 against the plain worker on
  the same rows with their exact normalised decimals."""
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _cross_checker as X
from . import _ffm_checker as F
from . import _rownorm_checker as Rn
from . import _valued_cases as Cs
from . import _valued_checker as V

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


# ------------------------------------------------------------------ the stage's minibatches
def _keys(rng, n):
    return rng.randint(0, 1 << 62, size=n).astype(np.uint64)


def _mb(rng, lens, rows=None):
    """(rowptr, keys, values): general-position values; rows: {row index: its values}"""
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(rowptr[-1])
    vals = Rn.general_values(rng, n)
    for r, x in (rows or {}).items():
        assert len(x) == lens[r]
        vals[int(rowptr[r]):int(rowptr[r + 1])] = x
    return rowptr, _keys(rng, n), vals


def sequence():
    """[(name, rowptr, keys, values)] in the order they are applied to one object"""
    G, W = capi.RowNorm.shape()
    rng = np.random.RandomState(43)
    out = []
    add = lambda name, mb: out.append((name,) + mb)  # noqa: E731
    add("no_rows", _mb(rng, []))
    add("all_rows_empty", _mb(rng, np.zeros(5, np.int64)))
    add("one_row", _mb(rng, [7]))
    add("one_empty_row", _mb(rng, [0]))
    add("group_edges", _mb(rng, [G - 1, G, G + 1, 2 * G, 3 * G - 1, 3 * G + 1, 4 * G, 4 * G + 1]))
    add("lengths", _mb(rng, [G - 1, G, G + 1, 63, 64, 65, 4095, 4096, 4097]))
    for where, at in (("first", 0), ("middle", 150), ("last", 300)):
        lens = rng.randint(0, 9, size=301)
        lens[at] = 5000
        add("long_row_" + where, _mb(rng, lens))
    for R in (W - 1, W, W + 1, 2 * W + 1):
        add("rows%d" % R, _mb(rng, rng.randint(0, 40, size=R)))
    lens = rng.randint(1, 40, size=700)
    lens[:3] = 0
    lens[-2:] = 0
    lens[300:340] = 0
    lens[rng.rand(700) < 0.05] = 0
    add("empty_rows", _mb(rng, lens))
    special = Rn.special_rows()
    lens = rng.randint(0, 30, size=3 * len(special) + 2)
    rows = {}
    for i, (_, x) in enumerate(special):
        lens[3 * i + 1] = len(x)
        rows[3 * i + 1] = x
    add("special_rows", _mb(rng, lens, rows))
    # a long row that holds a NaN / is all zero: the unchanged branch of the long path
    longnan = Rn.general_values(rng, 200)
    longnan[137] = np.nan
    add("long_special", _mb(rng, [3, 200, 100, 70, 5], {1: longnan, 2: np.zeros(100, np.float32),
                                                       3: np.full(70, 1e-45, np.float32)}))
    add("click_rows", _mb(rng, rng.randint(17, 40, size=4 * W * 40 + 3)))
    add("one_row_again", out[2][1:])
    add("no_rows_again", out[0][1:])
    return out


def expected(rowptr, vals):
    """(values, sums, rows scaled) by the host definition, row by row"""
    rp = rowptr.astype(np.int64)
    y, ss, scaled = np.empty(len(vals), np.float32), np.zeros(len(rp) - 1, np.float64), 0
    for r in range(len(rp) - 1):
        y[rp[r]:rp[r + 1]], ss[r] = capi.rownorm_row(vals[rp[r]:rp[r + 1]])
        scaled += int(Rn.scales(ss[r]))                 # the restatement's branch
    return y, ss, scaled


def test_the_stage_on_one_object():
    st = capi.RowNorm()
    rows = scaled = 0
    names = []
    for name, rowptr, keys, vals in sequence():
        at = capi.RowNorm.launches()
        got = st.apply(rowptr, keys, vals)
        y, ss, sc = expected(rowptr, vals)
        same(got[0], rowptr.astype(np.uint32), name + " rowptr")
        same(got[1], keys, name + " keys")
        same(got[2], y, name + " values")
        assert Rn.same_sums(got[3], ss), (name, got[3][:8], ss[:8])
        R = len(rowptr) - 1
        assert capi.RowNorm.launches() == at + (1 if R else 0), name   # R = 0 launches nothing
        rows, scaled = rows + R, scaled + sc
        assert st.stats() == (rows, scaled), name
        names.append(name)
        if name in ("special_rows", "long_special"):
            assert 0 < sc < R
    assert scaled < rows and len(names) == len(set(names)) == 19


def _upload(rowptr, keys, vals):
    """device copies of a minibatch's arrays (a cross none of whose fields occur is the identity)"""
    up = capi.Cross("300*301")
    d = up.apply_dev(rowptr, keys, np.zeros(len(keys), np.int32), values=vals, want_fgid=False)
    return up, d


def test_device_entry_and_host_entry_on_a_row_slice():
    """rows [100, 300) of a block through the host entry; the same rows through the device entry"""
    _, rowptr, keys, vals = [m for m in sequence() if m[0] == "empty_rows"][0]
    R = len(rowptr) - 1
    labels = np.arange(R, dtype=np.int32)
    fg = (keys % np.uint64(7)).astype(np.int32)
    st = capi.RowNorm()
    got = st.apply(rowptr, keys, vals, labels=labels, fgid=fg, row_begin=100, row_end=300)
    a, e = int(rowptr[100]), int(rowptr[300])
    rp = (rowptr[100:301] - rowptr[100])
    same(got[0], rp.astype(np.uint32), "rowptr")
    same(got[1], keys[a:e], "keys")
    same(got[4], labels[100:300], "labels")
    same(got[5], fg[a:e], "fgid")
    y, ss, sc = expected(rp, vals[a:e])
    same(got[2], y, "values")
    assert Rn.same_sums(got[3], ss) and st.stats() == (200, sc)
    # the device entry, on another object
    up, d = _upload(rp, keys[a:e], vals[a:e])
    dev = capi.RowNorm()
    dv, ds = dev.norm_dev(d.d_vals, d.d_rowptr, d.R, d.NNZ)
    same(capi.RowNorm.download(dv, d.NNZ, np.float32), got[2], "device entry values")
    assert Rn.same_sums(capi.RowNorm.download(ds, d.R, np.float64), got[3])
    same(capi.RowNorm.download(d.d_vals, d.NNZ, np.float32), vals[a:e], "the input is not written")
    # without the sums: the same values
    dv2, none = dev.norm_dev(d.d_vals, d.d_rowptr, d.R, d.NNZ, want_sumsq=False)
    assert none is None
    same(capi.RowNorm.download(dv2, d.NNZ, np.float32), got[2], "values without sums")
    assert dev.stats() == (400, 2 * sc)
    # R = 0 through the device entry: nothing is launched
    at = capi.RowNorm.launches()
    dev.norm_dev(None, None, 0, 0)
    assert capi.RowNorm.launches() == at and dev.stats() == (400, 2 * sc)


def test_the_host_entry_refuses_descending_offsets_and_lives_on():
    st = capi.RowNorm()
    keys, vals = np.arange(5, dtype=np.uint64), np.ones(5, np.float32)
    with pytest.raises(capi.XFError, match=r"xf_rownorm_apply: row offsets descend at row 2"):
        st.apply(np.array([0, 3, 2, 5], np.uint64), keys, vals)
    with pytest.raises(capi.XFError, match=r"xf_rownorm_apply: row offsets descend"):
        st.apply(np.array([4, 5, 2], np.uint64), keys, vals)
    with pytest.raises(capi.XFError, match=r"xf_rownorm_apply: .*vals is NULL"):
        st.apply_dev(np.array([0, 5], np.uint64), keys, None)
    assert st.stats() == (0, 0)
    got = st.apply(np.array([0, 4, 5], np.uint64), keys, vals)
    same(got[2], np.array([0.5, 0.5, 0.5, 0.5, 1.0], np.float32))
    assert got[3].tolist() == [4.0, 1.0] and st.stats() == (2, 2)


# ------------------------------------------------------------------ trainers fed from the stage
FIELDS = 5


def recipe_stream(seed=0, R=160, K=900):
    """three minibatches (rowptr, keys, fgid, values, labels) by the power-of-two recipe: a row
    holds a values +-1 and b values +-2 with a + 4 b in {4, 16, 64} (s is 4, 16 or 64 and the
    normalised values are exactly +-2^-k), one row in twelve is empty, row 1 holds a key twice"""
    tab = Cs._keytab(K)
    out = []
    for i in range(3):
        rng = np.random.RandomState(600 + seed + i)
        rows = [np.zeros(0, np.float32) if rng.rand() < 1 / 12 else
                Rn.recipe_row(rng, (4, 16, 16, 64)[rng.randint(0, 4)]) for _ in range(R)]
        rows[1] = Rn.recipe_row(rng, 16, 2)
        lens = np.array([len(x) for x in rows])
        rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
        keys = tab[rng.randint(0, K, size=int(rowptr[-1]))]
        keys[int(rowptr[1]) + 2] = keys[int(rowptr[1])]
        fg = F._fields_of(np.random.RandomState(7 + seed + i), keys, FIELDS)
        out.append((rowptr, keys, fg, np.concatenate(rows).astype(np.float32),
                    rng.randint(0, 2, size=R).astype(np.int32)))
    return out


def host_normalised(mbs):
    out = []
    for rowptr, keys, fg, vals, labels in mbs:
        y, ss, _ = Rn.apply(rowptr, vals)
        assert set(np.unique(ss).tolist()) <= {0.0, 4.0, 16.0, 64.0}
        assert set(np.unique(np.abs(y)).tolist()) <= {0.125, 0.25, 0.5, 1.0}
        out.append((rowptr, keys, fg, y, labels))
    return out


def export_same(table, store, opt, what):
    for a, e in zip(table.export()[:4 if opt == "ftrl" else 2], store.export()):
        same(a, e, what)


def _valued(model, opt, k):
    mbs = recipe_stream()
    cm = [(rp, ks, y, labels) for rp, ks, _, y, labels in host_normalised(mbs)]
    audit = []
    _, sw, sv, pctr = Cs.run_checker(model, opt, k, cm, audit)
    V.assert_exact(audit)
    st = capi.Sharded(model=model, optimizer=opt, k=k, capacity=1 << 18, seed=7,
                      fm_mode="canonical" if model == "fm" else "reference")
    st.w.import_(*Cs.old_state(Cs.stream_keys(cm), opt, 1, "w"))
    if model == "fm":
        st.v.import_(*Cs.old_state(Cs.stream_keys(cm), opt, k))
    n = capi.RowNorm()
    b = None
    for rowptr, keys, _, vals, labels in mbs:
        d, _ = n.apply_dev(rowptr, keys, vals, labels=labels, stream=st.stream())
        b = st.compile_valued_dev(d.d_keys, d.d_vals, d.d_rowptr, d.d_labels, d.R, d.NNZ)
        st.step(b)
        st.check()
    same(st.predict(b), pctr, "pctr")
    export_same(st.w, sw, opt, "w")
    if model == "fm":
        export_same(st.v, sv, opt, "v")
    assert n.stats()[0] == 3 * 160 and 0 < n.stats()[1] < n.stats()[0]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_valued_lr_on_the_cell_kernels_from_the_stage(opt):
    _valued("lr", opt, 1)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_valued_lr_on_the_generic_path_from_the_stage(opt):
    try:
        capi.tune("valued_lr", 1)
        _valued("lr", opt, 1)
    finally:
        capi.tune("valued_lr", 0)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_valued_canonical_fm_from_the_stage(opt):
    _valued("fm", opt, 4)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_valued_field_aware_fm_from_the_stage(opt):
    k, Fd = 4, FIELDS
    mbs = recipe_stream()
    cm = host_normalised(mbs)
    audit = []
    _, sw, sv, pctr = F.run_checker(opt, Fd, k, cm, audit, valued=True)
    F.assert_exact(audit)
    st = capi.Sharded(model="fm", optimizer=opt, k=k, capacity=1 << 18, seed=7,
                      fm_mode="field_aware", fields=Fd)
    st.w.import_(*Cs.old_state(F.stream_keys(cm), opt, 1, "w"))
    st.v.import_(*Cs.old_state(F.stream_keys(cm), opt, Fd * k))
    n = capi.RowNorm()
    b = None
    for rowptr, keys, fg, vals, labels in mbs:
        d, _ = n.apply_dev(rowptr, keys, vals, labels=labels, fgid=fg, stream=st.stream())
        h = capi.vp()
        capi.check(capi.lib().xf_sharded_compile_fielded_dev(
            st.h, capi.C.byref(h), d.d_keys, d.d_fgid, d.d_vals, d.d_rowptr, d.d_labels, d.R,
            d.NNZ, 1))
        b = capi.ShardedBatch(h, st)
        st.step(b)
        st.check()
    same(st.predict(b), pctr, "pctr")
    export_same(st.w, sw, opt, "w")
    export_same(st.v, sv, opt, "v")


# ------------------------------------------------------------------ the worker end to end
NFIELD = 6                  # fgids 0 .. 5
ADMIT = dict(admit_count=2, admit_log2_slots=16)


def _rows(seed, R, style):
    """[(label, [(fgid, fid, value)])]: rows by the recipe.  style 'plain': a values +-1, b values
    +-2; 'cross': values +-1 only, one member each of fields 1 and 2, and one nonzero fewer than
    the target (the cross 1*2 adds it: +-1); 'admit': plain, plus one or two nonzeros of value 3
    under keys that occur once in all the files (admission with admit_count=2 drops them)"""
    rng = np.random.RandomState(seed)
    out = []
    for r in range(R):
        label = int(rng.randint(0, 2))
        if style != "cross" and r % 29 == 5:                     # a row of zeros: left as it is
            out.append((label, [(int(rng.randint(0, NFIELD)), int(rng.randint(0, 120)), 0.0)
                                for _ in range(3)]))
            continue
        target = (4, 16, 16, 64)[rng.randint(0, 4)]
        if style == "cross":
            x = Rn.recipe_row(rng, target, 0)[:-1]
            fg = rng.choice([0, 3, 4, 5], size=len(x))
            fg[rng.permutation(len(x))[:2]] = (1, 2)
        else:
            x = Rn.recipe_row(rng, target)
            fg = rng.randint(0, NFIELD, size=len(x))
        # (few keys: every one occurs many times in the training file)
        toks = [(int(f), int(rng.randint(0, 120)), float(v)) for f, v in zip(fg, x)]
        if style == "admit":
            for j in range(1 + r % 2):
                toks.insert(int(rng.randint(0, len(toks) + 1)),
                            (int(rng.randint(0, NFIELD)), 1000000 + 1000 * seed + 2 * r + j, 3.0))
        out.append((label, toks))
    return out


def _write(path, rows, normalise):
    """the text of rows; normalise: the values of a row's nonzeros under frequent keys (fid below
    10^6) as their exact normalised decimals"""
    with open(path, "w") as f:
        for label, toks in rows:
            x = np.array([v for _, fid, v in toks if fid < 1000000], np.float32)
            y = iter(Rn.row(x)[0].tolist()) if normalise else iter(x.tolist())
            f.write("%d\t%s\n" % (label, " ".join(
                "%d:%d:%s" % (fg, fid, "%g" % (next(y) if fid < 1000000 else v))
                for fg, fid, v in toks)))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("rownorm")
    for style in ("plain", "cross", "admit"):
        for part, seed, R in (("train", 1, 240), ("test", 2, 90)):
            rows = _rows(seed + (10 if style == "admit" else 0), R, style)
            os.makedirs(str(d / style), exist_ok=True)
            _write(str(d / style / ("raw_%s-00000" % part)), rows, False)
            _write(str(d / style / ("unit_%s-00000" % part)), rows, True)
    return d


def test_the_files_hold_what_the_cases_need(data):
    raw = open(str(data / "plain" / "raw_train-00000")).read()
    unit = open(str(data / "plain" / "unit_train-00000")).read()
    def vals(s):
        return {t.split(":")[2] for ln in s.splitlines() for t in ln.split("\t")[1].split()}
    assert vals(raw) == {"1", "-1", "2", "-2", "0"}
    assert vals(unit) == {"1", "-1", "0.5", "-0.5", "0.25", "-0.25", "0.125", "-0.125", "0"}
    # admission: the restatement's filter admits exactly the frequent keys' nonzeros
    from . import _admit_checker as A
    flt = A.Filter(16, 2, 3, 0)
    (rp, keys, fg, labels, v), = capi.read_blocks(str(data / "admit" / "raw_train-00000"), 2 << 20,
                                                  values=True)
    assert (v == 3).sum() > 240
    kept = flt.filter(rp, keys, fg, v, update=True)
    assert len(kept[1]) == (v != 3).sum() and not (kept[3] == 3).any()
    (rp, keys, fg, labels, v), = capi.read_blocks(str(data / "admit" / "raw_test-00000"), 4 << 20,
                                                  values=True)
    kept = flt.filter(rp, keys, fg, v, update=False)
    assert len(kept[1]) == (v != 3).sum() and not (kept[3] == 3).any()


def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


MODES = {
    "lr": dict(model=0, optimizer="ftrl"),
    "fm": dict(model=1, optimizer="sgd", k=4, fm_mode="canonical"),
    "ffm": dict(model=1, optimizer="sgd", k=4, fm_mode="field_aware", fields=NFIELD),
}


def run(data, style, which, tag, capfd, **params):
    """one worker run -> (handle, prediction file's bytes, printed lines, tables)"""
    pred = str(data / style / ("pred_%s.txt" % tag))
    p = dict(epochs=2, capacity=1 << 14, feature_values="on", pred_path=pred)
    p.update(params)
    capfd.readouterr()
    x = capi.XFlow(str(data / style / (which + "_train")), str(data / style / (which + "_test")),
                   **p)
    x.train()
    lines = [ln for ln in capfd.readouterr().out.split("\n") if not ln.startswith("examples/sec")]
    wh, vh = x.tables()
    opt = _go(p.get("optimizer", "ftrl"))
    tables = [capi.Table.from_handle(wh, 1, opt).export()]
    if p.get("model", 0) == 1:
        width = p["k"] * (p["fields"] if p.get("fm_mode") == "field_aware" else 1)
        tables.append(capi.Table.from_handle(vh, width, opt).export())
    return x, open(pred, "rb").read(), lines, tables


METRICS = ("logloss_ref", "logloss_nat", "auc", "tp", "fp", "keys", "rows_trained")


def pair(data, style, tag, capfd, **params):
    """row_norm=l2 on the raw file against the plain worker on the normalised one"""
    x, pred_x, out_x, tab_x = run(data, style, "raw", tag + "_l2", capfd, row_norm="l2", **params)
    y, pred_y, out_y, tab_y = run(data, style, "unit", tag + "_unit", capfd, **params)
    assert pred_x == pred_y and len(pred_x) > 500
    norm_lines = [ln for ln in out_x if ln.startswith("row_norm:")]
    assert len(norm_lines) == 1 and not [ln for ln in out_y if "row_norm" in ln]
    assert [ln for ln in out_x if not ln.startswith("row_norm:")] == out_y
    for tx, ty in zip(tab_x, tab_y):
        assert len(tx[0]) > 100
        for a, e in zip(tx, ty):
            same(a, e, "table")
    for n in METRICS:
        a, e = x.metric(n), y.metric(n)
        assert a == e or (np.isnan(a) and np.isnan(e)), n
    assert (y.metric("norm_rows"), y.metric("norm_rows_scaled")) == (0, 0)
    return x, norm_lines[0]


def restated_rows(data, style, rows_through):
    """(rows, scaled rows) the stage sees: every row of `rows_through` passes of the training
    file and one of the test file, a row scaled iff the restatement scales it"""
    tot = sc = 0
    for part, times in (("train", rows_through), ("test", 1)):
        (rp, keys, fg, labels, v), = capi.read_blocks(
            str(data / style / ("raw_%s-00000" % part)), 4 << 20, values=True)
        if style == "admit":
            v = np.where(v == 3, np.float32(0), v)       # (dropped ahead of the stage)
        s = Rn.apply(rp, v)[2]
        tot, sc = tot + times * len(labels), sc + times * s
    return tot, sc


@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
@pytest.mark.parametrize("mode", ["lr", "fm", "ffm"])
def test_worker_end_to_end(data, capfd, mode, ingest):
    x, line = pair(data, "plain", "%s_%s" % (mode, ingest), capfd, ingest=ingest, **MODES[mode])
    # (two epochs: the second replays the compiled minibatches — one pass through the stage)
    rows, scaled = restated_rows(data, "plain", 1)
    assert (x.metric("norm_rows"), x.metric("norm_rows_scaled")) == (rows, scaled)
    assert scaled < rows
    (rp, _, _, labels, v), = capi.read_blocks(str(data / "plain" / "raw_train-00000"), 4 << 20,
                                              values=True)
    tr_scaled = Rn.apply(rp, v)[2]
    assert line == "row_norm: rows = %d scaled = %d left = %d" % (
        len(labels), tr_scaled, len(labels) - tr_scaled)


def test_worker_with_admission(data, capfd):
    x, _ = pair(data, "admit", "admit", capfd, ingest="gpu_fields", **ADMIT)
    assert (x.metric("norm_rows"), x.metric("norm_rows_scaled")) == restated_rows(data, "admit", 1)
    assert x.metric("admit_kept") < x.metric("admit_seen")


def test_worker_with_negative_subsampling(data, capfd):
    x, _ = pair(data, "plain", "neg", capfd, ingest="host", neg_keep=0.25)
    assert 0 < x.metric("rows_kept") < 240
    assert x.metric("norm_rows") == x.metric("rows_kept") + 90


def test_worker_with_holdout(data, capfd):
    x, _ = pair(data, "plain", "holdout", capfd, ingest="gpu_fields", holdout=0.25)
    assert x.metric("holdout_rows") > 20
    assert x.metric("norm_rows") == 240 + 90             # the train part and the held part


def test_worker_without_the_minibatch_cache(data, capfd):
    x, _ = pair(data, "plain", "nocache", capfd, ingest="host", cache_batches=0)
    assert (x.metric("norm_rows"), x.metric("norm_rows_scaled")) == restated_rows(data, "plain", 2)


def test_worker_with_a_cross(data, capfd):
    """The cross multiplies values, so no file of pre-normalised values gives the plain worker the
    same nonzeros: y_a y_b = rs^2 x_a x_b where the stage gives rs x_a x_b.  The reference here is
    the restatement of what the worker does — every block crossed (tests/_cross_checker.py),
    normalised (tests/_rownorm_checker.py), stepped by the exact valued checker — on rows whose
    crossed nonzeros complete the recipe."""
    style, spec = "cross", "1*2"
    chk, ws, audit = X.Cross(spec), O.Store(O.OPT_FTRL, 1), []
    ws.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))
    tot = sc = 0

    def staged(part, cap):
        nonlocal tot, sc
        (rp, keys, fg, labels, v), = capi.read_blocks(
            str(data / style / ("raw_%s-00000" % part)), cap, values=True)
        crp, ck, _, cv = chk.apply(rp, keys, fg, v)
        assert len(ck) == len(keys) + len(labels)          # one crossed nonzero per row
        y, ss, s = Rn.apply(crp, cv)
        assert set(np.unique(ss).tolist()) == {4.0, 16.0, 64.0}
        tot, sc = tot + len(labels), sc + s
        return crp.astype(np.uint64), ck, y, labels
    rp, ck, y, labels = staged("train", 2 << 20)
    for _ in range(2):
        V.lr_step(ws, rp, ck, y, labels, audit)
    rp, ck, y, labels = staged("test", 4 << 20)
    p = V.lr_predict(ws, rp, ck, y, labels, audit)
    V.assert_exact(audit)
    ll, auc, tp, fp = O.auc_logloss(labels, p)
    x, pred, out, tables = run(data, style, "raw", "cross", capfd, ingest="host", cross=spec,
                               row_norm="l2")
    for a, e in zip(tables[0][:4], ws.export()):
        same(a, e, "table")
    assert pred.decode().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b)
                                              for a, b in zip(p, labels)]
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp"), x.metric("keys")) == (tp, fp, len(ws))
    assert (x.metric("norm_rows"), x.metric("norm_rows_scaled")) == (tot, sc) == (330, 330)
    assert x.metric("cross_out") == x.metric("cross_in") + 330
    assert "row_norm: rows = 240 scaled = 240 left = 0" in out


def test_row_norm_off_is_the_run_without_it(data, capfd):
    """row_norm=off: output, tables, metrics and the launch counters of a run that never heard of
    it; the stage launches nothing"""
    def launches():
        grads = np.zeros(5, np.uint64)
        capi.lib().xf_lr_grad_launches(grads.ctypes.data_as(capi.u64p))
        more = np.array([capi.progress_launches(), capi.lib().xf_weigh_negatives_launches(),
                         capi.RowNorm.launches()], np.uint64)
        return np.concatenate([grads, more]).astype(np.int64)

    def counted(tag, **params):
        at = launches()
        x, pred, out, tables = run(data, "plain", "raw", tag, capfd, ingest="host", **params)
        return x, pred, out, tables, (launches() - at).tolist()
    x, pred_x, out_x, tab_x, n_x = counted("off", row_norm="off")
    y, pred_y, out_y, tab_y, n_y = counted("never")
    assert pred_x == pred_y and out_x == out_y and n_x == n_y and n_x[-1] == 0
    assert not [ln for ln in out_x if "row_norm" in ln]
    for a, e in zip(tab_x[0], tab_y[0]):
        same(a, e, "table")
    for n in METRICS + ("norm_rows", "norm_rows_scaled"):
        assert x.metric(n) == y.metric(n), n
    assert x.metric("norm_rows") == 0


REFUSALS = [
    (dict(feature_values="off"), r"row_norm=l2 needs feature_values=on"),
    (dict(key_build="host"), r"row_norm=l2 together with key_build=host"),
    (dict(parity="reference_order"), r"parity=reference_order"),
    (dict(core_num=2), r"row_norm=l2 needs core_num=1, not core_num=2"),
]


@pytest.mark.parametrize("params,msg", REFUSALS, ids=["feature_values", "key_build", "parity",
                                                      "core_num"])
def test_refusals_by_name_in_and_outside_training(data, tmp_path, params, msg):
    tr, te = str(data / "plain" / "raw_train"), str(data / "plain" / "raw_test")
    p = dict(row_norm="l2", feature_values="on")
    p.update(params)
    with pytest.raises(capi.XFError, match=msg):
        capi.XFlow(tr, te, **p).train()
    # XFLoadModel builds the tables without XFStartTrain's checks in front: the same refusal
    with pytest.raises(capi.XFError, match=msg):
        capi.XFlow(tr, te, **p).load(str(tmp_path / "no_model"))
    with pytest.raises(capi.XFError, match=r"row_norm must be l2 or off, not 'l1'"):
        capi.XFlow(tr, te, row_norm="l1")


def test_row_norm_cannot_change_once_the_stage_exists(data, capfd):
    x, _, _, _ = run(data, "plain", "raw", "change", capfd, ingest="host", row_norm="l2")
    with pytest.raises(capi.XFError, match=r"XFSetParam: row_norm cannot change"):
        x.set("row_norm", "off")
    x.set("row_norm", "l2")                                  # (no change)
    y, _, _, _ = run(data, "plain", "raw", "change2", capfd, ingest="host")
    with pytest.raises(capi.XFError, match=r"XFSetParam: row_norm cannot change"):
        y.set("row_norm", "l2")
