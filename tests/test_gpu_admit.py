"""Feature admission (xf_admit.hip, the worker's admit_count=) on a real MI355X.  The only reference
is the numpy restatement tests/_admit_checker.py (pinned to a plain loop by tests/test_admit_cpu.py);
every comparison is exact — counters, integer arrays, float arrays as their bits.

* the kernels: counters (export after every call) and the filtered arrays over N x h x L, on
  minibatches chosen where they can go wrong — ragged rows with empty rows first, last and in
  runs, one row of 5 000 nonzeros (many tiles), one key 20 000 times (one CAS word), four keys in
  one counter word, NNZ around 256 and around the scatter's tile, R = 0, NNZ = 0 — one after the
  other on ONE filter (the cumulative state), with a read-only call in between, each with no
  companion array, with fgid, with values and with both;
* N = 1 is the identity, down to the table a trainer steps on the filtered minibatch;
* save / load; the worker end to end in three models x two ingest paths against the restatement
  feeding the oracle / the checkers of each mode's own end-to-end test; the model file; the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi

from . import _admit_checker as A
from . import _fmc_checker as FC
from . import _general_cases as GC
from . import _general_checker as G
from . import _interval as I

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%d of %d differ; first (at, got, want): %s" % (
            i.size, a.size, [(j, a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


def tile_size():
    """the scatter's tile, read from the source"""
    src = open(os.path.join(os.path.dirname(HERE), "xflow_amd", "csrc", "xf_admit.hip")).read()
    return int(re.search(r"constexpr uint32_t kAdmitTile = (\d+);", src).group(1))


# ------------------------------------------------------------------ the minibatches
SEED = 0x5eed
POOL = None      # (filled on first use: needs the library)


def pool():
    global POOL
    if POOL is None:
        POOL = capi.hash_decimal_range(0, 3000)
    return POOL


def _csr(lens, keys):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(rowptr[-1]) == len(keys)
    return rowptr, np.asarray(keys, np.uint64)


def word_mates(L, want=4):
    """`want` distinct keys whose slot 0 (seed SEED) falls into the same 32-bit counter word, found
    by search among 100 000 keys (at L = 20 a word is one of 2^18)"""
    cand = capi.hash_decimal_range(0, 100000)
    s0 = A.slots(cand, SEED, L, 1)[0] >> np.uint64(2)
    words, counts = np.unique(s0, return_counts=True)
    assert (counts >= want).any()
    mates = cand[s0 == words[np.argmax(counts >= want)]][:want]
    assert len(set(mates.tolist())) == want
    return mates


def minibatches(L):
    """[(name, rowptr, keys, update)] in the order they are applied to one filter"""
    rng = np.random.RandomState(17)
    P = pool()
    out = []
    # a fresh filter's first minibatch: a few hundred nonzeros, most keys once or twice — at
    # L = 10 far from saturating anything, so nonzeros ARE dropped whatever N and h
    lens = rng.randint(0, 12, size=60)
    n = int(lens.sum())
    out.append(("first_touch",) + _csr(lens, P[np.minimum(rng.zipf(1.5, size=n), len(P)) - 1]) + (True,))
    # ragged: ~3000 rows of 0 .. 60 nonzeros, empty rows first, last and in runs; power-law keys
    lens = rng.randint(0, 61, size=3000)
    lens[:3] = 0
    lens[-2:] = 0
    lens[1000:1040] = 0
    lens[rng.rand(3000) < 0.05] = 0
    n = int(lens.sum())
    out.append(("ragged",) + _csr(lens, P[np.minimum(rng.zipf(1.3, size=n), len(P)) - 1]) + (True,))
    # one row of 5000 nonzeros between short rows
    lens = np.array([3, 0, 5000, 0, 7])
    out.append(("long_row",) + _csr(lens, P[rng.randint(0, len(P), size=int(lens.sum()))]) + (True,))
    # one key 20 000 times, among others
    keys = P[rng.randint(0, len(P), size=24000)]
    keys[rng.permutation(24000)[:20000]] = P[2999]
    out.append(("hot_key",) + _csr(np.full(480, 50), keys) + (True,))
    # four keys of one counter word, a few occurrences each, row by row
    m = word_mates(L)
    out.append(("word_mates",) + _csr([4, 4, 4, 0, 4], np.tile(m, 4)) + (True,))
    # a read-only call: filters by the present state, changes nothing
    lens = rng.randint(0, 20, size=400)
    out.append(("read_only",) + _csr(lens, P[rng.randint(0, len(P), size=int(lens.sum()))]) + (False,))
    T = tile_size()
    for n in (255, 256, 257, T - 1, T, T + 1):
        lens = np.array([n - n // 2, 0, n // 2])
        out.append(("nnz%d" % n,) + _csr(lens, P[np.minimum(rng.zipf(1.2, size=n), len(P)) - 1]) + (True,))
    out.append(("no_rows", np.zeros(1, np.uint64), np.zeros(0, np.uint64), True))
    out.append(("no_nonzeros", np.zeros(6, np.uint64), np.zeros(0, np.uint64), True))
    out.append(("ragged_again",) + out[1][1:3] + (True,))
    return out


def companions(keys):
    """an fgid and a value per nonzero that say where the nonzero came from"""
    n = len(keys)
    return (np.arange(n, dtype=np.int32) % 977,
            (np.arange(n, dtype=np.float32) * np.float32(0.25) - np.float32(3)).astype(np.float32))


GRID = [(N, h, L) for L in (2, 10, 20) for h in (1, 3, 4) for N in (1, 2, 3, 255)]


@pytest.mark.parametrize("N,h,L", GRID, ids=["N%d-h%d-L%d" % g for g in GRID])
def test_counters_and_filtered_arrays(N, h, L):
    mbs = minibatches(L)
    assert len([m for m in mbs if m[3]]) >= 5                  # cumulative state over many calls
    # the restatement first: the expected state and arrays of every call, and that the case is
    # worth running — before the GPU is asked anything
    ref = A.Filter(L, N, h, SEED)
    expect, seen_times = [], {}
    kept = dropped = false_adm = 0
    for name, rowptr, keys, update in mbs:
        fg, vs = companions(keys)
        if update:
            for k, c in zip(*np.unique(keys, return_counts=True)):
                seen_times[int(k)] = seen_times.get(int(k), 0) + int(c)
        rp, ks, efg, evs = ref.filter(rowptr, keys, fg, vs, update=update)
        expect.append((rp, ks, efg, evs, ref.c.copy(), (ref.seen, ref.kept)))
        kept += len(ks)
        dropped += len(keys) - len(ks)
        false_adm += sum(1 for k in np.unique(ks) if seen_times.get(int(k), 0) < N)
        if name == "read_only":
            assert np.array_equal(ref.c, expect[-2][4])
        if N == 1 and update:
            assert len(ks) == len(keys)
    if L == 10 and N > 1:
        assert kept > 0 and dropped > 0 and false_adm > 0, (kept, dropped, false_adm)
    for with_fg, with_vs in ((False, False), (True, False), (False, True), (True, True)):
        flt = capi.Admit(L, N, hashes=h, seed=SEED)
        assert not flt.export().any()
        for (name, rowptr, keys, update), (rp, ks, efg, evs, ctr, stats) in zip(mbs, expect):
            fg, vs = companions(keys)
            got = flt.apply(rowptr, keys, fgid=fg if with_fg else None,
                            values=vs if with_vs else None, update=update)
            same(flt.export(), ctr)
            same(got[0], rp)
            same(got[1], ks)
            at = 2
            if with_fg:
                same(got[at], efg)
                at += 1
            if with_vs:
                same(got[at], evs)
                at += 1
            assert len(got) == at and flt.stats() == stats, name


def test_labels_and_rows_are_untouched():
    rng = np.random.RandomState(3)
    name, rowptr, keys, _ = minibatches(10)[1]
    labels = rng.randint(0, 2, size=len(rowptr) - 1).astype(np.int32)
    flt, ref = capi.Admit(10, 3, seed=SEED), A.Filter(10, 3, 3, SEED)
    rp, ks, lb = flt.apply(rowptr, keys, labels=labels)
    erp, eks, _, _ = ref.filter(rowptr, keys)
    same(rp, erp)
    same(ks, eks)
    same(lb, labels)
    assert len(rp) == len(rowptr) and 0 < len(ks) < len(keys)
    # a row slice of a block (host arrays whose first offset is not 0), read-only
    d = flt.apply(rowptr[100:301], keys, labels=labels[100:300], update=False)
    erp, eks, _, _ = ref.filter(rowptr[100:301], keys, update=False)
    same(d[0], erp)
    same(d[1], eks)


def test_bad_arguments():
    for args in ((1, 2, 3), (33, 2, 3), (10, 0, 3), (10, 256, 3), (10, 2, 0), (10, 2, 9)):
        with pytest.raises(capi.XFError, match="admit_"):
            capi.Admit(args[0], args[1], hashes=args[2])
    flt = capi.Admit(4, 2)
    with pytest.raises(capi.XFError, match="descend"):
        flt.apply(np.array([0, 3, 2], np.uint64), np.zeros(3, np.uint64))
    with pytest.raises(capi.XFError, match="above admit_count"):
        flt.import_(np.full(16, 3, np.uint8))


# ------------------------------------------------------------------ N = 1: the identity
def test_count_one_is_the_identity():
    rng = np.random.RandomState(5)
    for name, rowptr, keys, update in minibatches(10):
        if not update:
            continue
        fg, vs = companions(keys)
        labels = rng.randint(0, 2, size=len(rowptr) - 1).astype(np.int32)
        rp, ks, lb, gfg, gvs = capi.Admit(10, 1, seed=SEED).apply(rowptr, keys, labels, fg, vs)
        for got, want in ((rp, rowptr.astype(np.uint32)), (ks, keys), (lb, labels), (gfg, fg),
                          (gvs, vs)):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
    # binary LR: a table stepped on the filtered device arrays is the table stepped on the minibatch
    name, rowptr, keys, _ = minibatches(10)[1]
    labels = rng.randint(0, 2, size=len(rowptr) - 1).astype(np.int32)
    flt = capi.Admit(10, 1, seed=SEED)
    a = capi.Sharded(model="lr", capacity=1 << 14)
    b = capi.Sharded(model="lr", capacity=1 << 14)
    for _ in range(3):
        d = flt.apply_dev(rowptr, keys, labels)
        assert (d.R, d.NNZ) == (len(labels), len(keys))
        a.step(a.compile_dev(*d[:5]))
        a.check()
        b.step(b.compile(rowptr, keys, labels))
        b.check()
    for x, y in zip(a.w.export(), b.w.export()):
        same(x, y)
    assert len(a.w) > 100


# ------------------------------------------------------------------ save / load
def test_round_trip(tmp_path):
    name, rowptr, keys, _ = minibatches(10)[1]
    flt = capi.Admit(10, 3, hashes=4, seed=99)
    flt.apply(rowptr, keys)
    path = str(tmp_path / "f.admit")
    flt.save(path)
    twin = capi.Admit(10, 3, hashes=4, seed=99)
    twin.load(path)
    same(twin.export(), flt.export())
    assert flt.export().any()
    same(twin.apply(rowptr, keys, update=False)[1], flt.apply(rowptr, keys, update=False)[1])
    for other in (dict(count=2), dict(log2_slots=11), dict(hashes=3), dict(seed=98)):
        p = dict(log2_slots=10, count=3, hashes=4, seed=99)
        p.update(other)
        with pytest.raises(capi.XFError, match=r"saved with admit_log2_slots=10 admit_hashes=4 "
                                               r"admit_count=3 seed=99, this filter has"):
            capi.Admit(**p).load(path)
    with pytest.raises(capi.XFError, match="nothere.admit"):
        twin.load(str(tmp_path / "nothere.admit"))
    open(path, "r+b").truncate(500)
    with pytest.raises(capi.XFError, match="ends before"):
        twin.load(path)


# ------------------------------------------------------------------ the worker end to end
FIELDS, K = 18, 4
MODELS = {
    "lr": (dict(model=0), "gpu"),
    "canonical": (dict(model=1, k=K, fm_mode="canonical"), "gpu_fields"),
    "field_aware+values": (dict(model=1, k=K, fm_mode="field_aware", fields=FIELDS,
                                feature_values="on", optimizer="sgd"), "gpu_fields"),
}
ADMIT = dict(admit_count=2, admit_log2_slots=12)


def zipf_text(seed, nbytes):
    """a training file in the manner of tests/_ingest_fields_cases.py's worker_text — field0 in
    [0, FIELDS), values of a few digits — with power-law fids: 300 hot ones (Zipf 1.1) and, one
    token in a thousand, a fid from a large space that occurs once or twice in the whole file"""
    rng = np.random.RandomState(seed)
    vals = ["1", "0.5", "2", "-1.25", "0.25", "3.5", "-0.75", "", "0.125", "1.5"]
    rows = nbytes // 30 + 1
    ntok = rng.randint(3, 15, size=rows)
    n = int(ntok.sum())
    p = 1.0 / np.arange(1, 301) ** 1.1
    fid = rng.choice(300, size=n, p=p / p.sum())
    rare = rng.rand(n) < 0.001
    fid[rare] = 1000 + rng.randint(0, 400, size=int(rare.sum())) * 7 + seed % 7 * 3000
    f, vi, lab = rng.randint(0, FIELDS, size=n), rng.randint(0, len(vals), size=n), rng.rand(rows) < 0.4
    toks = ["%d:%d:%s" % (f[i], fid[i], vals[vi[i]]) for i in range(n)]
    lines, size, at = [], 0, 0
    for r in range(rows):
        if size >= nbytes:
            break
        line = ("%d\t" % lab[r] + " ".join(toks[at:at + ntok[r]]) + "\n").encode()
        at += ntok[r]
        lines.append(line)
        size += len(line)
    return b"".join(lines)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("admit")
    # (the seed: the field-aware checker's sums are not exact in fp64, and a hot key's gv is one
    # sum of ~10^5 products of either sign; with seeds 21, 23, 24, 27, 29 the interval rule leaves
    # one or two of 149 000 such sums open — two adjacent fp32 candidates —, with 25, 26, 28 none,
    # in both the replaying and the recounting run: found with the checker alone)
    train = zipf_text(25, (2 << 20) + (200 << 10))
    assert 2 << 20 < len(train) < 3 << 20                        # three 1 MiB blocks
    (d / "train-00000").write_bytes(train)
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10))
    return d


class Model:
    """the oracle / checker of one mode, minibatch by minibatch, as that mode's own end-to-end
    test drives it: LR the exact-sum oracle, canonical FM tests/_fmc_checker.py, field-aware FM
    with values tests/_general_checker.py — its sums are not exact in fp64, the interval rule of
    tests/_interval.py must pin every one of them to a single fp32 value (no open sum: asserted
    before anything is compared)"""

    def __init__(self, name):
        self.name, self.judge = name, None
        key0 = np.zeros(1, np.uint64)
        if name == "lr":
            self.ws, self.vs = O.Store(O.OPT_FTRL, 1), None
        elif name == "canonical":
            self.ws, self.vs = FC.stores(O.OPT_FTRL, K, 0)
        else:
            self.ws, self.vs = GC.stores("ffm", "sgd", FIELDS, K, seed=0)
            self.judge = I.Judge()
            self.run = G.Run("ffm", self.ws, self.vs, self.judge, FIELDS)
        self.ws.push(key0, np.zeros(1, np.float32))              # the worker's init push of key 0
        if self.vs is not None:
            self.vs.push(key0, np.zeros(self.vs.dim, np.float32))

    def step(self, mb):
        rp, keys, fg, vals, labels = mb
        if self.name == "lr":
            if len(keys):
                with O.sum_mode(1):
                    O.lr_update(self.ws, O.Batch(rp, keys, labels))
        elif self.name == "canonical":
            FC.step(self.ws, self.vs, rp, keys, labels)
        else:
            self.run.step((rp, keys, fg, vals, labels))

    def predict(self, mb):
        rp, keys, fg, vals, labels = mb
        if self.name == "lr":
            if not len(keys):
                return FC._sigmoid(np.zeros(len(labels), np.float32))
            with O.sum_mode(1):
                b = O.Batch(rp, keys, labels)
                return b.lr_loss(self.ws.pull(b.ukeys))[1]
        if self.name == "canonical":
            return FC.predict(self.ws, self.vs, rp, keys, labels)
        return self.run.predict((rp, keys, fg, vals, labels))[:, 0]


_refs = {}


def reference(data, name, recount):
    """the restatement does what the worker does: the training blocks filtered in file order with
    update, the second epoch replaying the first epoch's filtered minibatches (recount: filtering
    and counting again), the test blocks filtered read-only"""
    if (name, recount) in _refs:
        return _refs[name, recount]
    flt, m = A.Filter(12, 2, 3, 0), Model(name)                  # the worker's seed: 0
    blocks = list(capi.read_blocks(str(data / "train-00000"), 1 << 20, values=True))
    assert len(blocks) == 3

    def admitted(blk, update):
        rp, keys, fg, labels, vals = blk
        frp, fk, ffg, fv = flt.filter(rp, keys, fg, vals, update=update)
        return frp.astype(np.uint64), fk, ffg, fv, labels

    first = None
    for epoch in range(2):
        mbs = [admitted(b, True) for b in blocks] if epoch == 0 or recount else first
        if epoch == 0:                                           # worth running: kept AND dropped
            assert all(0 < len(mb[1]) < len(b[1]) for mb, b in zip(mbs, blocks))
        first = first or mbs
        for mb in mbs:
            m.step(mb)
    cap = (4 << 20) if name == "lr" else (2 << 20)
    labs, ps, dropped = [], [], 0
    for blk in capi.read_blocks(str(data / "test-00000"), cap, values=True):
        mb = admitted(blk, False)
        dropped += len(blk[1]) - len(mb[1])
        ps.append(m.predict(mb))
        labs.append(blk[3])
    assert dropped > 0                                           # the test file's unseen keys
    if m.judge is not None:
        assert m.judge.open_count() == 0, m.judge.format(name)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    _refs[name, recount] = (m, lab, p, O.auc_logloss(lab, p), (flt.seen, flt.kept), flt.c.copy())
    return _refs[name, recount]


def check_worker(x, pred, ref, name):
    m, lab, p, (ll, auc, tp, fp), stats, _ = ref
    opt = capi.OPT_SGD if name.startswith("field_aware") else capi.OPT_FTRL
    wh, vh = x.tables()
    tabs = [(capi.Table.from_handle(wh, 1, opt), m.ws)]
    if m.vs is not None:
        tabs.append((capi.Table.from_handle(vh, m.vs.dim, opt), m.vs))
    for t, s in tabs:
        for a, e in zip(t.export()[:4 if opt == capi.OPT_FTRL else 2], s.export()):
            same(a, e)
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    assert x.metric("keys") == len(m.ws)
    assert (x.metric("admit_seen"), x.metric("admit_kept")) == stats


def run_worker(data, name, ingest, tag, **extra):
    pred = str(data / ("pred_%s_%s.txt" % (name, tag)))
    p = dict(MODELS[name][0], **ADMIT)
    p.update(extra)
    x = capi.XFlow(str(data / "train"), str(data / "test"), block_size_mb=1, capacity=1 << 14,
                   ingest=ingest, pred_path=pred, **p)
    x.train()
    return x, pred


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_worker_end_to_end(data, name, ingest):
    ingest = MODELS[name][1] if ingest == "gpu" else "host"
    ref = reference(data, name, False)
    x, pred = run_worker(data, name, ingest, ingest, epochs=2)
    assert x.metric("blocks_gpu") == (0 if ingest == "host" else 3)
    check_worker(x, pred, ref, name)


@pytest.mark.parametrize("name", ["lr", "field_aware+values"])
def test_worker_counts_again_without_the_batch_cache(data, name):
    ref = reference(data, name, True)
    assert ref[4] != reference(data, name, False)[4]             # (twice the nonzeros were seen)
    x, pred = run_worker(data, name, MODELS[name][1], "recount", epochs=2, cache_batches=0)
    check_worker(x, pred, ref, name)


def test_admission_off_is_todays_worker(data):
    """admit_count=0 with the other two set: nothing is created, the run is the plain one"""
    runs = []
    for extra in ({}, dict(admit_count=0, admit_log2_slots=5, admit_hashes=8)):
        pred = str(data / ("pred_off%d.txt" % len(runs)))
        x = capi.XFlow(str(data / "train"), str(data / "test"), block_size_mb=1, epochs=1,
                       capacity=1 << 14, pred_path=pred, **extra)
        x.train()
        wh, _ = x.tables()
        runs.append((capi.Table.from_handle(wh, 1).export(), open(pred).read()))
        assert x.metric("admit_seen") == 0 and x.metric("admit_kept") == 0
    for a, b in zip(runs[0][0], runs[1][0]):
        same(a, b)
    assert runs[0][1] == runs[1][1]
    assert len(runs[0][0][0]) > len(reference(data, "lr", False)[0].ws)    # admission keeps keys out


def test_model_file_carries_the_filter(data, tmp_path):
    name = "field_aware+values"
    ref = reference(data, name, False)
    ckpt = str(tmp_path / "m.bin")
    x, pred = run_worker(data, name, "host", "save", epochs=2, model_out=ckpt)
    saved = capi.Admit(12, 2)
    saved.load(ckpt + ".admit")
    same(saved.export(), ref[5])
    y, pred2 = run_worker(data, name, "host", "load", epochs=0, model_in=ckpt)
    assert open(pred2).read() == open(pred).read()
    assert y.metric("keys") == x.metric("keys") and y.metric("admit_seen") == 0
    os.unlink(ckpt + ".admit")
    with pytest.raises(capi.XFError, match=re.escape(ckpt + ".admit")):
        run_worker(data, name, "host", "load2", epochs=0, model_in=ckpt)
    # a save with admission off removes a stale filter file
    open(ckpt + ".admit", "wb").write(b"stale")
    z = capi.XFlow(str(data / "train"), str(data / "test"), block_size_mb=1, epochs=0,
                   capacity=1 << 14, pred_path=str(tmp_path / "z.txt"), model_in=ckpt,
                   **MODELS[name][0])
    z.train()
    z.save(ckpt)
    assert not os.path.exists(ckpt + ".admit")


def test_cli_prints_the_same_metric_line(data, tmp_path):
    _, lab, p, (ll, auc, tp, fp), _, _ = reference(data, "lr", False)
    out = subprocess.run([os.path.join(build.LIBDIR, "xflow_lr"), str(data / "train"),
                          str(data / "test"), "0", "2", "block_size_mb=1", "capacity=16384",
                          "pred_path=cli.txt", "admit_count=2", "admit_log2_slots=12"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == \
        ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
