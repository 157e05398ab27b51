"""k_lr_grad_dense (xf_cells_grad_dense.hip: the gradient + Push of the steady state) on
minibatches placed by state row (tests/_cells_edges.py), on a real MI355X.

launch_grad takes the dense kernel only for one source, at most four row windows and NO split
chunk; which kernel ran is read from the launch counters (capi.lr_grad_launches), and every case
asserts it.  Every case is held against the exact-sum oracle bit for bit, in the scheme of
tests/test_gpu_entry_streams.py: the losses of three steps, the whole table after them — the keys
no minibatch touches included: the table is settled with every key first, so that the key of rank r
owns state row r, and it starts many steps old (aged(): a weight of its own per key) — and
xf_table_check.  FTRL and SGD; kept minibatches (xf_batch_compile_local) and
one-shot ones (xf_lr_update_dev: the other key build lays out the same cells)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _cells_edges as E
from . import _hyper_cases as HC
from . import _negsample_checker as N
from . import _valued_cases as VC
from .test_gpu_entry_streams import same

pytestmark = pytest.mark.gpu
STEPS = 3
OPTS = ["ftrl", "sgd"]
CASES = {c.name: c for c in E.grad_cases()}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


_KEYS = {}


def keys_of(M):
    """M keys in key order: after pull + defrag, key r owns state row r"""
    if M not in _KEYS:
        _KEYS[M] = np.sort(capi.hash_decimal_range(0, M))
    return _KEYS[M]


def capacity_for(nkeys):
    """a power of two with room for the keys (a table holds state rows for 3/4 of its capacity)
    and for the few a test adds"""
    return 1 << max(17, (2 * nkeys).bit_length())


def aged(M, opt):
    """a table "many steps old" over keys_of(M) (tests/_valued_cases.py: old_state): every key its
    own weight, so that the losses depend on which rows the forward read and a key's gradient is
    no sum of +-0.5 that cancels.  (On a fresh table three steps leave every loss at
    sigmoid(0) - y: FTRL's w stays 0 below lambda1, SGD's 1e-8 rounds away inside the sigmoid.)"""
    return VC.old_state(keys_of(M), opt, 1, "w")


def _opt(opt):
    return (capi.OPT_FTRL, O.OPT_FTRL) if opt == "ftrl" else (capi.OPT_SGD, O.OPT_SGD)


def reference(raws, opt, settle, state=None, hyper=None, late=None):
    """the oracle's losses of STEPS steps over raws (cycled) and its table after them.  state: a
    model (keys, w, n, z) to import instead of the fresh keys `settle`; hyper: the set the table is
    made under; late: the set it gets with its keys already in"""
    s = O.Store(_opt(opt)[1], 1)
    if hyper is not None:
        hyper.to_store(s)
    if state is not None:
        s.import_(*state)
    else:
        s.pull(settle)
    if late is not None:
        late.to_store(s)
    losses = [N.lr_step(s, *raws[i % len(raws)], np.float32(1.0)) for i in range(STEPS)]
    return losses, s.export()


def gpu_run(raws, opt, settle, form="kept", tune=(), state=None, hyper=None, late=None):
    """the same on the GPU -> losses, table, cells_info per step, launches per kind during the
    steps, whether the table vouched for w when they began"""
    for k, v in tune:
        capi.tune(k, v)
    try:
        t = capi.Table(_opt(opt)[0], 1, capacity=capacity_for(len(settle)),
                       **(hyper.kw() if hyper else {}))
        ws = capi.Workspace()
        if state is not None:
            t.import_(*state)
        else:
            t.pull(settle)
        t.defrag()
        if late is not None:
            late.to_table(t)
        derived = t.w_derived() if opt == "ftrl" else False
        kept = [capi.LocalBatch(t, *r) for r in raws] if form == "kept" else None
        losses, infos = [], []
        n0 = capi.lr_grad_launches()
        for i in range(STEPS):
            if kept:
                b = kept[i % len(raws)]
                capi.lr_step(t, b, ws)
            else:
                b = capi.LocalBatch.update(t, ws, *raws[i % len(raws)], retain_keys=False)
            losses.append(ws.fetch_loss(b.R))
            infos.append(b.cells_info())
        n1 = capi.lr_grad_launches()
        t.check()
        return losses, t.export(), infos, {k: n1[k] - n0[k] for k in n1}, derived
    finally:
        for k, _ in tune:
            capi.tune(k, 0)


def against(got, ref, opt, what):
    for i, (a, e) in enumerate(zip(got[0], ref[0])):
        same(a, e, "%s: loss of step %d" % (what, i))
    m = 4 if opt == "ftrl" else 2
    for nm, a, e in zip(("keys", "w", "n", "z"), got[1][:m], ref[1][:m]):
        same(a, e, "%s: table %s" % (what, nm))


def launched(n, kernel, launches=STEPS, finish=0, derived=None):
    """the counters of a run: `launches` of `kernel` (dense_masked / dense_full / cells) and of no
    other gradient kernel, `finish` of k_lr_grad_split_finish; derived: how many of the dense
    launches derived the old weight (None: not looked at)"""
    want = dict(dense_masked=0, dense_full=0, cells=0, split_finish=finish)
    want[kernel] = launches
    got = {k: n[k] for k in want}
    assert got == want, (got, want)
    if derived is not None:
        assert n["dense_derived"] == derived, (n, derived)


_REF = {}


def ref_of(name, opt):
    """a case's minibatch and the oracle's run of it: once per case and optimizer, left unchanged"""
    if (name, opt) not in _REF:
        c = CASES[name]
        raws = [c.raw(keys_of(c.M))]
        _REF[(name, opt)] = (raws, reference(raws, opt, keys_of(c.M), state=aged(c.M, opt)))
    return _REF[(name, opt)]


def check_case(name, opt, form="kept", tune=(), kernel=None):
    c = CASES[name]
    raws, ref = ref_of(name, opt)
    got = gpu_run(raws, opt, keys_of(c.M), form, tune, state=aged(c.M, opt))
    against(got, ref, opt, "%s, %s, %s %s" % (name, opt, form, tune))
    L = c.layout()
    for info in got[2]:
        assert (info["nwin"], info["W"], info["nchunk"], info["M"], info["segments"]) == \
            (L["nwin"], L["W"], L["nchunk"], c.M, 1), info
        assert (info["nsplit_chunks"], info["nitems"]) == (L["nsplit"], L["nitems"]), info
    launched(got[3], kernel or c.kernel, finish=STEPS if L["nsplit"] else 0)
    return got


def names(prefix):
    return [n for n in CASES if n.startswith(prefix)]


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("form", ["kept", "one-shot"])
@pytest.mark.parametrize("name", names("gate-"))
def test_the_gate(name, form, opt):
    """an unsplit minibatch of 1, 2, 3 and 4 row windows (R = 17408, 17409, 34817, 52225, 69632)
    runs dense, 5 windows (69633) the general kernel; a chunk of 8192 entries stays dense, 8193
    send the whole minibatch to the general kernel and the finish kernel"""
    check_case(name, opt, form)


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name", names("store-"))
def test_the_store_variant(name, opt):
    """one entry either side of dense_touch's threshold: the shape picks byte-masked (3071) or
    whole-line stores (3072) by itself; each forced the other way (lr_gradient = 2 / 3) and through
    the general kernel (lr_gradient = 1): the same losses and table, the oracle's"""
    runs = [check_case(name, opt),
            check_case(name, opt, tune=[("lr_gradient", 2)], kernel="dense_masked"),
            check_case(name, opt, tune=[("lr_gradient", 3)], kernel="dense_full"),
            check_case(name, opt, tune=[("lr_gradient", 1)], kernel="cells")]
    for r in runs[1:]:
        for a, b in zip(runs[0][0] + list(runs[0][1]), r[0] + list(r[1])):
            same(a, b, "%s: one variant against another" % name)


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("form", ["kept", "one-shot"])
@pytest.mark.parametrize("var", [2, 3], ids=["masked", "full"])
@pytest.mark.parametrize("name", names("window") + names("round-"))
def test_windows_and_rounds(name, var, form, opt):
    """windows-*: at four windows and at two, chunks whose entries lie in every window, only in
    window 0, only in the last, only in the first and last, only in the middle ones, one entry per
    window; window-ends-*: row-in-window 0 and W - 1 of every window and row R - 1 of a shorter
    last window.  round-totals: chunks of 1, 2047, 2048, 2049, 4096, 4097, 8191 and 8192 entries
    (2048 per trip of the accumulate loop); round-boundaries: a trip's boundary inside a window's
    cell, and exactly on a cell boundary (c1 == 2048).  Both store variants."""
    check_case(name, opt, form, tune=[("lr_gradient", var)],
               kernel="dense_masked" if var == 2 else "dense_full")


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("var", [0, 2, 3], ids=["by-shape", "masked", "full"])
@pytest.mark.parametrize("name", ["positions-0-1-2047", "key-twice-in-a-row",
                                  "one-key-8192-times", "all-2048-positions-once",
                                  "first-and-last-of-30-chunks"])
def test_positions(name, var, opt):
    """positions 0, 1 and 2047 of a chunk; a key twice in one row; one key taking all 8192 entries
    of its chunk; all 2048 positions touched once each; only the first and the last chunk of a
    30-chunk table touched — the rows between keep their bits (the whole table is compared)"""
    kernel = {0: None, 2: "dense_masked", 3: "dense_full"}[var]
    got = check_case(name, opt, tune=[("lr_gradient", var)] if var else (), kernel=kernel)
    if name == "first-and-last-of-30-chunks":
        assert got[2][0]["nitems"] == 2
        w, w0 = got[1][1], aged(CASES[name].M, opt)[1].ravel()
        same(w[E.CHUNK:29 * E.CHUNK], w0[E.CHUNK:29 * E.CHUNK], "the chunks between")
        assert (w[:E.CHUNK] != w0[:E.CHUNK]).any() and (w[29 * E.CHUNK:] != w0[29 * E.CHUNK:]).any()


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("var", [2, 3], ids=["masked", "full"])
@pytest.mark.parametrize("name", names("end-"))
def test_the_end_of_the_index_space(name, var, opt):
    """M = 2048c - 1, 2048c, 2048c + 1 with the last state row touched; then minibatches that bring
    new keys: a second segment of cells (chunk0 != 0) whose rows start from fresh state, and both
    segments run dense"""
    c = CASES[name]
    check_case(name, opt, tune=[("lr_gradient", var)],
               kernel="dense_masked" if var == 2 else "dense_full")
    settle = keys_of(c.M)
    new = np.setdiff1d(capi.hash_decimal_range(10 ** 7, 60), settle)
    rng = np.random.RandomState(c.M)
    more_rows = np.concatenate([[0, c.R - 1], rng.randint(0, c.R, size=3 * len(new) - 2)])
    more = (more_rows, np.tile(new, 3))
    raws = [c.raw(settle), c.raw(settle, seed=1, more=more), c.raw(settle, seed=2, more=more)]
    ref = reference(raws, opt, settle, state=aged(c.M, opt))
    assert len(ref[1][0]) == c.M + len(new)
    for form in ("kept", "one-shot"):
        got = gpu_run(raws, opt, settle, form, [("lr_gradient", var)], state=aged(c.M, opt))
        against(got, ref, opt, "%s + new keys, %s" % (name, form))
        # (kept: all three are compiled before step 0, and the new keys arrive with the second)
        assert [i["segments"] for i in got[2]] == [1, 2, 2], got[2]
        launched(got[3], "dense_masked" if var == 2 else "dense_full", launches=5)


# ------------------------------------------------------------------------- the old weight
def _model(name):
    """a model the oracle made on the case's own stream from the aged table: (keys, w, n, z) of
    every key, the weights away from zero"""
    c = CASES[name]
    return reference([c.raw(keys_of(c.M), seed=7)], "ftrl", keys_of(c.M),
                     state=aged(c.M, "ftrl"))[1]


_OW_REF = {}


@pytest.mark.parametrize("ow", [0, 1, 2])
@pytest.mark.parametrize("var", [0, 2, 3], ids=["by-shape", "masked", "full"])
@pytest.mark.parametrize("name", names("store-"))
@pytest.mark.parametrize("state", ["fresh", "w_odd", "set_hyper", "NEG_L1"])
def test_the_old_weight_in_the_dense_kernel(state, name, var, ow):
    """k_lr_grad_dense derives the old weight from (n, z) only while the table vouches for that
    (TableDev::w_of_nz) and the shape or old_weight = 2 asks for it; a whole-line store writes
    ftrl_w_of(n, z) back into the rows the minibatch did not touch.  On a fresh table; on a model
    imported with rows whose w is NOT the w of their (n, z) — untouched rows keep that w —; after
    set_hyper with the keys already in the table; under NEG_L1 (a fresh row's w is not
    ftrl_w_of(0, 0)).  Both store variants, old_weight = 0 / 1 / 2, the oracle's losses and table
    each time, and from the counters the kernel, the variant and whether w was derived."""
    c = CASES[name]
    settle = keys_of(c.M)
    raws = [c.raw(settle)]
    kw = {}
    vouches = True
    if state == "w_odd":
        k, w, n, z = _model(name)
        touched = np.isin(np.arange(c.M), c.srows)
        # an untouched row between touched ones (a whole-line store rewrites it), and a touched one
        odd = [int(np.flatnonzero(~touched)[5]), int(np.flatnonzero(touched)[9]), c.M - 1]
        w = w.copy()
        w[odd] = np.float32([0.25, -0.5, 0.125])
        kw, vouches = dict(state=(k, w, n, z)), False
    elif state == "set_hyper":
        kw, vouches = dict(state=_model(name), late=HC.A), False
    elif state == "NEG_L1":
        kw, vouches = dict(hyper=HC.NEG_L1), False
    if (state, name) not in _OW_REF:            # (shared by the nine knob settings, unchanged)
        _OW_REF[(state, name)] = reference(raws, "ftrl", settle, **kw)
    ref = _OW_REF[(state, name)]
    tune = ([("lr_gradient", var)] if var else []) + ([("old_weight", ow)] if ow else [])
    got = gpu_run(raws, "ftrl", settle, "kept", tune, **kw)
    against(got, ref, "ftrl", "%s, %s, %s" % (name, state, tune))
    assert got[4] == vouches
    kernel = {0: c.kernel, 2: "dense_masked", 3: "dense_full"}[var]
    # launch_grad: read w where the table does not vouch, under old_weight = 1, and — unless
    # old_weight = 2 — where the SHAPE touches the table densely (whatever variant is forced)
    derives = vouches and ow != 1 and not (c.kernel == "dense_full" and ow != 2)
    launched(got[3], kernel, derived=STEPS if derives else 0)
    if state == "w_odd":
        same(got[1][1][odd[0]], np.float32(0.25), "the untouched row's odd w")
