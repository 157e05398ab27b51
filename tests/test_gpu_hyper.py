"""Every optimizer step away from the default hyper-parameters, on a real MI355X.

The points are those of tests/_hyper_cases.py: FTRL A, NO_L1 (lambda1 == 0), SPARSE (an L1 that
zeroes a fifth to four fifths of what it touches), NEG_L1 (lambda1 < 0), SGD lr 0.05 and 0.2.  A
step that takes a weight table and a factor table gives them DIFFERENT sets; one case per form
changes both tables' sets in mid-run (xf_table_set_hyper), on minibatches compiled before the
change and on fresh ones.  The checkers are the existing ones: tests/_general_checker.py under the
interval rule (the asserts of tests/test_gpu_general_position.py's _run), O.fm_update / O.lr_update
in sum_mode(1) bit for bit.  tests/test_general_position_cpu.py forms every stream here with the
oracle alone first (the cap, SPARSE's shares, and that a kernel mixing the sets up would fail).

div_by_const with its guard of the subnormal range, and the table's verdict on its alpha, run on
the device at the end of this file (tests/test_div_by_alpha_cpu.py is their host restatement)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _general_checker as G
from . import _hyper_cases as HC
from . import _interval as I
from . import test_gpu_general_position as GP      # same, one_of, table_is (the module's helpers)
from .test_div_by_alpha_cpu import inexact_list

pytestmark = pytest.mark.gpu
same, one_of, table_is = GP.same, GP.one_of, GP.table_is


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


def _derived_as_it_should(t, h):
    """a fresh FTRL w table vouches for w = ftrl_w_of(n, z) exactly when lambda1 >= 0"""
    if h.opt == "ftrl":
        assert t.w_derived() == (h.lambda1 >= 0), h


# ---------------------------------------------------------- 1. the interval checker's forms
def _run(plan, local=False, precompiled=False):
    """tests/test_gpu_general_position.py's _run with a set per table and, for a plan of two
    phases, the change before step HC.SWITCH.  local: the valued local build (cells; such a step
    forms neither the pulled weights nor the per-key gradients).  precompiled: every minibatch is
    compiled before step 0 — a minibatch, workspace or table that kept the values it first saw
    steps 2 and 3 with them."""
    form, fields, sgd = plan.form, plan.fields, plan.opt == "sgd"
    mbs = plan.stream()
    judge = I.Judge()
    sw, sv = plan.stores()
    run = G.Run(form, sw, sv, judge, fields)
    hw, hv = plan.phases[0]
    tw = capi.Table(_go(plan.opt), 1, capacity=1 << 16, **hw.kw())
    tv = None if form == "lr" else capi.Table(_go(plan.opt), sv.dim, capi.INIT_HASHNORM, 0.0,
                                              seed=plan.seed(), capacity=1 << 16, **hv.kw())
    _derived_as_it_should(tw, hw)
    ws = capi.Workspace()
    if form == "ffm":
        ws.fm_fields(fields)
        ws.fm_mode("field_aware")
    elif form == "fm":
        ws.fm_mode("canonical")

    def compiled(i):
        rowptr, keys, fg, vals, labels = mbs[i]
        if local:
            return capi.LocalBatch(tw, rowptr, keys, labels, values=vals)
        extra = {"fields": fields, "fgid": fg} if form == "ffm" else {}
        return capi.Batch(rowptr, keys, labels, on_gpu=i != 1, values=vals, **extra)

    pre = [compiled(i) for i in range(len(mbs))] if precompiled else None
    if pre and local:       # the local build has entered every minibatch's keys: zeros, as a Pull's
        sw.pull(np.unique(np.concatenate([mb[1] for mb in mbs])))
    b = None
    for i, mb in enumerate(mbs):
        new = plan.phase_at(i)
        if new:
            for h, t, s in ((new[0], tw, sw), (new[1], tv, sv)):
                if t is not None:
                    h.to_table(t)
                    h.to_store(s)
            if not sgd:
                assert not tw.w_derived()       # its rows hold the first set's w: they are read
        b = pre[i] if pre else compiled(i)
        ukeys, wu, loss_c = run.begin(mb)
        if form == "lr":
            capi.lr_step(tw, b, ws)
        else:
            capi.fm_step(tw, tv, b, ws)
        if local:
            g_loss = ws.fetch_loss(b.R)
        else:
            same(b.host()["ukeys"], ukeys, "ukeys")
            g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
            same(g_wu, wu, "step %d wu" % i)
        one_of(g_loss, loss_c, "step %d loss" % i)
        gw_c, ew, ev = run.finish(g_loss)               # the gradient of the GPU's own loss
        if not local:
            one_of(g_gw, gw_c, "step %d gw" % i)
        xw = table_is(tw, ew, "step %d w table" % i)
        xv = table_is(tv, ev, "step %d v table" % i) if tv is not None else None
        run.adopt(xw[:2] if sgd else xw, None if xv is None else (xv[:2] if sgd else xv))
    pctr = capi.lr_predict(tw, b, ws) if form == "lr" else capi.fm_predict(tw, tv, b, ws)
    one_of(pctr, run.predict(mbs[-1]), "pctr")
    print(judge.format(plan.id))
    judge.assert_cap()


@pytest.mark.parametrize("plan", HC.LR_BATCH, ids=HC.ids(HC.LR_BATCH))
def test_valued_lr(plan):
    _run(plan)


@pytest.mark.parametrize("plan", HC.LR_LOCAL, ids=HC.ids(HC.LR_LOCAL))
def test_valued_lr_on_the_local_build(plan):
    _run(plan, local=True)


@pytest.mark.parametrize("plan", HC.FM, ids=HC.ids(HC.FM))
def test_valued_canonical_fm_a_set_per_table(plan):
    _run(plan)


@pytest.mark.parametrize("plan", HC.FFM, ids=HC.ids(HC.FFM))
def test_field_aware_fm_a_set_per_table(plan):
    _run(plan)


@pytest.mark.parametrize("precompiled", [True, False], ids=["compiled_before", "fresh"])
@pytest.mark.parametrize("plan,local", [(p, False) for p in HC.LR_BATCH_CHANGED + HC.FM_CHANGED +
                                        HC.FFM_CHANGED] + [(p, True) for p in HC.LR_LOCAL_CHANGED],
                         ids=lambda v: v.id if isinstance(v, HC.Plan) else "local" if v else "batch")
def test_set_hyper_in_mid_run(plan, local, precompiled):
    _run(plan, local, precompiled)


# ---------------------------------------------------------- 2. the pooled FM step
def _table_same(t, s, what):
    for a, e in zip(t.export(), s):
        same(a, e, what)


@pytest.mark.parametrize("opt,phases,precompiled", [
    ("ftrl", [HC.PAIR["ftrl"]], False), ("sgd", [HC.PAIR["sgd"]], False),
    ("ftrl", [HC.PAIR["ftrl"], HC.PAIR_AFTER["ftrl"]], True),
    ("ftrl", [HC.PAIR["ftrl"], HC.PAIR_AFTER["ftrl"]], False),
    ("sgd", [HC.PAIR["sgd"], HC.PAIR_AFTER["sgd"]], True)],
    ids=["ftrl", "sgd", "ftrl_changed_compiled_before", "ftrl_changed_fresh",
         "sgd_changed_compiled_before"])
def test_pooled_fm_step_a_set_per_table(opt, phases, precompiled):
    """fm_mode=reference (k_fm_* of xf_model.hip step TV and TW side by side) against
    O.fm_update in sum_mode(1): both tables bit for bit after every step, then the predictions"""
    raw = HC.pooled_raw()
    want = []
    _, _, pctr = HC.pooled_oracle(raw, opt, phases,
                                  after_step=lambda i, sw, sv: want.append((sw.export(),
                                                                            sv.export())))
    _, _, init = HC.pooled_stores(opt)
    tw = capi.Table(_go(opt), 1, capacity=1 << 16, **phases[0][0].kw())
    tv = capi.Table(_go(opt), HC.POOLED_K, init[0], init[1], seed=99, capacity=1 << 16,
                    **phases[0][1].kw())
    _derived_as_it_should(tw, phases[0][0])
    ws = capi.Workspace()
    pre = [capi.Batch(*x) for x in raw] if precompiled else None
    for i, x in enumerate(raw):
        if i == HC.SWITCH and len(phases) > 1:
            phases[1][0].to_table(tw)
            phases[1][1].to_table(tv)
        b = pre[i] if pre else capi.Batch(*x)
        capi.fm_step(tw, tv, b, ws)
        _table_same(tw, want[i][0], "step %d w table" % i)
        _table_same(tv, want[i][1], "step %d v table" % i)
    same(capi.fm_predict(tw, tv, b, ws), pctr, "pctr")


@pytest.mark.parametrize("model", ["lr", "fm"])
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_keyed_steps_with_giant_heavy_keys(opt, model):
    """the keyed (capi.Batch) binary path on power-law heads: the tiled gradient + Push kernels of
    xf_model.hip, the chunked heavy keys' finish and the listed updates, LR under the weight
    table's set and the pooled FM (k = 16) under a set per table, against the exact-sum oracle"""
    raw = HC.giant_raw()
    hw, hv = HC.GIANT_PAIR[opt]
    o, go = (O.OPT_FTRL, capi.OPT_FTRL) if opt == "ftrl" else (O.OPT_SGD, capi.OPT_SGD)
    b, ob = capi.Batch(*raw, on_gpu=True), O.Batch(*raw)
    hc = b.heavy_chunks()
    assert b.H >= 3 and hc[-1] >= 8 and np.diff(hc).max() >= 6
    ws = capi.Workspace()
    tw, sw = capi.Table(go, 1, capacity=1 << 14, **hw.kw()), O.Store(o, 1)
    hw.to_store(sw)
    tv = sv = None
    if model == "fm":
        tv = capi.Table(go, HC.GIANT_K, capi.INIT_HASHNORM, seed=3, capacity=1 << 14, **hv.kw())
        sv = O.Store(o, HC.GIANT_K, O.INIT_HASHNORM, 0.0, 3)
        hv.to_store(sv)
    for _ in range(HC.GIANT_STEPS):
        with O.sum_mode(1):
            if model == "lr":
                capi.lr_step(tw, b, ws)
                O.lr_update(sw, ob)
            else:
                capi.fm_step(tw, tv, b, ws)
                O.fm_update(sw, sv, ob)
    _table_same(tw, sw.export(), "w table")
    if tv is not None:
        _table_same(tv, sv.export(), "v table")


@pytest.mark.parametrize("dim,init,c", [(1, capi.INIT_ZERO, 0.0), (10, capi.INIT_CONST, 0.001)])
def test_sgd_push_with_another_learning_rate(dim, init, c):
    """the table's own Push (k_update) under SGD with lr 0.2, then 0.05 through set_hyper"""
    rng = np.random.RandomState(1)
    keys = np.sort(np.unique(rng.randint(1, 2**62, size=800).astype(np.uint64)))
    t = capi.Table(capi.OPT_SGD, dim, init, c, capacity=4096, **HC.SGD_HI.kw())
    s = O.Store(O.OPT_SGD, dim, init, c)
    HC.SGD_HI.to_store(s)
    for i in range(4):
        if i == 2:
            HC.SGD_LO.to_table(t)
            HC.SGD_LO.to_store(s)
        g = rng.randn(len(keys) * dim).astype(np.float32)
        t.push(keys, g)
        s.push(keys, g)
    _table_same(t, s.export(), "table")
    d = O.Store(O.OPT_SGD, dim, init, c)
    d.push(keys, g)
    assert not np.array_equal(d.export()[1], s.export()[1])


@pytest.mark.parametrize("hyper,dim", [(HC.NO_L1, 1), (HC.SPARSE, 4), (HC.SGD_HI, 4)],
                         ids=lambda v: repr(v))
def test_merged_push_of_several_sources(hyper, dim):
    """xf_table_update_merged_dev (k_update_merged): three sources' key lists with shared keys,
    every key's steps one after the other in rank order — the oracle's three pushes"""
    import ctypes as C
    import torch
    rng = np.random.RandomState(8)
    base = np.array([O.hash_str(str(i)) for i in range(3000)], dtype=np.uint64)
    lists = [np.sort(rng.choice(base, size=1800, replace=False)) for _ in range(3)]
    allk = np.concatenate(lists)
    n = len(allk)
    o, go = (O.OPT_FTRL, capi.OPT_FTRL) if hyper.opt == "ftrl" else (O.OPT_SGD, capi.OPT_SGD)
    init = (capi.INIT_ZERO, O.INIT_ZERO) if dim == 1 else (capi.INIT_HASHNORM, O.INIT_HASHNORM)
    t = capi.Table(go, dim, init[0], 0.0, seed=5, capacity=1 << 13, **hyper.kw())
    s = O.Store(o, dim, init[1], 0.0, 5)
    hyper.to_store(s)
    order = np.argsort(allk, kind="stable").astype(np.uint32)       # a key's sources in rank order
    dk = torch.from_numpy(allk.view(np.int64)).cuda()
    ds = torch.from_numpy(allk[order].view(np.int64)).cuda()
    do = torch.from_numpy(order.view(np.int32)).cuda()
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    t.resolve_dev(dk.data_ptr(), n, rows.data_ptr())
    for ks in lists:
        s.pull(ks)
    for _ in range(3):
        g = (rng.randn(n, dim) * 10.0 ** rng.uniform(-5, 0, (n, 1))).astype(np.float32)
        dg = torch.from_numpy(g).cuda()
        capi.check(capi.lib().xf_table_update_merged_dev(
            t.h, C.c_void_p(ds.data_ptr()), C.c_void_p(do.data_ptr()), n,
            C.c_void_p(rows.data_ptr()), C.c_void_p(dg.data_ptr()), None))
        t.check()
        at = 0
        for ks in lists:
            s.push(ks, g[at:at + len(ks)])
            at += len(ks)
    _table_same(t, s.export(), "table")


# ---------------------------------------------------------- 3. binary LR on cells
@pytest.fixture(scope="module")
def cells():
    """the stream, and the oracle's table per set: formed once, shared by the kernel variants"""
    raw = HC.cells_raw()
    known = {}

    def table(*phases, **kw):
        """(unsplit=True: of HC.cells_raw_unsplit(), the stream that reaches k_lr_grad_dense)"""
        key = phases + (kw.get("unsplit", False),)
        if key not in known:
            known[key] = HC.cells_oracle(unsplit() if key[-1] else raw, list(phases)).export()
        return known[key]

    def unsplit():
        if "raw" not in known:
            known["raw"] = HC.cells_raw_unsplit()
        return known["raw"]
    table.unsplit = unsplit
    return raw, table


def _cells_steps(raw, phases, path, precompiled=False, split=True):
    t = capi.Table(_go(phases[0].opt), 1, capacity=1 << 19, **phases[0].kw())
    _derived_as_it_should(t, phases[0])
    ws = capi.Workspace()
    capi.tune(*path)
    try:
        pre = [capi.LocalBatch(t, *x) for x in raw] if precompiled else None
        for i in range(HC.CELLS_STEPS):
            if i == HC.SWITCH and len(phases) > 1:
                phases[1].to_table(t)
                assert not t.w_derived()
            b = pre[i % len(raw)] if pre else capi.LocalBatch(t, *raw[i % len(raw)],
                                                              retain_keys=False)
            if i == 1 or not split:
                assert (b.cells_info()["nsplit_chunks"] > 0) == split
                assert b.cells_info()["nwin"] == 3
            capi.lr_step(t, b, ws)
            t.check()
            del b
            if i == 1:
                t.defrag()      # holes and an arrival segment; a kept minibatch follows its keys
    finally:
        capi.tune(path[0], 0)
    return t


@pytest.mark.parametrize("path", HC.CELLS_PATHS, ids=lambda p: "%s%d" % p)
@pytest.mark.parametrize("hyper", HC.CELLS_SETS, ids=repr)
def test_every_variant_of_the_gradient_kernel_under_every_set(cells, hyper, path):
    """tests/test_gpu_cells.py's three-window power-law shape (split chunks, a defrag after step
    1), four steps: the table bit for bit the exact-sum oracle's under NO_L1, SPARSE, NEG_L1 (the
    kernels may not derive w: a fresh row's w is not ftrl_w_of(0, 0) there) and SGD lr 0.2.
    Every minibatch of that stream has split chunks, so all four knobs run k_lr_grad_cells and the
    finish kernel on it (and k_lr_grad_dense on the two small arrival segments only); the same
    steps over HC.cells_raw_unsplit() (three windows, no chunk split) run what the knob names — k_lr_grad_dense with byte-masked (lr_gradient = 2) or
    whole-line stores (3, and old_weight = 2 by the shape), the general kernel alone (1) — read
    from the launch counters."""
    raw, table = cells
    n0 = capi.lr_grad_launches()
    t = _cells_steps(raw, [hyper], path)
    _table_same(t, table(hyper), "table")
    n1 = capi.lr_grad_launches()
    t = _cells_steps(table.unsplit(), [hyper], path, split=False)
    _table_same(t, table(hyper, unsplit=True), "table of the unsplit stream")
    n2 = capi.lr_grad_launches()
    d1, d2 = ({k: b[k] - a[k] for k in a} for a, b in ((n0, n1), (n1, n2)))
    print(hyper, path, d1, d2)
    # the split stream: four steps, the general kernel and the finish kernel once each over the
    # rows the table held; steps 1 and 2 bring new keys, and their arrival segments (a few chunks,
    # none split) run dense — or the general kernel again under lr_gradient = 1
    forced = path == ("lr_gradient", 1)
    assert (d1["cells"], d1["split_finish"]) == (6 if forced else 4, 4), d1
    assert d1["dense_masked"] + d1["dense_full"] == (0 if forced else 2), d1
    # the unsplit stream: four steps and the arrival segment of step 1, five launches of the kernel
    # the knob names
    want = {("lr_gradient", 1): "cells", ("lr_gradient", 2): "dense_masked"}.get(path, "dense_full")
    assert d2["split_finish"] == 0, d2
    if path[0] == "lr_gradient":
        assert all(d2[k] == (5 if k == want else 0)
                   for k in ("dense_masked", "dense_full", "cells")), d2
    else:
        assert (d2["dense_masked"], d2["dense_full"], d2["cells"]) == (0, 5, 0), d2
        derives = hyper.opt == "ftrl" and hyper.lambda1 >= 0      # (the table vouches for w)
        assert d2["dense_derived"] == (5 if derives else 0), d2


@pytest.mark.parametrize("hyper", [HC.A, HC.NO_L1], ids=repr)
def test_import_vouches_for_w_under_the_tables_own_set(hyper):
    """xf_table_import's check (k_check_w_of_nz) on a fresh table created under another set: a
    model the oracle made under THAT set keeps w_derived() true, one made under the defaults turns
    it false (its w is not ftrl_w_of(n, z) under this table's values) — and the cells steps that
    follow equal the oracle's either way, deriving w in the first case and reading it in the
    second.  On HC.old_weight_raw() (split chunks: k_lr_grad_cells and the finish kernel) and on
    HC.old_weight_raw_unsplit() (none: k_lr_grad_dense), by the launch counters."""
    for raw, split in ((HC.old_weight_raw(), True), (HC.old_weight_raw_unsplit(), False)):
        n0 = capi.lr_grad_launches()
        _import_vouches(hyper, raw)
        n1 = capi.lr_grad_launches()
        d = {k: n1[k] - n0[k] for k in n0}
        print(hyper, "split" if split else "unsplit", d)
        # two models, two steps each on a table that holds every key: one segment a step
        dense = d["dense_masked"] + d["dense_full"]
        assert (d["cells"], d["split_finish"], dense) == ((4, 4, 0) if split else (0, 0, 4)), d


def _import_vouches(hyper, raw):
    obs = [O.Batch(*x) for x in raw]
    ws = capi.Workspace()
    for made_under, derived in ((hyper, True), (HC.FTRL_DEFAULT, False)):
        m = O.Store(O.OPT_FTRL, 1)
        made_under.to_store(m)
        for ob in obs:
            with O.sum_mode(1):
                O.lr_update(m, ob)
        k, w, n, z = m.export()
        assert np.count_nonzero(w) > 1000
        t, s = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 18, **hyper.kw()), O.Store(O.OPT_FTRL, 1)
        hyper.to_store(s)
        assert t.w_derived()
        t.import_(k, w, n, z)
        s.import_(k, w, n, z)
        assert t.w_derived() == derived, made_under
        t.defrag()
        for i in range(2):
            b = capi.LocalBatch(t, *raw[i], retain_keys=False)
            with O.sum_mode(1):
                O.lr_update(s, obs[i])
            capi.lr_step(t, b, ws)
            del b
        _table_same(t, s.export(), "table after a model made under %r" % made_under)


@pytest.mark.parametrize("precompiled", [True, False], ids=["compiled_before", "fresh"])
def test_cells_set_hyper_in_mid_run(cells, precompiled):
    raw, table = cells
    phases = [HC.SPARSE, HC.NO_L1]
    t = _cells_steps(raw, phases, ("lr_gradient", 0), precompiled)
    _table_same(t, table(*phases), "table")


# ---------------------------------------------------------- 4. div_by_const on the device
D_INEXACT = 50000.0


@pytest.fixture(scope="module")
def div_inputs():
    """every x at which the bare product with 1 / 50000 is not x / 50000 (the host finds them:
    1308), the 2^16 values around |q| = 2^-125 — the guard's threshold — on both sides and of
    both signs, +-0, the smallest subnormal, the largest finite x"""
    bad = inexact_list(D_INEXACT)
    assert len(bad) == 1308
    edge = np.float32(2.0 ** -125) * np.float32(D_INEXACT)          # x whose quotient is 2^-125
    around = edge.view(np.uint32) + np.arange(-(1 << 14), 1 << 14, dtype=np.int64)
    around = around.astype(np.uint32)
    around = np.concatenate([around, around | np.uint32(0x80000000)])
    assert around.size == 1 << 16
    ends = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF],
                    np.uint32)
    x = np.concatenate([bad, around, ends]).view(np.float32)
    with np.errstate(under="ignore"):
        q = x / np.float32(D_INEXACT)
    below = np.abs(q[1308:1308 + (1 << 16)]) < np.float32(2.0 ** -125)
    assert below.any() and (~below).any()                            # both sides of the guard
    return x, q


def test_div_by_const_guarded_is_the_quotient(div_inputs):
    x, q = div_inputs
    same(capi.div_by_const_probe(x, D_INEXACT, exact=False), q, "x / 50000, guarded")


def test_div_by_const_unguarded_differs_exactly_where_the_host_says(div_inputs):
    """... so the guarded branch is what makes the test above pass"""
    x, q = div_inputs
    got = capi.div_by_const_probe(x, D_INEXACT, exact=True)
    differ = np.flatnonzero(got.view(np.uint32) != q.view(np.uint32))
    assert np.array_equal(differ, np.arange(1308)), (differ.size, differ[:8])


def test_the_tables_verdict_on_alpha():
    for alpha in (0.05, 0.1):
        assert capi.Table(capi.OPT_FTRL, 1, capacity=1024, alpha=alpha).div_exact(), alpha
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1024, alpha=D_INEXACT)
    assert not t.div_exact()
    assert not capi.Table(capi.OPT_SGD, 1, capacity=1024).div_exact()    # no alpha to vouch for
    s = O.Store(O.OPT_FTRL, 1)
    s.set_ftrl(D_INEXACT, 1.0, 5e-5, 10.0)
    keys = np.sort(np.arange(1, 201, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    rng = np.random.RandomState(4)
    for _ in range(3):
        g = (rng.randn(len(keys)) * 10.0 ** rng.uniform(-6, 1, len(keys))).astype(np.float32)
        t.push(keys, g)
        s.push(keys, g)
    _table_same(t, s.export(), "push under alpha = 50000")
    t.set_hyper(0.05, 1.0, 5e-5, 10.0)
    assert t.div_exact()
