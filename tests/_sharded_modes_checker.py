"""Canonical FM, field-aware FM and feature values on several ranks, restated in numpy: the
checker of tests/test_sharded_modes_cpu.py and tests/test_gpu_sharded_modes.py.

No arithmetic of its own.  A rank's gradient comes from the one-rank checkers' pieces —
tests/_fmc_checker.py (pull / forward / gradient), tests/_valued_checker.py (forward_lr /
forward_fm / gradient_w / gradient_fm), tests/_ffm_checker.py (forward / gradient / push_touched)
— over ONE pair of O.Store: the ranks share the tables.  What is new is the order of the Pulls
and Pushes of N workers, the one xf_sharded.hip states:
  * per step, every rank pulls first; then the N pushes are applied in rank order
      sequential   at once
      stale1       after the NEXT step's pulls (the last step's after the loop)
  * every rank's gradient is scaled by its own 1 / R
  * field-aware: a rank's push steps coordinate (u, h) of v only if THAT rank's minibatch touched
    it (push_touched per rank); w is stepped for every key the rank pushed
  * the held-out minibatch of every rank is predicted at the end.
Every family of sums is formed in both orders and left in `audit`, as those checkers do.  A binary
canonical rank is computed by _fmc_checker (which keeps no audit) AND by _valued_checker with every
x = 1, which audits the same sums; the two must agree bit for bit.

A minibatch is (rowptr, keys, fgid, values, labels); fgid is None outside field-aware FM, a
binary trainer ignores the values.  A rank without rows holds a minibatch of zero rows."""
import numpy as np

from oracle import pyoracle as O
from tests import _ffm_checker as FF
from tests import _fmc_checker as FC
from tests import _valued_cases as Cs
from tests import _valued_checker as V
from xflow_amd import capi

MODES = ("canonical", "lr", "field_aware")
STEPS = Cs.STEPS
EMPTY = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), None, np.zeros(0, np.float32),
         np.zeros(0, np.int32))


# ---------------------------------------------------------------- streams
PROBE = np.array([capi.hash_str("probe-a"), capi.hash_str("probe-b")], np.uint64)


def rank_seed(rank):
    """the streams' generators take seed + step: ten apart, no two (rank, step) share one"""
    return 100 + 10 * rank


def rank_stream(mode, case, rank, F=0):
    """-> (the rank's STEPS training minibatches, its held-out minibatch)"""
    seeds = (rank_seed(rank), rank_seed(rank) + 5)
    if mode == "field_aware":
        train, held = (FF.stream(case, F, seed=s) for s in seeds)
        if case == "ragged":
            train = [_probe_row(m, rank, F) for m in train]
        return list(train), held[0]
    train, held = (Cs.stream(case, seed=s) for s in seeds)
    five = lambda m: (m[0], m[1], None, m[2], m[3])  # noqa: E731
    return [five(m) for m in train], five(held[0])


def _probe_row(mb, rank, F):
    """`ragged` holds 1500 keys about 24 times each in rows of about 20: with few fields every
    (key, field) is touched by some rank, and the masked push would never meet a coordinate that
    must keep its bits.  So the first row of exactly two nonzeros (after row 1) is re-keyed to two
    keys outside the key table, under fields that depend on the rank: each of the two is pushed
    by every rank in every step with ONE touched field — the other's — and the ranks' masks
    differ.  Rows, nonzeros, values and labels stay as they are."""
    rowptr, keys, fg, vals, labels = mb
    lens = np.diff(rowptr.astype(np.int64))
    r = 2 + int(np.flatnonzero(lens[2:] == 2)[0])
    a = int(rowptr[r])
    keys, fg = keys.copy(), fg.copy()
    keys[a:a + 2] = PROBE
    fg[a:a + 2] = (rank % F, (rank + 1) % F)
    return rowptr, keys, fg, vals, labels


def streams(mode, case, world, F=0, empty_ranks=()):
    """-> per rank (training minibatches, held-out minibatch); a rank of empty_ranks holds
    zero-row minibatches throughout"""
    out = []
    for r in range(world):
        if r in empty_ranks:
            e = EMPTY if mode != "field_aware" else \
                (EMPTY[0], EMPTY[1], np.zeros(0, np.int32), EMPTY[3], EMPTY[4])
            out.append(([e] * STEPS, e))
        else:
            out.append(rank_stream(mode, case, r, F))
    return out


def all_keys(strs):
    return np.unique(np.concatenate([m[1] for train, held in strs for m in train + [held]]))


def owner_of(keys, world):
    """the rank that owns each key: the oracle's xo_shard_of, the one definition the tests use"""
    return np.array([O.lib().xo_shard_of(int(k), world) for k in keys], np.int64)


def old_tables(mode, opt, k, F, keys):
    """tests/_valued_cases.old_state for `keys`: -> (w state, v state or None), each (keys, w, n, z)"""
    dim = {"canonical": k, "lr": 0, "field_aware": F * k}[mode]
    return Cs.old_state(keys, opt, 1, "w"), (Cs.old_state(keys, opt, dim) if dim else None)


def stores(mode, opt, k, F, strs, seed=7):
    """the oracle's stores — w from zero, v hash-normal for both optimizers — holding the old state
    of every key of every rank's minibatches"""
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    dim = {"canonical": k, "lr": 0, "field_aware": F * k}[mode]
    ws = O.Store(o, 1)
    vs = O.Store(o, dim, O.INIT_HASHNORM, 0.0, seed) if dim else None
    sw, sv = old_tables(mode, opt, k, F, all_keys(strs))
    ws.import_(*sw)
    if vs is not None:
        vs.import_(*sv)
    return ws, vs


# ---------------------------------------------------------------- one rank's share of a step
def _pull(mode, ws, vs, ukeys):
    if mode == "lr":
        return V._f32(ws.pull(ukeys)).reshape(len(ukeys)), None
    return FC.pull(ws, vs, ukeys)


def _same(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _forward(mode, valued, F, rp, uidx, fg, x, labels, wu, vu, audit):
    """-> loss, pctr, what the gradient needs beside them"""
    if mode == "lr":
        loss, pctr = V.forward_lr(rp, uidx, x, labels, wu, audit)
        return loss, pctr, None
    if mode == "field_aware":
        loss, pctr, _, pairs = FF.forward(rp, uidx, fg, x, labels, wu, vu, F, audit)
        return loss, pctr, pairs
    loss, pctr, S = V.forward_fm(rp, uidx, x, labels, wu, vu, audit)
    if not valued:      # the binary form's own checker, and the audited one with x = 1 agree
        loss1, pctr1, S1, _, _ = FC.forward(rp, uidx, labels, wu, vu)
        for a, b, nm in ((loss1, loss, "loss"), (pctr1, pctr, "pctr"), (S1, S, "S")):
            _same(a, b, "binary canonical forward: " + nm)
        loss, pctr, S = loss1, pctr1, S1
    return loss, pctr, S


def _gradient(mode, valued, F, rp, uidx, fg, U, x, loss, aux, vu, audit):
    """-> gw[U], gv[U, dim] or None, touched[U, F] or None"""
    if mode == "lr":
        return V.gradient_w(rp, uidx, U, x, loss, audit)[0], None, None
    if mode == "field_aware":
        return FF.gradient(rp, uidx, fg, U, x, loss, F, aux, audit)
    gw, gv = V.gradient_fm(rp, uidx, U, x, loss, aux, vu, audit)
    if not valued:
        gw1, gv1 = FC.gradient(rp, uidx, U, loss, aux, vu)
        _same(gw1, gw, "binary canonical gradient: gw")
        _same(gv1, gv, "binary canonical gradient: gv")
        gw, gv = gw1, gv1
    return gw, gv, None


def _slice(mode, valued, mb):
    rowptr, keys, fg, vals, labels = mb
    rp, ukeys, uidx, fgs, x = FF._slice(rowptr, keys, fg if mode == "field_aware" else
                                        np.zeros(len(keys), np.int64),
                                        vals if valued else None)
    return rp, ukeys, uidx, fgs, x, labels


def _push(mode, ws, vs, F, ukeys, gw, gv, touched):
    if len(ukeys) == 0:
        return
    ws.push(ukeys, gw)
    if mode == "canonical":
        vs.push(ukeys, gv)
    elif mode == "field_aware":
        FF.push_touched(vs, ukeys, gv, touched, vs.dim // F)


# ---------------------------------------------------------------- the run
def run(mode, opt, k, F, valued, schedule, strs, audit, seed=7, steps=STEPS):
    """`steps` steps of len(strs) ranks on shared stores.
    -> ws, vs, [held-out pctr per rank], log[step][rank] = (ukeys, gw, gv, touched)"""
    assert mode in MODES and schedule in ("sequential", "stale1")
    assert valued or mode != "lr", "binary LR is the reference's: the oracle's own update"
    ws, vs = stores(mode, opt, k, F, strs, seed)
    world = len(strs)
    log, outstanding = [], []
    for s in range(steps):
        cut = [_slice(mode, valued, strs[r][0][s]) for r in range(world)]
        pulled = [_pull(mode, ws, vs, c[1]) if len(c[1]) else (None, None) for c in cut]
        for p in outstanding:               # stale1: step s-1's pushes land after step s's pulls
            _push(mode, ws, vs, F, *p)
        grads = []
        for (rp, ukeys, uidx, fg, x, labels), (wu, vu) in zip(cut, pulled):
            if len(ukeys) == 0:
                grads.append((ukeys, None, None, None))
                continue
            loss, _, aux = _forward(mode, valued, F, rp, uidx, fg, x, labels, wu, vu, audit)
            grads.append((ukeys,) + _gradient(mode, valued, F, rp, uidx, fg, len(ukeys), x, loss,
                                              aux, vu, audit))
        log.append(grads)
        if schedule == "sequential":
            for p in grads:
                _push(mode, ws, vs, F, *p)
            outstanding = []
        else:
            outstanding = grads
    for p in outstanding:
        _push(mode, ws, vs, F, *p)
    pctr = []
    for r in range(world):
        rp, ukeys, uidx, fg, x, labels = _slice(mode, valued, strs[r][1])
        if len(ukeys) == 0:
            pctr.append(FC._sigmoid(np.zeros(len(rp) - 1, np.float32)))
            continue
        wu, vu = _pull(mode, ws, vs, ukeys)
        pctr.append(_forward(mode, valued, F, rp, uidx, fg, x, labels, wu, vu, audit)[1])
    return ws, vs, pctr, log


# ---------------------------------------------------------------- what the streams must hold
def shared_key_steps(log):
    """steps in which some key is pushed by two ranks"""
    out = []
    for s, grads in enumerate(log):
        ks = np.concatenate([g[0] for g in grads])
        if len(np.unique(ks)) < len(ks):
            out.append(s)
    return out


def differing_mask_steps(log):
    """field-aware: steps in which two ranks push one key with different touched masks"""
    out = []
    for s, grads in enumerate(log):
        for a in range(len(grads)):
            for b in range(a + 1, len(grads)):
                (ka, _, _, ta), (kb, _, _, tb) = grads[a], grads[b]
                if len(ka) == 0 or len(kb) == 0:
                    continue
                both, ia, ib = np.intersect1d(ka, kb, return_indices=True)
                if len(both) and np.any(ta[ia] != tb[ib]):
                    out.append(s)
    return sorted(set(out))


def never_touched(log, keys, F):
    """field-aware: bool [len(keys), F], the (key, field) pairs no rank touched in any step"""
    seen = np.zeros((len(keys), F), bool)
    for grads in log:
        for ukeys, _, _, touched in grads:
            if len(ukeys):
                seen[np.searchsorted(keys, ukeys)] |= touched
    return ~seen


# ---------------------------------------------------------------- the tests' cases
# (mode, world, fields, k, optimizer, schedule, stream, valued): what tests/test_gpu_sharded_modes.py
# steps on the GPU; tests/test_sharded_modes_cpu.py shows every sum of the checker exact on them
CASES = (("canonical", 2, 0, 4, "ftrl", "sequential", "ragged", False),
         ("canonical", 3, 0, 7, "sgd", "stale1", "zipf_heavy", False),
         ("canonical", 2, 0, 16, "ftrl", "stale1", "zipf_chunks", True),
         ("canonical", 3, 0, 4, "sgd", "sequential", "ragged", True),
         ("lr", 2, 0, 0, "ftrl", "stale1", "zipf_chunks", True),
         ("lr", 3, 0, 0, "sgd", "sequential", "ragged", True),
         ("field_aware", 2, 3, 4, "ftrl", "sequential", "ragged", True),
         ("field_aware", 3, 18, 4, "ftrl", "stale1", "zipf_heavy", False),
         ("field_aware", 2, 5, 7, "sgd", "sequential", "zipf_chunks", True))
# a group of one on the exchange path against the fused step
GENERAL = (("canonical", 1, 0, 16, "ftrl", "sequential", "zipf_heavy", True),
           ("field_aware", 1, 3, 4, "ftrl", "sequential", "ragged", False))
# a rank without rows: world 2 with rank 1 empty, and the one-rank run it must equal — one case
# per branch of the trainer's gradient selection (canonical, field-aware, valued LR)
EMPTY_RANK = ((("canonical", 2, 0, 4, "ftrl", "sequential", "ragged", True),
               ("canonical", 1, 0, 4, "ftrl", "sequential", "ragged", True)),
              (("field_aware", 2, 3, 4, "ftrl", "sequential", "ragged", False),
               ("field_aware", 1, 3, 4, "ftrl", "sequential", "ragged", False)),
              (("lr", 2, 0, 0, "sgd", "stale1", "ragged", True),
               ("lr", 1, 0, 0, "sgd", "stale1", "ragged", True)))
_RUNS = {}


def case_id(c):
    return "-".join(str(x) for x in c)


def run_case(c, empty_ranks=()):
    """the checker over one case, computed once per session and left unchanged:
    -> (ws, vs, pctr per rank, log, streams, audit)"""
    key = (c, tuple(empty_ranks))
    if key not in _RUNS:
        mode, world, F, k, opt, schedule, case, valued = c
        strs = streams(mode, case, world, F, empty_ranks)
        audit = []
        ws, vs, pctr, log = run(mode, opt, k, F, valued, schedule, strs, audit)
        _RUNS[key] = (ws, vs, pctr, log, strs, audit)
    return _RUNS[key]
