"""Table eviction restated in numpy (xf_table_evict): a row is dropped iff w == 0 (either sign of
zero) and n < x, in float32; a NaN n compares false and is kept.  Applied to an export (keys
ascending, w, n, z), so the survivors keep their order.  Also the crafted tables and the training
stream that tests/test_gpu_evict.py and tests/test_evict_cpu.py share."""
import numpy as np

from tests._hyper_cases import synth

SPARE = np.uint64(2**64 - 1)      # the reserved key value: judged like any other


def keep_mask(w, n, x):
    w, n = np.asarray(w, np.float32), np.asarray(n, np.float32)
    with np.errstate(invalid="ignore"):
        return ~((w == np.float32(0)) & (n < np.float32(x)))


def evict(state, x):
    """state = (keys, w, n, z) of an export -> (the survivors' state, rows seen, rows dropped);
    x == 0 does nothing and judges nothing"""
    keys, w, n, z = state
    if float(x) == 0.0:
        return state, 0, 0
    keep = keep_mask(w, n, x)
    return tuple(a[keep] for a in state), len(keys), int((~keep).sum())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_state(got, want, what=""):
    for name, g, r in zip(("keys", "w", "n", "z"), got, want):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.shape, r.shape)
        assert np.array_equal(bits(g), bits(r)), (what, name)


# ------------------------------------------------------------------ crafted tables
X = 1.0       # the threshold of the crafted tables: dropped rows hold n = 0.5, kept zero rows 2.0
PATTERNS = ("none", "all", "every_other", "first", "last", "blocks", "one_per_wave",
            "one_per_block_last", "random_half")


def sizes(B, S):
    """the row counts: around a wavefront, around a block, several blocks, and more blocks than
    the scan has threads (257 blocks + 1 row)"""
    return [1, S - 1, S, S + 1, B - 1, B, B + 1, 2 * B + 1, 5 * B + 37, 257 * B + 1]


def drop_pattern(name, n, B, S):
    """which of the n rows (rank order == key order) go"""
    r = np.arange(n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "every_other":
        return r % 2 == 0
    if name == "first":
        return r == 0
    if name == "last":
        return r == n - 1
    if name == "blocks":                       # whole blocks dropped between kept ones
        return (r // B) % 2 == 1
    if name == "one_per_wave":                 # the survivor's lane moves from wave to wave
        return r % S != ((r // S) * 7 + 3) % S
    if name == "one_per_block_last":           # (a ragged last block keeps nothing)
        return r % B != B - 1
    if name == "random_half":
        return np.random.default_rng(n).random(n) < 0.5
    raise KeyError(name)


def crafted(n, drop, seed=1):
    """(keys ascending, w, n, z) of n rows of which drop[r] go at x = X.  Dropped rows: w = +0 or
    -0, n = 0.5, z anything; kept rows: a nonzero w, or w = 0 with n = 2."""
    rng = np.random.default_rng(seed + n)
    keys = np.unique(rng.integers(1, 2**63, size=n + n // 8 + 16, dtype=np.uint64))[:n]
    assert len(keys) == n
    w = rng.normal(0, 1, n).astype(np.float32)
    w[w == 0] = 1.0
    nn = rng.random(n).astype(np.float32) * 4
    z = rng.normal(0, 1, n).astype(np.float32)
    kept_zero = ~drop & (rng.random(n) < 0.5)
    w[kept_zero] = 0.0
    nn[kept_zero] = 2.0
    w[drop] = np.where(rng.random(int(drop.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    nn[drop] = 0.5
    return keys, w, nn, z


# ------------------------------------------------------------------ the training stream
# lambda1 of the training tests: the oracle's CPU run of T1 steps of stream() leaves 59.5 % of the
# 4783 keys at w == 0 (tests/test_evict_cpu.py asserts 10 % .. 90 %); at the default 5e-5 .. 8e-4
# it is 19.8 % (a minibatch of 600 rows: one occurrence moves z by ~8e-4)
L1 = 1.6e-3
HYPER = dict(alpha=0.05, beta=1.0, lambda1=L1, lambda2=10.0)
T1, T2 = 3, 2
X_TRAIN = 5e-6        # a finite threshold inside the zero rows' n (0 .. 2.4e-5)
# The replay stream (replay_stream(): the T1 minibatches replayed for EPOCHS = 4 epochs, 4737
# keys), the oracle's CPU run, share of rows dropped at each eviction (tests/test_evict_cpu.py
# asserts 10 % .. 90 %):
#   HYPER, x = inf:      every boundary 61.7 %, 61.7 %, 61.7 %; every second boundary 20.7 %
#   HYPER, x = X_TRAIN:  every boundary 59.8 %, 59.8 %, 59.8 %; every second boundary 18.9 %
#   HYPER_ALL_ZERO, x = inf: 100 % at every eviction
# The reserved key is kept under HYPER (its labels follow it) and dropped under HYPER_ALL_ZERO.
#
# lambda1 of the worker tests on the three-block zipf text (worker_text(): 466 keys with key 0;
# a row of a 1 MiB block moves z by ~1.4e-5): 8e-5 leaves the rare fids at w == 0.  Shares dropped
# at the evictions, epochs / evict_every 4/1, 4/2, 3/2:
#   x = inf:       29.0 28.8 28.8 28.8 % | 24.5 23.7 % | 24.5 24.3 %
#   x = X_WORKER:  26.2 25.8 25.8 25.8 % | 23.4 22.8 % | 23.4 23.2 %
#   feature values on, 4/1, inf: 24.2 24.1 24.1 24.1 %;  two ranks, 3/1, inf: 39.8 39.7 39.7 %
# (at 2e-5 and below 1 % go; X_WORKER = 2e-9 takes 0.9 % when n has two epochs to grow)
L1_WORKER = 8e-5
X_WORKER = 3e-9       # inside the zero rows' n (0 .. 6.8e-9 after one epoch, most at 1.4e-9)


def stream():
    """T1 + T2 training minibatches and a held one (the suite's exact-sum inputs)"""
    rng = np.random.RandomState(41)
    return [synth(rng, 600, 12, 5000, 1.2 if i % 2 else None, True) for i in range(T1 + T2 + 1)]


def oracle_after_t1():
    from oracle import pyoracle as O
    s = O.Store(O.OPT_FTRL, 1)
    s.set_ftrl(HYPER["alpha"], HYPER["beta"], HYPER["lambda1"], HYPER["lambda2"])
    for raw in stream()[:T1]:
        with O.sum_mode(1):
            O.lr_update(s, O.Batch(*raw))
    return s.export()


# ------------------------------------------------------------------ the evicting oracle
# Every weight stays 0 under this lambda1 (|z| never reaches it): every eviction at x = inf empties
# the table, and every replayed minibatch meets a created table again
HYPER_ALL_ZERO = dict(HYPER, lambda1=1e3)
EPOCHS = 4
# drops only rows whose n is 0.  After ONE epoch of the replay stream 126 keys hold n == 0 (every
# prediction of the first step is 0.5, so a key's losses can cancel exactly); after two epochs
# none does: the eviction that drops nothing runs at the boundaries in AT_NONE
X_NONE = 1e-30
AT_NONE = [1, 2]


class EvictingStore:
    """O.Store(O.OPT_FTRL, 1) under `hyper`, with xf_table_evict restated on it: export, the
    evict() filter above, a fresh Store (same hyper-parameters), import.  Steps are the oracle's
    O.lr_update in sum_mode(1), valued steps tests/_valued_checker.py's."""

    def __init__(self, hyper=None):
        self.hyper = dict(HYPER if hyper is None else hyper)
        self.s = self._fresh()
        self.audit = []           # the valued restatement's sums (V.assert_exact)

    def _fresh(self):
        from oracle import pyoracle as O
        s = O.Store(O.OPT_FTRL, 1)
        h = self.hyper
        s.set_ftrl(h["alpha"], h["beta"], h["lambda1"], h["lambda2"])
        return s

    def step(self, raw, values=None):
        from oracle import pyoracle as O
        if values is not None:
            from tests import _valued_checker as V
            V.lr_step(self.s, raw[0], raw[1], values, raw[2], self.audit)
            return
        with O.sum_mode(1):
            O.lr_update(self.s, O.Batch(*raw))

    def predict(self, raw, values=None):
        """the forward (a Pull inserts the unseen keys, as the GPU's does)"""
        from oracle import pyoracle as O
        if values is not None:
            from tests import _valued_checker as V
            return V.lr_predict(self.s, raw[0], raw[1], values, raw[2], self.audit)
        ob = O.Batch(*raw)
        with O.sum_mode(1):
            return ob.lr_loss(self.s.pull(ob.ukeys))[1]

    def evict(self, x):
        """-> (seen, dropped)"""
        want, seen, dropped = evict(self.s.export(), x)
        if dropped:
            self.s = self._fresh()
            self.s.import_(*want)
        return seen, dropped

    def export(self):
        return self.s.export()


class _Prepared:
    """one rank's minibatch between its Pull and its Push"""

    def __init__(self, raw, values, audit):
        from oracle import pyoracle as O
        self.values, self.audit = values, audit
        if values is None:
            self.ob = O.Batch(*raw)
            self.ukeys = self.ob.ukeys
        else:
            from tests import _valued_checker as V
            self.rp, self.ukeys, self.uidx, self.x = V._slice(raw[0], raw[1], values)
            self.labels = raw[2]

    def grad(self, pulled):
        from oracle import pyoracle as O
        if self.values is None:
            with O.sum_mode(1):
                return self.ob.lr_grad(self.ob.lr_loss(pulled)[0])
        from tests import _valued_checker as V
        wu = np.asarray(pulled, np.float32).reshape(len(self.ukeys))
        loss, _ = V.forward_lr(self.rp, self.uidx, self.x, self.labels, wu, self.audit)
        return V.gradient_w(self.rp, self.uidx, len(self.ukeys), self.x, loss, self.audit)[0]


class Ranks:
    """the pull / push rule of several ranks on one EvictingStore (tests/test_sharded_gloo.py's
    _simulate): sequential — all ranks pull, then push in rank order; stale1 — the previous step's
    pushes land after this step's pulls.  An eviction lands the outstanding pushes first, as
    xf_sharded_evict flushes."""

    def __init__(self, store, schedule):
        assert schedule in ("sequential", "stale1")
        self.store, self.schedule, self.outstanding = store, schedule, None

    def flush(self):
        if self.outstanding is not None:
            for ukeys, g in self.outstanding:
                self.store.s.push(ukeys, g)
            self.outstanding = None

    def step(self, raws, values=None):
        """raws: one minibatch per rank (None: the rank has none this turn)"""
        values = values or [None] * len(raws)
        mbs = [_Prepared(r, v, self.store.audit) for r, v in zip(raws, values) if r is not None]
        mbs = [m for m in mbs if len(m.ukeys)]
        pulled = [self.store.s.pull(m.ukeys) for m in mbs]
        self.flush()
        done = [(m.ukeys, m.grad(p)) for m, p in zip(mbs, pulled)]
        if self.schedule == "stale1":
            self.outstanding = done
        else:
            for ukeys, g in done:
                self.store.s.push(ukeys, g)

    def evict(self, x):
        self.flush()
        return self.store.evict(x)

    def export(self):
        self.flush()
        return self.store.export()


def boundaries(epochs, every, last=False):
    """the epochs (0-based) after which an eviction runs: every `every`-th boundary; last: after
    the final epoch too (the worker's rule)"""
    return [e for e in range(epochs)
            if ((e + 1) % every == 0 and e + 1 < epochs) or (last and e + 1 == epochs)]


def replay_stream(seed=43):
    """T1 training minibatches of stream()'s shape, replayed epoch after epoch.  The reserved key
    2^64 - 1 stands in about half the rows of every minibatch and the labels follow it (nine in
    ten), so that it earns a weight under HYPER; key 0 stands in a few rows."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(T1):
        rowptr, keys, labels = synth(rng, 600, 12, 5000, 1.2 if i % 2 else None, True)
        keys, labels = keys.copy(), labels.copy()
        first = rowptr[:-1].astype(np.int64)
        full = np.flatnonzero(np.diff(rowptr.astype(np.int64)) > 0)
        with_spare = full[rng.rand(len(full)) < 0.5]
        keys[first[with_spare]] = SPARE
        has = np.zeros(len(labels), bool)
        has[with_spare] = True
        labels[:] = np.where(rng.rand(len(labels)) < 0.9, has, ~has).astype(np.int32)
        with_zero = np.setdiff1d(full, with_spare)[:5]
        keys[first[with_zero]] = 0
        out.append((rowptr, keys, labels))
    return out


def replay_values(raw):
    """a value per nonzero from {0.5, 1, 2} (products and sums stay exact)"""
    rng = np.random.default_rng(len(raw[1]))
    return rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=len(raw[1]))


def replay_run(hyper, x, every, epochs=EPOCHS, valued=False, schedule=None, stream=None,
               last=False, at=None):
    """the evicting oracle over `epochs` epochs of the replay stream.  Evictions: at every
    `every`-th boundary (last: after the final epoch too), none with every = 0; `at` names the
    epochs (0-based) after which to evict instead.  schedule: None (one table, step after step)
    or the one-rank exchange rule.
    -> ([(kind, epoch, state, counts)], the store): ("epoch", e, export, None) after every epoch
    and ("evict", e, export, (seen, dropped)) after every eviction"""
    raws = replay_stream() if stream is None else stream
    vals = [replay_values(r) for r in raws] if valued else [None] * len(raws)
    st = EvictingStore(hyper)
    rk = Ranks(st, schedule) if schedule else None
    if at is None:
        at = boundaries(epochs, every, last) if every else []
    out = []
    for e in range(epochs):
        for raw, v in zip(raws, vals):
            if rk:
                rk.step([raw], [v])
            else:
                st.step(raw, v)
        if rk:
            rk.flush()     # (an export flushes: the state the GPU shows after the epoch)
        out.append(("epoch", e, st.export(), None))
        if e in at:
            counts = rk.evict(x) if rk else st.evict(x)
            out.append(("evict", e, st.export(), counts))
    if valued:
        from tests import _valued_checker as V
        V.assert_exact(st.audit)
    return out, st


# ------------------------------------------------------------------ the worker
def worker_text(tmp, two=False):
    """the worker tests' files under `tmp`: a zipf text of just over 2 MiB (three 1 MiB blocks; two:
    a second rank's of just over 1 MiB) and a test file"""
    from tests._zipf_text import zipf_text
    import os
    texts = [zipf_text(27, (2 << 20) + (200 << 10))]
    assert 2 << 20 < len(texts[0]) < 3 << 20
    if two:
        texts.append(zipf_text(26, (1 << 20) + (200 << 10)))
    for r, text in enumerate(texts):
        with open(os.path.join(str(tmp), "train-%05d" % r), "wb") as f:
            f.write(text)
    with open(os.path.join(str(tmp), "test-00000"), "wb") as f:
        f.write(zipf_text(22, 60 << 10, 0.3))
    return str(tmp)


def worker_reference(d, epochs, every, x, lambda1=None, schedule="sequential", valued=False,
                     ranks=1, cache=True):
    """the evicting oracle doing what the worker does: the key-0 init push, then per epoch one
    turn per 1 MiB block (a turn: one block of every rank that still has one, under the
    schedule's rule), the flush at the end of the epoch, an eviction at every `every`-th boundary
    and after the last epoch (every = 0: never), then the forward over the test file.
    The worker checks the trainer (xf_sharded_check, which flushes) after the step of every block
    it has just compiled — xf_worker.cc did so before eviction existed, see DESIGN.md "Replay
    across evictions" — so under stale1 only the epochs that replay cache_ leave a Push
    outstanding: the first epoch, and every epoch with cache_batches=0 (cache=False), lands its
    Pushes after each turn.
    -> dict: model (the state after the last eviction: what is saved), log [(epoch, seen,
    dropped)], rows (trained), labels, pctr and metrics (of the test file), blocks (per rank),
    states (the export after every epoch, before its eviction), store (after the forward)"""
    import os
    from oracle import pyoracle as O
    from xflow_amd import capi
    st = EvictingStore(dict(HYPER, lambda1=L1_WORKER if lambda1 is None else lambda1))
    st.s.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))
    blocks = [list(capi.read_blocks(os.path.join(d, "train-%05d" % r), 1 << 20, values=valued))
              for r in range(ranks)]
    rk = Ranks(st, schedule)
    log, rows, states = [], 0, []
    for e in range(epochs):
        for t in range(max(len(b) for b in blocks)):
            mine = [b[t] if t < len(b) else None for b in blocks]
            rk.step([None if m is None else (m[0], m[1], m[3]) for m in mine],
                    [m[4] if valued and m is not None else None for m in mine])
            rows += sum(len(m[3]) for m in mine if m is not None)
            if e == 0 or not cache:
                rk.flush()
        rk.flush()
        states.append(st.export())
        if every and ((e + 1) % every == 0 or e + 1 == epochs):
            log.append((e + 1,) + st.evict(x))
    model = st.export()
    labs, ps = [], []
    for blk in capi.read_blocks(os.path.join(d, "test-00000"), 4 << 20, values=valued):
        ps.append(st.predict((blk[0], blk[1], blk[3]), blk[4] if valued else None))
        labs.append(blk[3])
    if valued:
        from tests import _valued_checker as V
        V.assert_exact(st.audit)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    return dict(model=model, log=log, rows=rows, labels=lab, pctr=p, metrics=O.auc_logloss(lab, p),
                blocks=[len(b) for b in blocks], states=states, store=st)
