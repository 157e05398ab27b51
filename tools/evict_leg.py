#!/usr/bin/env python3
"""Table eviction measured on a GPU box (profiles/evict/README.md holds the table).

    python tools/evict_leg.py OUT.jsonl [--keys 10000000,100000000] [--skip-push]

Records "evict": an FTRL table of N keys (settled: key r owns row r), of which a random share f
— 0.1 %, 50 %, 99 % — holds w = 0, n = 0.5; xf_table_evict(1.0) drops exactly those.  Warm: one
whole cycle (import, defrag, evict) runs first, so the second state buffer, the tiers and the
scratch arena exist; then `runs` times: the same state imported again (the dropped keys come back
through the arrival index), defrag, and ONE evict between two device events on the null stream
(the call's own stream) and two host clocks.  The call waits for the device three times (the count,
the survivors' count, the swap), so the two clocks agree; every run is listed.
bytes: mark 12.125 per row; compact 0.125 per row + 40 per survivor; directories 8 read + ~8
written per survivor; the zeroed tail 24 per dropped row (12 in each buffer).
Record "defrag": the nearest existing operation on the same build — the same table with 5 % of its
keys in the arrival index, xf_table_defrag timed the same way.
Record "push": the LR gradient + Push kernel (the workspace's `gradient` events) on a minibatch of
BASELINE configs[1]'s shape (50 000 rows x 200 nonzeros over 1e7 keys) against a table that holds
the minibatch's U keys and as many dead ones (pulled, never stepped: w = n = z = 0) spread among
them by the hash — before and after xf_table_evict(1e-30) drops the dead half.
Record "copy": bench.py's stream_copy_gbs(), the measured streaming peak the fractions refer to."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xflow_amd import capi  # noqa: E402

X = 1.0


def _timed(fn):
    """fn() between two device events on the null stream and two host clocks -> (ms, ms, result)"""
    import torch
    L = capi.lib()
    capi.check(L.xf_stream_sync(None))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    res = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, res


def _capacity(n):
    cap = 1 << 16
    while cap * 0.55 < n:
        cap *= 2
    return cap


def evict_bytes(n, kept):
    return {"mark": 12.125 * n, "compact": 0.125 * n + 40.0 * kept, "dirs": 16.0 * kept,
            "zero_tail": 24.0 * (n - kept)}


def evict_leg(N, share, runs, copy_gbs):
    rng = np.random.default_rng(17)
    keys = capi.hash_decimal_range(0, N)
    drop = rng.random(N) < share
    w = np.where(drop, np.float32(0), np.float32(1)).astype(np.float32)
    n = np.where(drop, np.float32(0.5), np.float32(2)).astype(np.float32)
    z = np.full(N, 0.25, np.float32)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(N))
    dev, host = [], []
    for run in range(runs + 1):                 # (run 0: the warm cycle, not listed)
        t.import_(keys, w, n, z)
        t.defrag()
        assert t.settled == N == len(t)
        d_ms, h_ms, (seen, dropped) = _timed(lambda: t.evict(X))
        assert (seen, dropped) == (N, int(drop.sum())) and len(t) == N - dropped
        if run:
            dev.append(d_ms)
            host.append(h_ms)
    by = evict_bytes(N, N - int(drop.sum()))
    med = statistics.median(dev)
    return {"leg": "evict", "keys": N, "share": share, "dropped": int(drop.sum()),
            "device_ms": dev, "host_ms": host, "median_ms": med, "bytes": by,
            "gbs": sum(by.values()) / (med * 1e-3) / 1e9,
            "frac_of_copy_peak": sum(by.values()) / (med * 1e-3) / 1e9 / copy_gbs}


def defrag_leg(N, runs):
    """5 % of the keys in the arrival index, the rest settled; every run on a fresh table (a
    defrag cannot be undone), its second state buffer and tiers allocated before the clock
    (xf_table_prepare_defrag), as the worker does"""
    keys = capi.hash_decimal_range(0, N)
    cut = N - N // 20
    dev, host = [], []
    for run in range(runs + 1):                 # (run 0: the warm cycle, not listed)
        t = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(N))
        t.pull(keys[:cut])
        t.defrag()
        capi.check(capi.lib().xf_table_prepare_defrag(t.h))
        t.pull(keys[cut:])
        d_ms, h_ms, _ = _timed(t.defrag)
        assert t.settled == N
        if run:
            dev.append(d_ms)
            host.append(h_ms)
        del t
    return {"leg": "defrag", "keys": N, "arrival_share": 0.05, "device_ms": dev, "host_ms": host,
            "median_ms": statistics.median(dev)}


def push_leg(steps=100):
    R, NNZ, K = 50000, 200, 10_000_000
    rng = np.random.RandomState(11)
    keytab = capi.hash_decimal_range(0, K)
    rowptr = np.arange(R + 1, dtype=np.uint64) * np.uint64(NNZ)
    keys = keytab[rng.randint(0, K, size=R * NNZ)]
    labels = (rng.rand(R) < 0.05).astype(np.int32)
    live = np.unique(keys)
    dead = capi.hash_decimal_range(K, len(live))          # as many keys nobody ever steps
    t = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(2 * len(live)))
    t.pull(live)
    t.pull(dead)
    t.defrag()
    ws = capi.Workspace()
    b = capi.LocalBatch(t, rowptr, keys, labels)
    L = capi.lib()

    def grad_us():
        for _ in range(20):
            capi.lr_step(t, b, ws)
        capi.check(L.xf_stream_sync(None))
        ws.profile(True)
        for _ in range(steps):
            capi.lr_step(t, b, ws)
        capi.check(L.xf_stream_sync(None))
        ms, n = ws.profile_read()
        ws.profile(False)
        return ms["gradient"] / max(n, 1) * 1e3, ms["forward"] / max(n, 1) * 1e3, n
    before = grad_us()
    seen, dropped = t.evict(1e-30)                        # n == 0: the dead rows and no other
    assert seen == len(live) + len(dead) and dropped >= len(dead), (seen, dropped, len(dead))
    after = grad_us()
    t.check()
    return {"leg": "push", "rows": R, "nnz": R * NNZ, "U": int(len(live)),
            "table_keys_before": int(seen), "table_keys_after": int(seen - dropped),
            "steps_timed": [before[2], after[2]],
            "gradient_us_before": before[0], "gradient_us_after": after[0],
            "forward_us_before": before[1], "forward_us_after": after[1]}


if __name__ == "__main__":
    capi.require_gpu()
    sizes = [10_000_000, 100_000_000]
    args = sys.argv[2:]
    if "--keys" in args:
        sizes = [int(float(s)) for s in args[args.index("--keys") + 1].split(",")]
    from bench import stream_copy_gbs
    with open(sys.argv[1], "a") as out:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
        copy = stream_copy_gbs()
        emit({"leg": "copy", "gbs": copy})
        if "--skip-push" not in args:
            emit(push_leg())
        for N in sizes:
            runs = 5 if N <= 20_000_000 else 2
            for share in (0.001, 0.5, 0.99):
                emit(evict_leg(N, share, runs, copy))
            emit(defrag_leg(N, min(runs, 3)))
