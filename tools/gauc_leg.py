#!/usr/bin/env python3
"""The grouped AUC measured on a GPU box: one xf_gauc_reduce of 2 * 10^6 records (5 % of 4 * 10^7
rows held) under three id distributions, and one xf_gauc_append_dev of a held minibatch beside
xf_progress_accumulate_dev on the same rows.

    python tools/gauc_leg.py OUT.jsonl [records]

Every figure is the time between two device events on the null stream around the call (a reduce
holds its own stream waits, so that is the call's whole time), warm, in ms, the median of 5 calls:
    ids              one_group: every record in one group; zipf1.1: Zipf(1.1) over 10^5 ids;
                     distinct: every record a group of its own
    reduce_ms        xf_gauc_reduce with the entries copied out (no reset: the log stays)
    count_ms         the same without entries: the two sorts, the tile pass and the scan — what is
                     left of reduce_ms is the group pass and the copy of the entries
    reduce_pinned_ms reduce_ms with the entries copied into page-locked host memory instead of a
                     numpy array: the difference is what copying 40 bytes a group into pageable
                     memory costs
    groups           the entries
    append_ms        xf_gauc_append_dev of `mb_rows` rows (the held part of one 64 MiB block of
                     profiles/holdout/README.md) into a log sized ahead
    accumulate_ms    xf_progress_accumulate_dev on the same rows
The scores are those of a trained model: p = sigmoid(N(0, 2)), 5 % of the rows positive."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xflow_amd import capi  # noqa: E402

MB_ROWS = 5515


def event_ms(fn, n=5):
    import torch
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), r


def rows(rng, n):
    p = (1.0 / (1.0 + np.exp(-rng.normal(0, 2, size=n)))).astype(np.float32)
    y = (rng.random(n) < 0.05).astype(np.int32)
    return (p - y.astype(np.float32)).astype(np.float32), y


def ids_of(name, rng, n):
    if name == "one_group":
        return np.full(n, 0x1234567890ABCDEF, np.uint64)
    table = (np.arange(1, max(n, 100000) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    if name == "distinct":
        return rng.permutation(table[:n])
    return table[np.minimum(rng.zipf(1.1, size=n), 100000) - 1]


def leg(name, n):
    import torch
    rng = np.random.default_rng(11)
    loss, y = rows(rng, n)
    ids = ids_of(name, rng, n)
    d_loss, d_y = torch.from_numpy(loss).cuda(), torch.from_numpy(y).cuda()
    d_id = torch.from_numpy(ids.view(np.int64)).cuda()
    g = capi.Gauc()
    g.reserve(n + 8 * MB_ROWS)
    g.append_dev(d_loss.data_ptr(), d_y.data_ptr(), d_id.data_ptr(), n)
    capi.stream_sync()
    assert g.count() == n
    g.reduce()                                              # (warm: code objects, the buffers)
    t_count, groups = event_ms(g.groups)
    t_reduce, got = event_ms(lambda: g.reduce(cap=groups))
    assert len(got[0]) == groups and int(got[1][:, :2].sum()) == n
    rec = {"ids": name, "records": n, "groups": groups, "reduce_ms": t_reduce, "count_ms": t_count,
           "scored": int(((got[1][:, 0] > 0) & (got[1][:, 1] > 0)).sum())}
    # the same into page-locked host memory: what of reduce_ms is the copy into pageable memory
    pinned = torch.empty((max(groups, 1), capi.GAUC_WORDS + 1), dtype=torch.int64).pin_memory()
    m = capi.C.c_uint64()

    def into_pinned():
        capi.check(capi.lib().xf_gauc_reduce(g.h, capi.C.cast(pinned.data_ptr(), capi.u64p),
                                             max(groups, 1), capi.C.byref(m), None, None, 0))
    into_pinned()
    rec["reduce_pinned_ms"], _ = event_ms(into_pinned)
    assert m.value == groups and np.array_equal(pinned.numpy().view(np.uint64)[:groups, 0], got[0])
    # one held minibatch: the pack beside the progress's accumulate, on the same rows
    p = capi.Progress()
    R = MB_ROWS
    p.accumulate(d_loss.data_ptr(), d_y.data_ptr(), R)
    rec["mb_rows"] = R
    rec["append_ms"], _ = event_ms(lambda: g.append_dev(d_loss.data_ptr(), d_y.data_ptr(),
                                                        d_id.data_ptr(), R))
    rec["accumulate_ms"], _ = event_ms(lambda: p.accumulate(d_loss.data_ptr(), d_y.data_ptr(), R))
    return rec


if __name__ == "__main__":
    capi.require_gpu()
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    with open(sys.argv[1], "a") as out:
        for name in ("one_group", "zipf1.1", "distinct"):
            rec = leg(name, n)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
