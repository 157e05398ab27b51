#!/usr/bin/env python3
"""Sliced progressive validation measured on a GPU box, at the shape of BASELINE.json configs[1].

    python tools/slices_leg.py OUT.jsonl

The step (records "lr_step"): 50 000 rows x 200 nonzeros over 1e7 keys, 5 % of the rows positive,
every key settled in the table (tools/progress_leg.py's step).  Three settings take turns in one
session — a progress attached alone, a progress and slices with ids on D distinct slices — for
D in 10, 1e3, 1e5, ids drawn uniformly and Zipf(1.1); `runs` times 200 steps per setting, each run
one host clock around 200 (xf_workspace_slice_ids +) xf_lr_step and one stream synchronise -> us
per step, every run listed.  The progress-alone setting also makes the ids call's ctypes trip (with
no ids), so the difference is the device's.
The kernel (records "accumulate"): xf_slices_accumulate_dev alone at R = 50 000 on the same ids and
click-shaped losses; 200 launches and one synchronise -> us per launch.
The extract (record "extract"): xf_slices_extract_dev alone on the CSR arrays of a 64 MiB text block
of click-shaped rows (39 fields a row, one token each, the sliced field at position 3), beside
xf_calib_stream reading the bytes the kernel reads (a row's fgids, its two offsets, one key) and
writing the bytes it writes (one id a row), 16 B per lane; ms per call, median of five."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import NNZ, K, ms  # noqa: E402

R = 50000
SLOTS = 20          # 2^20 entries: 1e5 slices at a load of 0.1


def draw_ids(rng, distinct, zipf):
    pool = capi.hash_decimal_range(1, distinct)
    if zipf:
        at = np.minimum(rng.zipf(1.1, size=R), distinct) - 1
    else:
        at = rng.randint(0, distinct, size=R)
    return pool[at]


def settings():
    rng = np.random.RandomState(29)
    return [("%s_%d" % ("zipf" if z else "uniform", d), draw_ids(rng, d, z))
            for d in (10, 1000, 100000) for z in (False, True)]


def step_leg(runs=5, steps=200):
    import torch
    rng = np.random.RandomState(11)
    keytab = capi.hash_decimal_range(0, K)
    rowptr = (np.arange(R + 1, dtype=np.uint64) * np.uint64(NNZ))
    keys = keytab[rng.randint(0, K, size=R * NNZ)]
    labels = (rng.rand(R) < 0.05).astype(np.int32)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 25)
    t.pull(keytab)
    t.defrag()
    b = capi.LocalBatch(t, rowptr, keys, labels)
    ws = capi.Workspace()
    p = capi.Progress()
    ws.progress(p)
    L = capi.lib()
    recs = []
    for name, ids in settings():
        s = capi.Slices(3, SLOTS)
        ws.slices(s)
        d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
        ptr = {False: None, True: d_ids.data_ptr()}
        out = {False: [], True: []}
        for on in (False, True):                          # (warm: the code objects, the table's keys)
            for _ in range(20):
                ws.slice_ids(ptr[on], R)
                capi.lr_step(t, b, ws)
        for _ in range(runs):
            for on in (False, True):
                capi.check(L.xf_stream_sync(None))
                t0 = time.perf_counter()
                for _ in range(steps):
                    ws.slice_ids(ptr[on], R)
                    capi.lr_step(t, b, ws)
                capi.check(L.xf_stream_sync(None))
                out[on].append((time.perf_counter() - t0) / steps * 1e6)
        keys_out, words, none, overflow = s.read()
        fed = (20 + runs * steps) * R
        assert int(words[:, [0, 1, 6]].sum()) + int(none[[0, 1, 6]].sum()) + \
            int(overflow[[0, 1, 6]].sum()) == fed
        ws.slices(None)
        recs.append({"leg": "lr_step", "ids": name, "rows": R, "nnz": R * NNZ, "keys": K,
                     "slices_resident": len(keys_out), "overflow_rows": int(overflow[[0, 1, 6]].sum()),
                     "log2_slots": SLOTS, "steps_per_run": steps,
                     "progress_us": out[False], "sliced_us": out[True],
                     "progress_median_us": statistics.median(out[False]),
                     "sliced_median_us": statistics.median(out[True])})
    ws.progress(None)
    t.check()
    return recs


def kernel_leg(runs=5, launches=200):
    import torch
    rng = np.random.RandomState(13)
    y = (rng.rand(R) < 0.05).astype(np.int32)
    click_p = (1.0 / (1.0 + np.exp(-rng.normal(-3.0, 0.5, size=R)))).astype(np.float32)
    loss = (click_p - y.astype(np.float32)).astype(np.float32)
    d_loss, d_lab = torch.from_numpy(loss).cuda(), torch.from_numpy(y).cuda()
    L = capi.lib()
    recs = []
    for name, ids in settings():
        d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
        s = capi.Slices(3, SLOTS)
        args = (d_loss.data_ptr(), d_lab.data_ptr(), d_ids.data_ptr(), R)
        for _ in range(20):
            s.accumulate(*args)
        us = []
        for _ in range(runs):
            capi.check(L.xf_stream_sync(None))
            t0 = time.perf_counter()
            for _ in range(launches):
                s.accumulate(*args)
            capi.check(L.xf_stream_sync(None))
            us.append((time.perf_counter() - t0) / launches * 1e6)
        recs.append({"leg": "accumulate", "ids": name, "rows": R, "slices": s.count(),
                     "launches_per_run": launches, "us": us, "median_us": statistics.median(us)})
    return recs


def extract_leg(block_mb=64, fields=39, at=3):
    import torch
    rows = (block_mb << 20) // (fields * 12)          # (a token of such a block is ~12 bytes of text)
    nnz = rows * fields
    rng = np.random.RandomState(7)
    keys = capi.hash_decimal_range(0, 1 << 20)[rng.randint(0, 1 << 20, size=nnz)]
    fgid = (np.arange(nnz, dtype=np.int64) % fields).astype(np.int32)
    rowptr = (np.arange(rows + 1, dtype=np.int64) * fields).astype(np.uint32)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    df = torch.from_numpy(fgid).cuda()
    dr = torch.from_numpy(rowptr.view(np.int32)).cuda()
    s = capi.Slices(at, 2)
    L = capi.lib()

    def extract():
        d = s.extract_dev(dk.data_ptr(), df.data_ptr(), dr.data_ptr(), rows, nnz)
        capi.check(L.xf_stream_sync(None))
        return d

    d = extract()
    ids = capi.Slices.download_ids(d, rows)
    assert np.array_equal(ids, keys[at::fields])
    t_extract, _ = ms(extract, 5)
    bytes_in, bytes_out = nnz * 4 + rows * (4 + 8), rows * 8

    def calib():
        capi.check(L.xf_calib_stream(2, bytes_in, 1))
        capi.check(L.xf_calib_stream(5, bytes_out, 1))
        capi.check(L.xf_stream_sync(None))

    calib()
    t_calib, _ = ms(calib, 5)
    return [{"leg": "extract", "block_mb": block_mb, "rows": rows, "nnz": nnz, "fields": fields,
             "bytes_in": bytes_in, "bytes_out": bytes_out, "extract_ms": t_extract,
             "extract_gbps": (bytes_in + bytes_out) / t_extract / 1e6, "calib_ms": t_calib}]


if __name__ == "__main__":
    capi.require_gpu()
    with open(sys.argv[1], "a") as out:
        for leg in (extract_leg, kernel_leg, step_leg):
            for rec in leg():
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
