#!/usr/bin/env python3
"""Progressive validation measured on a GPU box: the LR cells step with a progress attached beside
the same step without one, at the shape of BASELINE.json configs[1], and the accumulate kernel
alone at that R on three loss vectors.

    python tools/progress_leg.py OUT.jsonl

The step (record "lr_step"): 50 000 rows x 200 nonzeros over 1e7 keys, 5 % of the rows positive,
every key settled in the table (the steady state bench.py times; tools/negsample_leg.py's shape);
`runs` times 200 steps per setting, the settings taking turns (off, on, off, on, ...), each run one
host clock around 200 xf_lr_step and one stream synchronise -> us per step, every run listed.
The kernel (records "accumulate"): R = 50 000 losses, 5 % of the rows positive:
    spread      q uniform in [0, 1): about as many ranks as rows
    click       p clustered (logits N(-3, 0.5^2)): a few hundred ranks
    one_rank    every row's q = 0.5: one word per class
`runs` times 200 launches and one stream synchronise -> us per launch, every run listed."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import NNZ, K  # noqa: E402

R = 50000


def step_leg(runs=7, steps=200):
    rng = np.random.RandomState(11)
    nnz = NNZ
    keytab = capi.hash_decimal_range(0, K)
    rowptr = (np.arange(R + 1, dtype=np.uint64) * np.uint64(nnz))
    keys = keytab[rng.randint(0, K, size=R * nnz)]
    labels = (rng.rand(R) < 0.05).astype(np.int32)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 25)
    t.pull(keytab)
    t.defrag()
    b = capi.LocalBatch(t, rowptr, keys, labels)
    ws = capi.Workspace()
    p = capi.Progress()
    L = capi.lib()
    out = {False: [], True: []}
    for on in (False, True):                              # (warm: both kernels' code objects)
        ws.progress(p if on else None)
        for _ in range(20):
            capi.lr_step(t, b, ws)
    for _ in range(runs):
        for on in (False, True):
            ws.progress(p if on else None)
            capi.check(L.xf_stream_sync(None))
            t0 = time.perf_counter()
            for _ in range(steps):
                capi.lr_step(t, b, ws)
            capi.check(L.xf_stream_sync(None))
            out[on].append((time.perf_counter() - t0) / steps * 1e6)
    ws.progress(None)
    t.check()
    counts, other = p.read()
    assert counts.sum() + other.sum() == (20 + runs * steps) * R
    return {"leg": "lr_step", "rows": R, "nnz": R * nnz, "keys": K, "steps_per_run": steps,
            "off_us": out[False], "on_us": out[True],
            "off_median_us": statistics.median(out[False]),
            "on_median_us": statistics.median(out[True])}


def kernel_leg(name, loss, labels, runs=7, launches=200):
    import torch
    d_loss = torch.from_numpy(loss).cuda()
    d_lab = torch.from_numpy(labels).cuda()
    p = capi.Progress()
    L = capi.lib()
    for _ in range(20):
        p.accumulate(d_loss.data_ptr(), d_lab.data_ptr(), len(loss))
    us = []
    for _ in range(runs):
        capi.check(L.xf_stream_sync(None))
        t0 = time.perf_counter()
        for _ in range(launches):
            p.accumulate(d_loss.data_ptr(), d_lab.data_ptr(), len(loss))
        capi.check(L.xf_stream_sync(None))
        us.append((time.perf_counter() - t0) / launches * 1e6)
    counts, other = p.read()
    assert counts.sum() + other.sum() == (20 + runs * launches) * len(loss)
    return {"leg": "accumulate", "vector": name, "rows": len(loss),
            "distinct_words": int((counts != 0).sum()), "launches_per_run": launches, "us": us,
            "median_us": statistics.median(us)}


def vectors():
    rng = np.random.RandomState(13)
    y = (rng.rand(R) < 0.05).astype(np.int32)
    sign = np.where(y != 0, np.float32(-1), np.float32(1))
    spread = rng.rand(R).astype(np.float32)
    click_p = (1.0 / (1.0 + np.exp(-rng.normal(-3.0, 0.5, size=R)))).astype(np.float32)
    click = np.where(y != 0, np.float32(1) - click_p, click_p).astype(np.float32)
    one = np.full(R, 0.5, np.float32)
    return [(n, (q * sign).astype(np.float32), y) for n, q in
            (("spread", spread), ("click", click), ("one_rank", one))]


if __name__ == "__main__":
    capi.require_gpu()
    with open(sys.argv[1], "a") as out:
        recs = [kernel_leg(*v) for v in vectors()] + [step_leg()]
        for rec in recs:
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
