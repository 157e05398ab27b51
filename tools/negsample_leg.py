#!/usr/bin/env python3
"""Negative subsampling measured on a GPU box: the sampler's time per 64 MiB text block beside
the key build of the sampled and of the unsampled block, on the two streams of
tools/admit_leg.py (uniform and Zipf(1.1) keys, bench-shaped rows of 200 tokens, key space 1e7),
and the weighted LR step beside the unweighted one at the shape of BASELINE.json configs[1].

    python tools/negsample_leg.py OUT.jsonl [block_mb]

Per stream one block is drawn as admit_leg draws its blocks (half its rows positive) and a second
text is made from it by rewriting the labels so that 5 % of the rows are positive (click data).
keep = 0.25.  Every figure is a host clock around a call that ends in a stream synchronise, in ms,
the median of 5 calls unless it says otherwise:
    apply            xf_negsample_apply_dev of the block (flag, scan, place, copy + the one wait)
    bytes_in/out     NNZ * 8 read and kept NNZ * 8 written (keys only: no fgid, no values), plus
                     R * 8 of row offsets and labels read twice and the kept rows' 12 bytes written
    apply_gbps       (bytes_in + bytes_out) / apply
    key_build_first  xf_sharded_compile_dev into an empty LR table (first-touch inserts), one call
                     each for the unsampled and the sampled block, each on a table of its own
    key_build_again  the same minibatch compiled again (every key in the table)
The step (one record, "stream": "lr_step"): 50 000 rows x 200 nonzeros over 1e7 keys, 5 % of the
rows positive, every key settled in the table (the steady state bench.py times); `runs` times 200
steps per weight, the weights taking turns (1, 4, 1, 4, ...), each run one host clock around 200
xf_lr_step and one stream synchronise -> us per step, every run listed."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import NNZ, K, block_text, ms  # noqa: E402

KEEP = 0.25
STREAM = 0


def relabel(text, positives, rng):
    """the same rows with other labels: the first byte of every line"""
    a = np.frombuffer(text, np.uint8).copy()
    starts = np.r_[0, np.flatnonzero(a[:-1] == 10) + 1]
    a[starts] = np.where(rng.rand(len(starts)) < positives, ord("1"), ord("0"))
    return a.tobytes()


def one_block(tag, text, cap, smp):
    ing = capi.Ingest(cap)
    ok, R, N, dk, dr, dl = ing.block_dev(text)
    assert ok
    smp.sample_dev(STREAM, 0, dk, dr, dl, R, N)           # (warm: code objects, the scratch)
    warm = capi.Sharded(model="lr", capacity=1 << 12)     # (... and the key build's, on 100 rows)
    warm.compile_dev(dk, dr, dl, min(R, 100), 100 * NNZ if R >= 100 else 0)
    warm.close()
    t_apply, d = ms(lambda: smp.sample_dev(STREAM, 0, dk, dr, dl, R, N), 5)
    bytes_in = N * 8 + 2 * R * 8
    bytes_out = d.NNZ * 8 + d.R * 12
    out = {"labels": tag, "rows": R, "nnz": N, "rows_kept": d.R, "nnz_kept": d.NNZ,
           "apply_ms": t_apply, "bytes_in": bytes_in, "bytes_out": bytes_out,
           "apply_gbps": (bytes_in + bytes_out) / t_apply / 1e6}
    for name, args in (("unsampled", (dk, dr, dl, R, N)), ("sampled", tuple(d[:5]))):
        st = capi.Sharded(model="lr", capacity=30_000_000)
        t1, mb = ms(lambda: st.compile_dev(*args))
        st.step(mb)
        st.check()
        t2, _ = ms(lambda: st.compile_dev(*args), 5)
        out["key_build_first_%s_ms" % name], out["key_build_again_%s_ms" % name] = t1, t2
        st.close()
    return out


def leg(name, zipf, block_mb):
    rng = np.random.RandomState(7)
    cap = block_mb << 20
    block_text(rng, cap, zipf)                            # (block A of admit_leg: B is the next draw)
    b = block_text(rng, cap, zipf)
    smp = capi.NegSample(KEEP, seed=0)
    recs = []
    for tag, text in (("half positive", b), ("5% positive", relabel(b, 0.05, rng))):
        rec = {"stream": name, "block_bytes": len(text), "keep": KEEP}
        rec.update(one_block(tag, text, cap, smp))
        recs.append(rec)
    return recs


def step_leg(runs=7, steps=200):
    rng = np.random.RandomState(11)
    R, nnz = 50000, NNZ
    keytab = capi.hash_decimal_range(0, K)
    rowptr = (np.arange(R + 1, dtype=np.uint64) * np.uint64(nnz))
    keys = keytab[rng.randint(0, K, size=R * nnz)]
    labels = (rng.rand(R) < 0.05).astype(np.int32)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 25)
    t.pull(keytab)
    t.defrag()
    b = capi.LocalBatch(t, rowptr, keys, labels)
    ws = capi.Workspace()
    L = capi.lib()
    out = {1.0: [], 4.0: []}
    for w in (1.0, 4.0):                                  # (warm: both kernels' code objects)
        ws.neg_weight(w)
        for _ in range(20):
            capi.lr_step(t, b, ws)
    for _ in range(runs):
        for w in (1.0, 4.0):
            ws.neg_weight(w)
            capi.check(L.xf_stream_sync(None))
            t0 = time.perf_counter()
            for _ in range(steps):
                capi.lr_step(t, b, ws)
            capi.check(L.xf_stream_sync(None))
            out[w].append((time.perf_counter() - t0) / steps * 1e6)
    t.check()
    return {"stream": "lr_step", "rows": R, "nnz": R * nnz, "keys": K, "steps_per_run": steps,
            "unweighted_us": out[1.0], "weighted_us": out[4.0],
            "unweighted_median_us": statistics.median(out[1.0]),
            "weighted_median_us": statistics.median(out[4.0])}


if __name__ == "__main__":
    capi.require_gpu()
    block_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    with open(sys.argv[1], "a") as out:
        for name, zipf in (("uniform", None), ("zipf1.1", 1.1)):
            for rec in leg(name, zipf, block_mb):
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
        rec = step_leg()
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
