#!/usr/bin/env python3
"""Held-out validation measured on a GPU box: the split's time per 64 MiB text block beside the
negative sampler's apply on the same block in the same run, and validate beside predict on the
held part, on the two streams of tools/negsample_leg.py (uniform and Zipf(1.1) keys, bench-shaped
rows of 200 tokens, key space 1e7; block B of tools/admit_leg.py, 5 % of its rows positive).

    python tools/holdout_leg.py OUT.jsonl [block_mb]

share = keep = 0.25.  Every figure is a host clock around a call that ends in a stream
synchronise, in ms, the median of 5 calls, the two calls of a pair taking turns:
    split            xf_holdout_split_dev of the block (flag, scan, place, copy + the one wait)
    apply            xf_negsample_apply_dev of the same block (the same four passes, one output)
    bytes            the split reads NNZ * 8 of keys and R * 8 of row offsets and labels twice and
                     writes EVERY nonzero (NNZ * 8) and every row (R * 12); the sampler writes the
                     kept ones only — split_gbps / apply_gbps set the two against their own traffic
    split_over_apply the ratio of the two times
    predict          xf_sharded_predict of the held part compiled into a table that holds every key
                     of the block (forward + the copy of pctr to the host)
    validate         xf_sharded_validate of the same minibatch + the stream synchronise a reader
                     of the counts would wait for (forward + one accumulate launch, nothing copied)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import block_text, ms  # noqa: E402
from negsample_leg import relabel  # noqa: E402

SHARE = KEEP = 0.25
STREAM = 0


def median_pair(fa, fb, n=5):
    """the medians of n calls each of fa and fb, taking turns"""
    ta, tb, ra, rb = [], [], None, None
    for _ in range(n):
        t, ra = ms(fa)
        ta.append(t)
        t, rb = ms(fb)
        tb.append(t)
    return float(np.median(ta)), ra, float(np.median(tb)), rb


def leg(name, zipf, block_mb):
    rng = np.random.RandomState(7)
    cap = block_mb << 20
    block_text(rng, cap, zipf)                            # (block A of admit_leg: B is the next draw)
    text = relabel(block_text(rng, cap, zipf), 0.05, rng)
    ing = capi.Ingest(cap)
    ok, R, N, dk, dr, dl = ing.block_dev(text)
    assert ok
    split, smp = capi.Holdout(SHARE, seed=0), capi.NegSample(KEEP, seed=0)
    split.part_dev(STREAM, 0, dk, dr, dl, R, N)           # (warm: code objects, the scratch)
    smp.sample_dev(STREAM, 0, dk, dr, dl, R, N)
    t_split, parts, t_apply, d = median_pair(
        lambda: split.part_dev(STREAM, 0, dk, dr, dl, R, N),
        lambda: smp.sample_dev(STREAM, 0, dk, dr, dl, R, N))
    train, held = parts
    assert train.R + held.R == R and train.NNZ + held.NNZ == N
    read = N * 8 + 2 * R * 8
    rec = {"stream": name, "block_bytes": len(text), "share": SHARE, "keep": KEEP, "rows": R,
           "nnz": N, "rows_held": held.R, "nnz_held": held.NNZ, "rows_kept": d.R, "nnz_kept": d.NNZ,
           "split_ms": t_split, "apply_ms": t_apply, "split_over_apply": t_split / t_apply,
           "split_gbps": (read + N * 8 + R * 12) / t_split / 1e6,
           "apply_gbps": (read + d.NNZ * 8 + d.R * 12) / t_apply / 1e6}
    st = capi.Sharded(model="lr", capacity=30_000_000)
    st.set_holdout(True)
    st.step(st.compile_dev(dk, dr, dl, R, N))             # every key of the block is in the table
    st.check()
    hb = st.compile_dev(*held[:5])
    st.predict(hb)
    st.validate(hb)
    st.flush()

    def validate():
        st.validate(hb)
        st.flush()
        capi.check(capi.lib().xf_stream_sync(None))
    rec["predict_ms"], _, rec["validate_ms"], _ = median_pair(lambda: st.predict(hb), validate)
    rec["validate_over_predict"] = rec["validate_ms"] / rec["predict_ms"]
    counts, other = st.holdout_read(reset=True)
    assert int(counts.sum() + other.sum()) == 6 * held.R  # (the warm call and the 5 timed ones)
    st.close()
    return rec


if __name__ == "__main__":
    capi.require_gpu()
    block_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    with open(sys.argv[1], "a") as out:
        for name, zipf in (("uniform", None), ("zipf1.1", 1.1)):
            rec = leg(name, zipf, block_mb)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
