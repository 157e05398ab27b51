#!/usr/bin/env python3
"""Value binning measured on a GPU box: k_bin_count and k_bin_apply on the nonzeros of one 64 MiB
block of click rows beside xf_calib_stream moving the same bytes, in the same run.

    python tools/bin_leg.py OUT.jsonl [nonzeros] [calls]

The block: a row holds one token per field; the first `listed` fields are numeric and listed with
32 bins each — 13 of 39 (the Criteo shape), 32 of 64 (the most LUTs that fit LDS) and 64 of 64
(every nonzero listed, eight groups of the count).  Numeric values are counts: 70 % small integers
0 .. 19, the rest exp(N(0, 4)).

Every figure is a host clock around `calls` calls (default 2000) EACH followed by a device
synchronise — xf_calib_stream ends in one itself, so both sides pay the same round trip per call
— divided by calls, in ms, the median of 5 such windows after a warm call of the same shape:
    count        xf_bin_count_dev: 8 bytes read per nonzero, once per group of 8 listed fields
    calib_count  xf_calib_stream reading 8 * nnz bytes `groups` times in one call (16 B per lane):
                 the same buffer again and again, as the count's groups read the same arrays
    apply        xf_bin_apply_dev: 16 bytes read, 12 written per nonzero, LUTs in global memory
    apply_lds    the same with the LUTs staged in LDS (only a library built with
                 XF_EXTRA_FLAGS=-DXF_EXPERIMENTS has the variant, exp_knob 410; null otherwise, and
                 for specs of more than 32 fields, whose LUTs do not fit)
    calib_read / calib_write   xf_calib_stream reading 16 * nnz / writing 12 * nnz bytes, one call
                 each: the apply does both in one launch, so it stands beside their sum and beside
                 the larger of the two
Kernel times without the host's round trip come from a run of this script under
rocprofv3 --kernel-trace --stats (profiles/bin/README.md)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xflow_amd import capi  # noqa: E402


def sync():
    capi.check(capi.lib().xf_stream_sync(None))


def window(fn, calls):
    fn()
    sync()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
            sync()
        ts.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(ts))


def has_experiments():
    try:
        capi.tune("exp_knob", 0)
        return True
    except capi.XFError:
        return False


def leg(nnz, fields, listed, calls):
    rng = np.random.RandomState(5)
    fgid = (np.arange(nnz) % fields).astype(np.int32)
    vals = rng.randint(0, 20, size=nnz).astype(np.float32)
    vals = np.where(rng.rand(nnz) < 0.3, np.exp(rng.randn(nnz) * 4), vals).astype(np.float32)
    keys = rng.randint(0, 1 << 62, size=nnz).astype(np.uint64)
    rowptr = np.array([0, nnz], np.uint64)
    spec = [(f, 32) for f in range(listed)]
    fit = capi.Bin(spec)
    fit.count(fgid, vals)
    fit.fit()
    up = capi.Cross("300*301")       # (a cross none of whose fields occur: the block's uploader)
    d = up.apply_dev(rowptr, keys, fgid, values=vals)
    sync()
    cnt = capi.Bin(spec)
    L = capi.lib()
    groups = (listed + 7) // 8
    rec = {"nnz": nnz, "fields": fields, "listed": listed, "count_groups": groups, "calls": calls}
    rec["count_ms"] = window(lambda: cnt.count_dev(d.d_fgid, d.d_vals, nnz), calls)
    rec["calib_count_ms"] = window(lambda: capi.check(L.xf_calib_stream(2, 8 * nnz, groups)), calls)
    # the two apply variants alternate, window by window
    apply = lambda: fit.bin_dev(d.d_keys, d.d_fgid, d.d_vals, nnz)  # noqa: E731
    lds = has_experiments() and listed <= 32
    a, b = [], []
    for _ in range(3):
        a.append(window(apply, calls))
        if lds:
            capi.tune("exp_knob", 410)
            b.append(window(apply, calls))
            capi.tune("exp_knob", 0)
    rec["apply_ms"] = float(np.median(a))
    rec["apply_lds_ms"] = float(np.median(b)) if lds else None
    rec["calib_read_ms"] = window(lambda: capi.check(L.xf_calib_stream(2, 16 * nnz, 1)), calls)
    rec["calib_write_ms"] = window(lambda: capi.check(L.xf_calib_stream(5, 12 * nnz, 1)), calls)
    return rec


if __name__ == "__main__":
    capi.require_gpu()
    nnz = int(sys.argv[2]) if len(sys.argv) > 2 else 4_300_000
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    with open(sys.argv[1], "a") as out:
        for fields, listed in ((39, 13), (64, 32), (64, 64)):
            rec = leg(nnz, fields, listed, calls)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
