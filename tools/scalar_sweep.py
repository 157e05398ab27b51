#!/usr/bin/env python3
"""The scalar layer on every float, device against host, timed: sigmoid_ref, sqrtf and div_by_rows
(seven row counts) through xf_scalar_sweep and the oracle's xo_scalar_sweep, all 2^32 inputs each.

  python tools/scalar_sweep.py [OUT.jsonl]

One JSON record per sweep: device_s (a host clock around the call: allocation, one launch of
65536 workgroups, the copy of the digests back), host_s (the oracle on `threads` threads),
blocks_differing, and — from the elementwise probe on the differing blocks — n_inputs_differing
with the first of them as "input: device, host" bit patterns.  tests/test_gpu_scalar.py asserts
what this reports."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as O  # noqa: E402
from xflow_amd import capi  # noqa: E402

ROWS = (1, 3, 50000, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 32) - 1)


def is_nan_bits(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    capi.require_gpu()
    threads = O.sweep_threads()
    capi.scalar_sweep(capi.SCALAR_SQRT, 0, 0, 16)   # the code object's load is not a sweep's time
    cases = [("sigmoid_ref", capi.SCALAR_SIGMOID, 0), ("sqrtf", capi.SCALAR_SQRT, 0)] + \
        [("div_by_rows", capi.SCALAR_DIV_ROWS, r) for r in ROWS]
    for name, op, param in cases:
        t = time.perf_counter()
        dev = capi.scalar_sweep(op, param)
        device_s = time.perf_counter() - t
        t = time.perf_counter()
        host = O.scalar_sweep(op, param, 0, 1 << 16, threads)
        host_s = time.perf_counter() - t
        bad = np.flatnonzero(dev != host)
        n, first = 0, []
        for blk in bad:
            a = (np.arange(65536, dtype=np.uint32) + np.uint32(int(blk) << 16))
            g = capi.scalar_probe(op, a.view(np.float32), None, param).view(np.uint32)
            w = O.scalar_ref(op, a.view(np.float32), None, param).view(np.uint32)
            idx = np.flatnonzero((g != w) & ~(is_nan_bits(g) & is_nan_bits(w)))
            n += idx.size
            first += ["%08x: %08x, %08x" % (a[i], g[i], w[i]) for i in idx[:100 - len(first)]]
        rec = dict(op=name, rows=param or None, inputs=1 << 32, threads=threads,
                   device_s=round(device_s, 4), host_s=round(host_s, 3),
                   blocks_differing=int(bad.size), n_inputs_differing=n, first_differing=first)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
