#!/usr/bin/env python3
"""Experiment driver (GPU box): feature values (feature_values=on) beside the binary paths, on
the same four minibatches of bench.py's generator, the two sides alternated within one call.
  * canonical FM — BASELINE configs[3] (k = 16 + SGD, 10^7 keys, the config-2 row shape) and
    k = 64 + FTRL on the Zipf(1.1) stream: the valued step against the binary canonical step.
    The valued step streams 8 NNZ more bytes (xval in the forward, coo_val in the gradient);
    the margin of the ratio is the spread of the binary figure over its five repeats.
  * the generic build (xf_batch_compile_dev) with and without values, same shapes: host clock
    around a call that ends in a stream wait.
  * valued LR at the configs[1] shape beside the binary cells step — for orientation only: a
    different algorithm (sort-based build, Pull, gradient tiles).
Compiled minibatches replayed from HBM, device events, every shape warmed up, five repeats.  One
JSON line.  --leg k16_sgd | k64_ftrl | lr runs one configuration (a profiler run of its own).
  python tools/valued_leg.py [--leg L] [--rows R --nnz-per-row N --keys-per-gpu K]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.fm_canonical_leg import canonical_bytes  # noqa: E402

PEAK_BYTES_PER_S = 8e12
NB, STEPS, REPEATS = 4, 40, 5


def values_for(batches, seed=5):
    """a value per nonzero, magnitudes 2^-4 ... 4, both signs, one in ten an exact zero"""
    rng = np.random.RandomState(seed)
    out = []
    for rowptr, keys, labels in batches:
        n = len(keys)
        x = np.exp2(rng.uniform(-4, 2, size=n)).astype(np.float32)
        x *= rng.choice(np.array([-1.0, 1.0], np.float32), size=n)
        x[rng.rand(n) < 0.1] = 0.0
        out.append(x)
    return out


def lr_bytes(NNZ, R, U, opt, valued):
    """SURVEY 8(d), LR: 12 NNZ + 8 R + (32 FTRL | 16 SGD) U; valued: + 8 NNZ (the two value arrays)"""
    return NNZ * (20 if valued else 12) + 8 * R + (32 if opt == "ftrl" else 16) * U


def timed(trainers, comps):
    """ms/step per side, REPEATS times, the sides alternated repeat by repeat"""
    import torch
    per = [[] for _ in trainers]
    for _ in range(REPEATS):
        for s, (tr, comp) in enumerate(zip(trainers, comps)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(STEPS):
                tr.step(comp[i % NB])
            e1.record()
            e1.synchronize()
            per[s].append(e0.elapsed_time(e1) / STEPS)
    return per


def side(per, comp, nbytes):
    ms = min(per)
    R = sum(c.R for c in comp) / NB
    return {"ms_per_step": ms, "ms_per_step_repeats": per,
            "spread": (max(per) - min(per)) / min(per), "examples_per_sec": R / (ms * 1e-3),
            "R": R, "NNZ": sum(c.NNZ for c in comp) / NB, "U": sum(c.U for c in comp) / NB,
            "algorithmic_bytes": nbytes, "fraction_of_8TBps": nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S}


def prepare(tr, comp):
    for c in comp:
        tr.predict(c)          # every key in the tables before the clock starts
    tr.check()
    tr.defrag()
    for i in range(2 * NB):    # warm-up: every minibatch, twice
        tr.step(comp[i % NB])
    tr.check()


def build_ms(batches, vals):
    """the generic build from device arrays, with and without values: ms per build (host clock;
    the call waits for its stream), alternated, after a warm-up build of each"""
    import ctypes as C
    import torch
    from xflow_amd import capi
    L = capi.lib()
    # (xf_batch_compile_dev also lays out the LR forward's panel view, which the valued build —
    # like every FM build — leaves out: switched off here, so that the two builds differ by the
    # values alone)
    capi.tune("min_panel_nnz", 1e18)
    per = {"binary": [], "valued": []}
    for rep in range(REPEATS + 1):
        for name in ("binary", "valued"):
            t = 0.0
            for (rowptr, keys, labels), x in zip(batches[:NB], vals):
                dk = torch.from_numpy(keys.view(np.int64)).cuda()
                dr = torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).cuda()
                dl = torch.from_numpy(labels).cuda()
                dv = torch.from_numpy(x).cuda()
                torch.cuda.synchronize()
                h = capi.vp()
                t0 = time.perf_counter()
                if name == "valued":
                    capi.check(L.xf_batch_compile_valued_dev(
                        C.byref(h), dk.data_ptr(), dv.data_ptr(), dr.data_ptr(), dl.data_ptr(),
                        len(labels), len(keys), None))
                else:
                    capi.check(L.xf_batch_compile_dev(C.byref(h), dk.data_ptr(), dr.data_ptr(),
                                                      dl.data_ptr(), len(labels), len(keys), None))
                torch.cuda.synchronize()
                t += time.perf_counter() - t0
                L.xf_batch_free(h)
            if rep:            # (the first round warms the builders' scratch up)
                per[name].append(t / NB * 1e3)
    capi.tune("min_panel_nnz", 4e6)
    return {n: {"ms_per_build": min(p), "ms_per_build_repeats": p} for n, p in per.items()}


def fm_leg(args, k, opt):
    from xflow_amd.single import SingleGpuTrainer
    keytab = bench.make_key_table(args.keys_per_gpu)
    batches = bench.make_batches(args, 0, args.keys_per_gpu, keytab)[:NB]
    vals = values_for(batches)
    cap = int(args.keys_per_gpu / args.load_factor) + 1024
    a = SingleGpuTrainer(model="fm", optimizer=opt, k=k, capacity=cap, fm_mode="canonical")
    b = SingleGpuTrainer(model="fm", optimizer=opt, k=k, capacity=cap, fm_mode="canonical",
                         feature_values=True)
    ca = [a.compile(*m) for m in batches]
    cb = [b.compile(*m, values=x) for m, x in zip(batches, vals)]
    prepare(a, ca)
    prepare(b, cb)
    pa, pb = timed((a, b), (ca, cb))
    R, NNZ, U = (sum(getattr(c, n) for c in ca) / NB for n in ("R", "NNZ", "U"))
    cbytes = canonical_bytes(NNZ, R, U, k, opt)
    res = {"k": k, "optimizer": opt, "zipf": args.zipf,
           "binary_canonical": side(pa, ca, cbytes),
           "valued_canonical": side(pb, cb, cbytes + 8 * NNZ)}
    res["valued_over_binary"] = res["valued_canonical"]["ms_per_step"] / \
        res["binary_canonical"]["ms_per_step"]
    res["margin_binary_spread"] = res["binary_canonical"]["spread"]
    del a, b, ca, cb
    res["generic_build"] = build_ms(batches, vals)
    return res


def lr_leg(args, opt="ftrl"):
    from xflow_amd.single import SingleGpuTrainer
    keytab = bench.make_key_table(args.keys_per_gpu)
    batches = bench.make_batches(args, 0, args.keys_per_gpu, keytab)[:NB]
    vals = values_for(batches)
    cap = int(args.keys_per_gpu / args.load_factor) + 1024
    a = SingleGpuTrainer(model="lr", optimizer=opt, capacity=cap)
    b = SingleGpuTrainer(model="lr", optimizer=opt, capacity=cap, feature_values=True)
    ca = [a.compile(*m) for m in batches]
    cb = [b.compile(*m, values=x) for m, x in zip(batches, vals)]
    prepare(a, ca)
    prepare(b, cb)
    pa, pb = timed((a, b), (ca, cb))
    R, NNZ, U = (sum(getattr(c, n) for c in cb) / NB for n in ("R", "NNZ", "U"))

    class _Dims:   # (the cells minibatch has no key list: the valued one's dimensions)
        pass
    da = []
    for c in cb:
        d = _Dims()
        d.R, d.NNZ, d.U = c.R, c.NNZ, c.U
        da.append(d)
    return {"optimizer": opt, "zipf": args.zipf,
            "binary_cells": side(pa, da, lr_bytes(NNZ, R, U, opt, False)),
            "valued_generic": side(pb, cb, lr_bytes(NNZ, R, U, opt, True)),
            "note": "orientation only: different algorithms"}


def main():
    legs = ["k16_sgd", "k64_ftrl", "lr"]
    if "--leg" in sys.argv:
        i = sys.argv.index("--leg")
        legs = [sys.argv[i + 1]]
        assert legs[0] in ("k16_sgd", "k64_ftrl", "lr"), legs
        del sys.argv[i:i + 2]
    args = bench.parse_args()
    if not args.keys_per_gpu:
        args.keys_per_gpu = 10_000_000
    args.batches = min(args.batches, NB)
    from xflow_amd import capi
    capi.require_gpu()
    out = {"what": "feature values beside the binary paths, same minibatches, alternated"}
    if "k16_sgd" in legs:
        args.zipf = 0.0
        out["configs3_k16_sgd"] = fm_leg(args, 16, "sgd")
    if "k64_ftrl" in legs:
        args.zipf = 1.1
        out["k64_ftrl_zipf1.1"] = fm_leg(args, 64, "ftrl")
    if "lr" in legs:
        args.zipf = 0.0
        out["configs1_lr_ftrl"] = lr_leg(args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
