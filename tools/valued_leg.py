#!/usr/bin/env python3
"""Experiment driver (GPU box): feature values (feature_values=on) beside the binary paths, on
the same four minibatches of bench.py's generator, the two sides alternated within one call.
  * canonical FM — BASELINE configs[3] (k = 16 + SGD, 10^7 keys, the config-2 row shape) and
    k = 64 + FTRL on the Zipf(1.1) stream: the valued step against the binary canonical step.
    The valued step streams 8 NNZ more bytes (xval in the forward, coo_val in the gradient);
    the margin of the ratio is the spread of the binary figure over its five repeats.
  * the generic build (xf_batch_compile_dev) with and without values, same shapes: host clock
    around a call that ends in a stream wait.
  * valued LR at the configs[1] shape: the binary cells step, the generic valued path (sort-based
    generic build, Pull, gradient tiles: valued_lr = 1) and the local valued path (local build +
    valued cell kernels: valued_lr = 2) — steps by device events; builds, and a build plus one
    step of the fresh minibatch, by the host clock around calls that end in a stream wait.
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


class _Handle:
    """a minibatch handle the step functions take"""

    def __init__(self, h):
        self.h = h


def lr_build_and_once(batches, vals, tables, wss):
    """LR from device arrays, the generic valued build (xf_batch_compile_valued_dev) beside the
    local valued build (xf_batch_compile_local_valued_dev, retain_keys = 0) and the binary local
    build: ms per build, and ms per build + ONE step of the fresh minibatch (what a minibatch that
    is stepped once costs) — host clock, every timed call ends in a stream wait; the sides
    alternated, five repeats after a warm-up round.  tables / wss: per side, in steady state."""
    import ctypes as C
    import torch
    from xflow_amd import capi
    L = capi.lib()
    capi.tune("min_panel_nnz", 1e18)   # (as build_ms: the generic build without the panel view)
    names = ("binary_local", "valued_generic", "valued_local")
    dev = []
    for (rowptr, keys, labels), x in zip(batches[:NB], vals):
        dev.append((torch.from_numpy(keys.view(np.int64)).cuda(),
                    torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).cuda(),
                    torch.from_numpy(labels).cuda(), torch.from_numpy(x).cuda(),
                    len(labels), len(keys)))
    torch.cuda.synchronize()

    def compile_(name, d):
        dk, dr, dl, dv, R, NNZ = d
        h = capi.vp()
        if name == "valued_generic":
            capi.check(L.xf_batch_compile_valued_dev(C.byref(h), dk.data_ptr(), dv.data_ptr(),
                                                     dr.data_ptr(), dl.data_ptr(), R, NNZ, None))
        elif name == "valued_local":
            capi.check(L.xf_batch_compile_local_valued_dev(
                C.byref(h), tables[name].h, dk.data_ptr(), dv.data_ptr(), dr.data_ptr(),
                dl.data_ptr(), R, NNZ, 0, None))
        else:
            capi.check(L.xf_batch_compile_local_dev(C.byref(h), tables[name].h, dk.data_ptr(),
                                                    dr.data_ptr(), dl.data_ptr(), R, NNZ, 0, None))
        return h

    build = {n: [] for n in names}
    once = {n: [] for n in names}
    for rep in range(REPEATS + 1):
        for with_step, per in ((False, build), (True, once)):
            for name in names:
                t = 0.0
                for d in dev:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h = compile_(name, d)
                    if with_step:
                        capi.lr_step(tables[name], _Handle(h), wss[name])
                    torch.cuda.synchronize()
                    t += time.perf_counter() - t0
                    L.xf_batch_free(h)
                if rep:        # (the first round warms the builders' scratch up)
                    per[name].append(t / NB * 1e3)
    capi.tune("min_panel_nnz", 4e6)

    def fig(p):
        return {"ms": min(p), "ms_repeats": p, "spread": (max(p) - min(p)) / min(p)}
    out = {"build": {n: fig(p) for n, p in build.items()},
           "build_plus_one_step": {n: fig(p) for n, p in once.items()}}
    g, l = out["build_plus_one_step"]["valued_generic"], out["build_plus_one_step"]["valued_local"]
    # the rule of the by-shape default ("Feature values"): the local path for every
    # minibatch if it is not slower than the generic one, the generic figure's spread the margin
    out["stepped_once_local_over_generic"] = l["ms"] / g["ms"]
    out["stepped_once_margin_generic_spread"] = g["spread"]
    out["stepped_once_local_not_slower"] = l["ms"] <= g["ms"] * (1.0 + g["spread"])
    return out


def lr_leg(args, opt="ftrl"):
    """configs[1]: the binary cells step, the generic valued path (valued_lr = 1: the parent's
    code) and the local valued path (valued_lr = 2: valued cells), same minibatches, alternated"""
    from xflow_amd import capi
    from xflow_amd.single import SingleGpuTrainer
    keytab = bench.make_key_table(args.keys_per_gpu)
    batches = bench.make_batches(args, 0, args.keys_per_gpu, keytab)[:NB]
    vals = values_for(batches)
    cap = int(args.keys_per_gpu / args.load_factor) + 1024
    a = SingleGpuTrainer(model="lr", optimizer=opt, capacity=cap)
    b = SingleGpuTrainer(model="lr", optimizer=opt, capacity=cap, feature_values=True)
    c = SingleGpuTrainer(model="lr", optimizer=opt, capacity=cap, feature_values=True)
    ca = [a.compile(*m) for m in batches]
    try:
        capi.tune("valued_lr", 1)
        cb = [b.compile(*m, values=x) for m, x in zip(batches, vals)]
        capi.tune("valued_lr", 2)
        cc = [c.compile(*m, values=x) for m, x in zip(batches, vals)]
    finally:
        capi.tune("valued_lr", 0)
    assert all(x.U > 0 for x in cb) and all(x.cells_info()["segments"] == 1 for x in cc)
    prepare(a, ca)
    prepare(b, cb)
    prepare(c, cc)
    pa, pb, pc = timed((a, b, c), (ca, cb, cc))
    R, NNZ, U = (sum(getattr(x, n) for x in cb) / NB for n in ("R", "NNZ", "U"))

    class _Dims:   # (a cells minibatch has no key list: the generic one's dimensions)
        pass
    da = []
    for x in cb:
        d = _Dims()
        d.R, d.NNZ, d.U = x.R, x.NNZ, x.U
        da.append(d)
    res = {"optimizer": opt, "zipf": args.zipf,
           "binary_cells": side(pa, da, lr_bytes(NNZ, R, U, opt, False)),
           "valued_generic": side(pb, cb, lr_bytes(NNZ, R, U, opt, True)),
           "valued_cells": side(pc, da, lr_bytes(NNZ, R, U, opt, True)),
           "cells_info": cc[0].cells_info()}
    res["valued_cells_over_binary_cells"] = res["valued_cells"]["ms_per_step"] / \
        res["binary_cells"]["ms_per_step"]
    res["valued_generic_over_valued_cells"] = res["valued_generic"]["ms_per_step"] / \
        res["valued_cells"]["ms_per_step"]
    del ca, cb, cc
    res.update(lr_build_and_once(
        batches, vals, {"binary_local": a.w, "valued_generic": b.w, "valued_local": c.w},
        {"binary_local": a.ws, "valued_generic": b.ws, "valued_local": c.ws}))
    return res


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
