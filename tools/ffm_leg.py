#!/usr/bin/env python3
"""Experiment driver (GPU box): the field-aware FM step (fm_mode=field_aware) beside the canonical
step (fm_mode=canonical, the same k) on the same minibatches of bench.py's generator, in two
shapes: the sample files' (fields = 18, k = 4) and a Criteo-like one (fields = 39, k = 4).  A row
holds one nonzero per field (nnz per row = fields, nonzero j of a row under field j), the keys
uniform over --keys-per-gpu.  Compiled minibatches replayed from HBM, device-event timing after a
warm-up, three repeats.  One JSON line: ms/step per form, examples/s, pairs per row.
--leg f18_k4 | f39_k4 runs one shape only (a profiler run per shape: rocprofv3 --kernel-trace
--stats -- python tools/ffm_leg.py --leg ...).
  python tools/ffm_leg.py [--leg L] [--rows R --keys-per-gpu K --optimizer ftrl|sgd]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

LEGS = {"f18_k4": (18, 4), "f39_k4": (39, 4)}


def time_mode(args, batches, fields, k, opt, mode, nb=4, steps=12, repeats=3):
    import torch
    from xflow_amd.single import SingleGpuTrainer
    cap = int(args.keys_per_gpu / args.load_factor) + 1024
    if mode == "field_aware":
        tr = SingleGpuTrainer(model="fm", optimizer=opt, k=k, capacity=cap, fm_mode=mode,
                              fields=fields)
        fg = np.tile(np.arange(fields, dtype=np.int32), args.rows)
        comp = [tr.compile(*b, fgid=fg) for b in batches[:nb]]
    else:
        tr = SingleGpuTrainer(model="fm", optimizer=opt, k=k, capacity=cap, fm_mode=mode)
        comp = [tr.compile(*b) for b in batches[:nb]]
    for c in comp:
        tr.predict(c)          # every key in both tables before the clock starts
    tr.check()
    tr.defrag()
    for i in range(4):         # warm-up
        tr.step(comp[i % nb])
    tr.check()
    torch.cuda.synchronize()
    per = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            tr.step(comp[i % nb])
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / steps)
    tr.check()
    R = sum(c.R for c in comp) / nb
    ms = min(per)
    return {"ms_per_step": ms, "ms_per_step_repeats": per, "examples_per_sec": R / (ms * 1e-3),
            "R": R, "NNZ": sum(c.NNZ for c in comp) / nb, "U": sum(c.U for c in comp) / nb}


def leg(args, fields, k, opt):
    args.nnz_per_row = fields
    keytab = bench.make_key_table(args.keys_per_gpu)
    batches = bench.make_batches(args, 0, args.keys_per_gpu, keytab)
    res = {"fields": fields, "k": k, "optimizer": opt, "rows": args.rows,
           "pairs_per_row": fields * (fields - 1) // 2}
    for mode in ("canonical", "field_aware"):
        res[mode] = time_mode(args, batches, fields, k, opt, mode)
    res["field_aware_over_canonical"] = res["field_aware"]["ms_per_step"] / \
        res["canonical"]["ms_per_step"]
    return res


def main():
    legs = list(LEGS)
    if "--leg" in sys.argv:
        i = sys.argv.index("--leg")
        legs = [sys.argv[i + 1]]
        assert legs[0] in LEGS, legs
        del sys.argv[i:i + 2]
    args = bench.parse_args()
    if not args.keys_per_gpu:
        args.keys_per_gpu = 1_000_000
    args.batches = min(args.batches, 4)
    args.zipf = 0.0
    opt = args.optimizer or "ftrl"
    from xflow_amd import capi
    capi.require_gpu()
    out = {"what": "FM step, canonical vs field-aware form, same minibatches",
           "keys_per_gpu": args.keys_per_gpu}
    for name in legs:
        out[name] = leg(args, LEGS[name][0], LEGS[name][1], opt)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
