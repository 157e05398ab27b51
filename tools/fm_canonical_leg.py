#!/usr/bin/env python3
"""Experiment driver (GPU box): the FM step in both forms — the reference's pooled second-order
term and canonical FM (fm_mode=canonical) — on the same minibatches of bench.py's generator:
BASELINE configs[3] (FM k = 16 + SGD, 10^7 keys, the config-2 row shape) and k = 64 + FTRL on
the Zipf(1.1) stream.  Compiled minibatches replayed from HBM, device-event timing after a
warm-up, three repeats.  One JSON line: ms/step per form, examples/s, the canonical form's
algorithmic bytes and their fraction of 8 TB/s.  --leg k16_sgd | k64_ftrl runs one
configuration only (a profiler run per configuration).
  python tools/fm_canonical_leg.py [--leg L] [--rows R --nnz-per-row N --keys-per-gpu K]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def canonical_bytes(NNZ, R, U, k, opt):
    """NNZ (12 + 8k) + R (8 + 4k) + U (1 + k) x (32 FTRL | 16 SGD): the reference form's SURVEY
    8(d) count plus the S round trip (written once, read once per occurrence)"""
    return NNZ * (12 + 8 * k) + R * (8 + 4 * k) + (32 if opt == "ftrl" else 16) * U * (1 + k)


def time_mode(args, batches, k, opt, mode, nb=4, steps=12, repeats=3):
    import torch
    from xflow_amd.single import SingleGpuTrainer
    cap = int(args.keys_per_gpu / args.load_factor) + 1024
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
    NNZ = sum(c.NNZ for c in comp) / nb
    U = sum(c.U for c in comp) / nb
    ms = min(per)
    out = {"ms_per_step": ms, "ms_per_step_repeats": per, "examples_per_sec": R / (ms * 1e-3),
           "R": R, "NNZ": NNZ, "U": U}
    if mode == "canonical":
        b = canonical_bytes(NNZ, R, U, k, opt)
        out["algorithmic_bytes"] = b
        out["fraction_of_8TBps"] = b / (ms * 1e-3) / PEAK_BYTES_PER_S
    return out


def leg(args, k, opt):
    keytab = bench.make_key_table(args.keys_per_gpu)
    batches = bench.make_batches(args, 0, args.keys_per_gpu, keytab)
    res = {"k": k, "optimizer": opt, "zipf": args.zipf}
    for mode in ("reference", "canonical"):
        res[mode] = time_mode(args, batches, k, opt, mode)
    res["canonical_over_reference"] = res["canonical"]["ms_per_step"] / \
        res["reference"]["ms_per_step"]
    return res


def main():
    legs = ["k16_sgd", "k64_ftrl"]
    if "--leg" in sys.argv:
        i = sys.argv.index("--leg")
        legs = [sys.argv[i + 1]]
        assert legs[0] in ("k16_sgd", "k64_ftrl"), legs
        del sys.argv[i:i + 2]
    args = bench.parse_args()
    if not args.keys_per_gpu:
        args.keys_per_gpu = 10_000_000
    args.batches = min(args.batches, 4)
    from xflow_amd import capi
    capi.require_gpu()
    out = {"what": "FM step, reference vs canonical form, same minibatches"}
    if "k16_sgd" in legs:
        args.zipf = 0.0
        out["configs3_k16_sgd"] = leg(args, 16, "sgd")
    if "k64_ftrl" in legs:
        args.zipf = 1.1
        out["k64_ftrl_zipf1.1"] = leg(args, 64, "ftrl")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
