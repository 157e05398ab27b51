#!/usr/bin/env python3
"""Row normalisation measured on a GPU box: the stage's time on the rows of one 64 MiB text block
beside the same bytes streamed by xf_calib_stream, beside the cross and beside the valued key
build of the same block, in the same run.

    python tools/rownorm_leg.py OUT.jsonl [block_mb]

Two row shapes — click rows of 17 .. 39 tokens (one token per field, fields 0 .. 38 in order) and
bench-shaped rows of 200 tokens over 18 fields — on uniform and Zipf(1.1) keys over a key space of
1e7, as tools/cross_leg.py and tools/admit_leg.py build them.  Each block is tokenised on the GPU
with its fields and values (ingest=gpu_fields); one record per block.  Every figure is a host
clock around calls that end in a stream synchronise, in ms, the median of 5 unless it says
otherwise:
    norm             xf_rownorm_apply_dev of the block (no sums out) and a wait for it
    norm_sums        the same with the rows' sums of squares written (8 bytes per row more)
    bytes            what the kernel must move: 4 read + 4 written per nonzero, 4 per row of offsets
    norm_gbps        bytes / norm
    calib4 / calib16 xf_calib_stream reading bytes / 2 and writing bytes / 2, 4 and 16 B per lane
    cross            xf_cross_apply_dev of the block with its values (click rows: 4 pairs, one
                     crossed nonzero per pair and row; 200-token rows: 1 pair of multi-valued
                     fields), its own wait included
    key_build_first  xf_sharded_compile_valued_dev into an empty LR table (first-touch inserts)
    key_build_again  the same minibatch compiled again (every key in the table)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import K, block_text as bench_text, ms  # noqa: E402

CLICK_FIELDS = 39


def click_text(rng, nbytes, zipf):
    """rows of 17 .. 39 tokens, a row's fields 0, 1, ... in order"""
    rows = nbytes // (28 * 12) + 1
    lens = rng.randint(17, CLICK_FIELDS + 1, size=rows)
    n = int(lens.sum())
    fid = (np.minimum(rng.zipf(zipf, size=n), K) - 1) if zipf else rng.randint(0, K, size=n)
    lab = rng.randint(0, 2, size=rows)
    fid = fid.tolist()
    lines, size, at = [], 0, 0
    for r in range(rows):
        m = int(lens[r])
        line = ("%d\t" % lab[r] + " ".join("%d:%d:0.37" % (j, fid[at + j]) for j in range(m)) +
                "\n").encode()
        at += m
        if size + len(line) >= nbytes:
            break
        lines.append(line)
        size += len(line)
    return b"".join(lines)


def sync():
    capi.check(capi.lib().xf_stream_sync(None))


def key_build(args):
    st = capi.Sharded(model="lr", capacity=60_000_000)
    sync()
    t1, mb = ms(lambda: st.compile_valued_dev(*args))
    st.step(mb)
    st.check()
    t2, _ = ms(lambda: st.compile_valued_dev(*args), 5)
    st.close()
    return t1, t2


def leg(shape, name, zipf, block_mb):
    rng = np.random.RandomState(7)
    cap = block_mb << 20
    text = (click_text if shape == "click" else bench_text)(rng, cap, zipf)
    ing = capi.Ingest(cap).fields(fgid=True, values=True)
    ok, R, N, dk, dr, dl = ing.block_dev(text)
    assert ok
    dfg, dv = capi.vp(), capi.vp()
    capi.check(capi.lib().xf_ingest_fields(ing.h, capi.C.byref(dfg), capi.C.byref(dv)))
    assert dfg.value and dv.value
    n = capi.RowNorm()

    def norm(sums):
        out = n.norm_dev(dv.value, dr, R, N, want_sumsq=sums)
        sync()
        return out

    norm(False)                                           # (warm: the code object, the buffers)
    norm(True)
    t_norm, _ = ms(lambda: norm(False), 5)
    t_sums, _ = ms(lambda: norm(True), 5)
    assert n.stats() == (12 * R, 12 * R)
    nbytes = 8 * N + 4 * (R + 1)
    L = capi.lib()

    def calib(read, write):
        capi.check(L.xf_calib_stream(read, nbytes // 2, 1))
        capi.check(L.xf_calib_stream(write, nbytes // 2, 1))
        sync()

    calib(0, 3)
    calib(2, 5)
    t_c4, _ = ms(lambda: calib(0, 3), 5)
    t_c16, _ = ms(lambda: calib(2, 5), 5)
    pairs = [(2 * p, 2 * p + 1) for p in range(4 if shape == "click" else 1)]
    x = capi.Cross(pairs)

    def cross():
        out = x.cross_dev(dk, dr, R, N, dfg.value, d_vals=dv.value, want_fgid=False)
        sync()
        return out

    cross()
    t_cross, (_, _, total, _, _) = ms(cross, 5)
    first, again = key_build((dk, dv.value, dr, dl, R, N))
    return {"shape": shape, "stream": name, "block_bytes": len(text), "rows": R, "nnz": N,
            "norm_ms": t_norm, "norm_sums_ms": t_sums, "bytes": nbytes,
            "norm_gbps": nbytes / t_norm / 1e6, "calib4_ms": t_c4, "calib16_ms": t_c16,
            "norm_over_calib16": t_norm / t_c16, "cross_pairs": len(pairs), "cross_nnz_out": total,
            "cross_ms": t_cross, "key_build_first_ms": first, "key_build_again_ms": again}


if __name__ == "__main__":
    capi.require_gpu()
    block_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    with open(sys.argv[1], "a") as out:
        for shape in ("click", "rows200"):
            for name, zipf in (("uniform", None), ("zipf1.1", 1.1)):
                rec = leg(shape, name, zipf, block_mb)
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
