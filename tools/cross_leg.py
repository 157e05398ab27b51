#!/usr/bin/env python3
"""Feature crosses measured on a GPU box: the stage's time per 64 MiB text block of click-shaped
rows beside the same bytes streamed by xf_calib_stream and beside the key build of the crossed and
of the plain block.

    python tools/cross_leg.py OUT.jsonl [block_mb]

Per stream (uniform and Zipf(1.1) keys over a key space of 1e7) one block of 39-field rows, one
token per field, is drawn and tokenised on the GPU with its fields (ingest=gpu_fields).  Per spec of
1, 4 and 16 pairs — (0, 1), (2, 3), ...: every field in at most one pair, one crossed nonzero per
pair and row — one record.  Every figure is a host clock around calls that end in a stream
synchronise, in ms, the median of 5 unless it says otherwise:
    apply            xf_cross_apply_dev of the block, keys only (no values, no fgid out): count,
                     scan, the one wait, emit, and a wait for the emit
    apply_long       the same with xf_tune cross_short_max = 0: every row through the
                     workgroup-per-row emit (member lists in LDS) instead of the wave-per-row one
    bytes_in/out     what the two passes must move: fgid and rowptr for the count, keys, fgid and
                     rowptr for the emit, the row counts written and read; the crossed keys, rowptr
                     and the row counts written
    apply_gbps       (bytes_in + bytes_out) / apply
    calib            xf_calib_stream reading bytes_in and writing bytes_out, 16 B per lane
    key_build_first  xf_sharded_compile_dev into an empty LR table (first-touch inserts), one call
                     each for the plain and the crossed block, each on a table of its own
    key_build_again  the same minibatch compiled again (every key in the table)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xflow_amd import capi  # noqa: E402
from admit_leg import K, ms  # noqa: E402

FIELDS = 39


def block_text(rng, nbytes, zipf):
    """rows of one token per field, fields 0 .. 38 in order: Criteo-shaped click rows"""
    rows = nbytes // (FIELDS * 12) + 1
    n = rows * FIELDS
    fid = (np.minimum(rng.zipf(zipf, size=n), K) - 1) if zipf else rng.randint(0, K, size=n)
    lab = rng.randint(0, 2, size=rows)
    toks = ["%d:%d:0.37" % (j % FIELDS, f) for j, f in enumerate(fid.tolist())]
    lines, size = [], 0
    for r in range(rows):
        line = ("%d\t" % lab[r] + " ".join(toks[r * FIELDS:(r + 1) * FIELDS]) + "\n").encode()
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
    t1, mb = ms(lambda: st.compile_dev(*args))
    st.step(mb)
    st.check()
    t2, _ = ms(lambda: st.compile_dev(*args), 5)
    st.close()
    return t1, t2


def leg(name, zipf, block_mb):
    rng = np.random.RandomState(7)
    cap = block_mb << 20
    text = block_text(rng, cap, zipf)
    ing = capi.Ingest(cap).fields(fgid=True)
    ok, R, N, dk, dr, dl = ing.block_dev(text)
    assert ok
    dfg, dv = capi.vp(), capi.vp()
    capi.check(capi.lib().xf_ingest_fields(ing.h, capi.C.byref(dfg), capi.C.byref(dv)))
    assert dfg.value
    warm = capi.Sharded(model="lr", capacity=1 << 12)     # (the key build's code objects, 100 rows)
    warm.compile_dev(dk, dr, dl, min(R, 100), 100 * FIELDS if R >= 100 else 0)
    warm.close()
    plain_first, plain_again = key_build((dk, dr, dl, R, N))
    recs = []
    for npairs in (1, 4, 16):
        x = capi.Cross([(2 * p, 2 * p + 1) for p in range(npairs)])

        def apply():
            out = x.cross_dev(dk, dr, R, N, dfg.value, want_fgid=False)
            sync()                                        # (the emit follows the stage's own wait)
            return out

        apply()                                           # (warm: code objects, the buffers)
        t_apply, (ck, cr, total, _, _) = ms(apply, 5)
        capi.tune("cross_short_max", 0)
        try:
            apply()
            t_long, _ = ms(apply, 5)
        finally:
            capi.tune("cross_short_max", 64)
        apply()                                           # (the arrays of the default path again)
        bytes_in = N * 4 + N * 12 + 3 * R * 4 + R * 4
        bytes_out = total * 8 + 2 * R * 4
        L = capi.lib()

        def calib():
            capi.check(L.xf_calib_stream(2, bytes_in, 1))
            capi.check(L.xf_calib_stream(5, bytes_out, 1))
            sync()

        calib()
        t_calib, _ = ms(calib, 5)
        first, again = key_build((ck, cr, dl, R, total))
        recs.append({"stream": name, "block_bytes": len(text), "rows": R, "nnz": N,
                     "pairs": npairs, "nnz_out": total, "apply_ms": t_apply,
                     "apply_long_ms": t_long, "bytes_in": bytes_in, "bytes_out": bytes_out,
                     "apply_gbps": (bytes_in + bytes_out) / t_apply / 1e6, "calib_ms": t_calib,
                     "key_build_first_plain_ms": plain_first,
                     "key_build_again_plain_ms": plain_again,
                     "key_build_first_crossed_ms": first, "key_build_again_crossed_ms": again})
    return recs


if __name__ == "__main__":
    capi.require_gpu()
    block_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    with open(sys.argv[1], "a") as out:
        for name, zipf in (("uniform", None), ("zipf1.1", 1.1)):
            for rec in leg(name, zipf, block_mb):
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
