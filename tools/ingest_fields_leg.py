#!/usr/bin/env python3
"""The GPU tokeniser's field modes (xf_ingest_set_fields, ingest=gpu_fields) measured on a GPU box:
a bench-shaped libsvm file (200 tokens "fg:fid:0.37" per row, fg in [0, 18), key space 1e7).

    python tools/ingest_fields_leg.py gen DIR [rows]
        writes DIR/train-00000 and DIR/test-00000
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python tools/ingest_fields_leg.py kernel DIR [modes]
        the file's first 64 MiB block through k_tok_emit, 20 times in each of the modes (default
        "none,fg,val,fg+val": the four instantiations; "none" alone also runs against a library
        that has no field modes, XF_LIB=<its path>, e.g. a build of the parent commit) — the
        kernel stats name the instantiations
    python tools/ingest_fields_leg.py e2e DIR OUT.jsonl
        first-epoch examples/s of the xflow_lr binary, fresh process each: valued LR and
        field-aware FM (fields=18, k=4) under ingest=host and ingest=gpu_fields"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNZ, K, FIELDS = 200, 10_000_000, 18


def gen(d, rows):
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(0)
    chunk = 20000        # the text is generated once for this many rows and written out repeatedly
    for name, n in (("train-00000", rows), ("test-00000", min(rows // 10, 20000))):
        m = min(n, chunk)
        fid = rng.randint(0, K, size=(m, NNZ))
        val = rng.randint(0, 100, size=(m, NNZ))
        lab = rng.randint(0, 2, size=m)
        lines = ["%d\t" % lab[r] + " ".join("%d:%d:0.%02d" % (j % FIELDS, fid[r, j], val[r, j])
                                            for j in range(NNZ)) + "\n" for r in range(m)]
        with open(os.path.join(d, name), "w") as f:
            left = n
            while left > 0:
                f.write("".join(lines[:min(left, m)]))
                left -= m
    print("generated %d rows, %.0f MB" % (rows, os.path.getsize(os.path.join(d, "train-00000")) / 1e6))


def kernel(d, modes):
    """raw ctypes, so that a library without the field modes can be driven too"""
    L = C.CDLL(os.environ.get("XF_LIB") or os.path.join(ROOT, "xflow_amd", "lib", "libxflow_amd.so"))
    L.xf_last_error.restype = C.c_char_p
    cap = 64 << 20
    with open(os.path.join(d, "train-00000"), "rb") as f:
        text = f.read(cap - 1)
    text = text[:text.rindex(b"\n") + 1]
    g = C.c_void_p()

    def check(rc):
        if rc:
            raise SystemExit("error %d: %s" % (rc, L.xf_last_error().decode()))
    check(L.xf_ingest_create(C.byref(g), C.c_size_t(cap)))
    rows, nnz, ok = C.c_uint32(), C.c_uint32(), C.c_int()
    for mode in modes:
        if mode != "none" or hasattr(L, "xf_ingest_set_fields"):
            check(L.xf_ingest_set_fields(g, int("fg" in mode), int("val" in mode)))
        t0 = time.time()
        for _ in range(20):
            check(L.xf_ingest_block(g, text, C.c_size_t(len(text)), None, None, None, None,
                                    C.byref(rows), C.byref(nnz), C.byref(ok)))
            assert ok.value == 1, "the block was handed back"
        print(json.dumps({"mode": mode, "text_bytes": len(text), "rows": rows.value,
                          "nnz": nnz.value, "ms_per_block_with_upload": (time.time() - t0) / 20 * 1e3}))
    check(L.xf_ingest_destroy(g))


def e2e(d, out_path):
    legs = {"lr_values": ["0", "1", "feature_values=on"],
            "field_aware": ["1", "1", "fm_mode=field_aware", "fields=%d" % FIELDS, "k=4"]}
    rows = sum(1 for _ in open(os.path.join(d, "train-00000"), "rb"))
    with open(out_path, "a") as out:
        for leg, args in legs.items():
            for ingest in ("host", "gpu_fields", "host", "gpu_fields"):     # (two runs of each)
                t0 = time.time()
                p = subprocess.run([os.path.join(ROOT, "xflow_amd/lib/xflow_lr"), os.path.join(d, "train"),
                                    os.path.join(d, "test")] + args +
                                   ["block_size_mb=64", "capacity=30000000", "ingest=" + ingest,
                                    "pred_path=" + os.path.join(d, "pred.txt")],
                                   capture_output=True, text=True, timeout=280,
                                   env=dict(os.environ, XF_TRACE_WORKER="1"))
                m = re.search(r"examples/sec \(train loop\): ([0-9.e+]+)", p.stdout)
                blocks = re.search(r"\((\d+) tokenised on the GPU, (\d+) parsed on the host\)", p.stderr)
                rec = {"leg": leg, "ingest": ingest, "rows": rows, "rc": p.returncode,
                       "first_epoch_examples_per_sec": float(m.group(1)) if m else None,
                       "blocks_gpu_host": [int(x) for x in blocks.groups()] if blocks else None,
                       "wall_seconds_incl_predict": time.time() - t0}
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                if p.returncode != 0:      # (nothing more is started on the GPU after a failure)
                    print(p.stdout[-2000:], p.stderr[-2000:])
                    raise SystemExit(1)


if __name__ == "__main__":
    what, d = sys.argv[1], sys.argv[2]
    if what == "gen":
        gen(d, int(sys.argv[3]) if len(sys.argv) > 3 else 120000)
    elif what == "kernel":
        kernel(d, (sys.argv[3] if len(sys.argv) > 3 else "none,fg,val,fg+val").split(","))
    else:
        e2e(d, sys.argv[3])
