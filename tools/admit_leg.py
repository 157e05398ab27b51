#!/usr/bin/env python3
"""Feature admission measured on a GPU box: the filter's time per 64 MiB text block beside the
tokeniser and the key build of the same block, on a uniform and on a Zipf(1.1) key stream
(bench-shaped rows: 200 tokens "fg:fid:0.37", key space 1e7).

    python tools/admit_leg.py OUT.jsonl [block_mb]

Per stream two blocks A and B are drawn.  Every figure is a host clock around a call that ends in
a stream synchronise (xf_ingest_block, xf_admit_apply_dev and xf_sharded_compile_dev all wait),
in ms:
    tokenise        xf_ingest_block of B from the staging buffer (upload + kernels), median of 5
    admit_fresh     the filter's first call: block A into zeroed counters (every nonzero a CAS)
    admit_next      block B on the filter that has seen A (what a stream's next block costs)
    admit_repeat    block B again, median of 5 (every counter it touches saturated or counted)
    admit_readonly  block B with update = 0 (predict), median of 5
    key_build_first xf_sharded_compile_dev of B into an empty LR table (first-touch inserts)
    key_build_again the same minibatch compiled again (every key in the table), median of 5
The filter is the worker's default: 2^26 counters, 3 hashes; admit_count = 2.
A shared filter (xf_admit_create_shared) on a group of ONE runs beside the plain one on the same
two blocks: routing, count-by-slot, answer and test-from-answers with every slot staying on the
rank — what the shared path costs before any transport (`shared_transport` says how the group
moved the rank's slice to itself: 0 RCCL — a copy on the device —, 1 staged through the host):
    plain_next5 / shared_next5          block B on a filter that has seen A, median over 5 filters
    plain_readonly / shared_readonly    block B with update = 0, median of 5"""
import ctypes as C
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xflow_amd import capi  # noqa: E402

NNZ, K, FIELDS = 200, 10_000_000, 18


def block_text(rng, nbytes, zipf):
    rows = nbytes // (NNZ * 13) + 1
    n = rows * NNZ
    fid = (np.minimum(rng.zipf(zipf, size=n), K) - 1) if zipf else rng.randint(0, K, size=n)
    lab = rng.randint(0, 2, size=rows)
    toks = ["%d:%d:0.37" % (j % FIELDS, f) for j, f in enumerate(fid.tolist())]
    lines, size = [], 0
    for r in range(rows):
        line = ("%d\t" % lab[r] + " ".join(toks[r * NNZ:(r + 1) * NNZ]) + "\n").encode()
        if size + len(line) >= nbytes:
            break
        lines.append(line)
        size += len(line)
    return b"".join(lines)


def staged_block(ing, text):
    """xf_ingest_block on text that lies in the tokeniser's pinned staging buffer, as the worker's
    staging thread leaves it (Ingest.block_dev copies the text there first, inside the call)"""
    L = capi.lib()
    buf, cap = capi.vp(), C.c_size_t()
    capi.check(L.xf_ingest_staging(ing.h, C.byref(buf), C.byref(cap)))
    if not getattr(ing, "_staged", None) == len(text):
        C.memmove(buf.value, text, len(text))
        ing._staged = len(text)
    dk, dr, dl = capi.vp(), capi.vp(), capi.vp()
    rows, nnz, ok = C.c_uint32(), C.c_uint32(), C.c_int()
    capi.check(L.xf_ingest_block(ing.h, None, len(text), None, C.byref(dk), C.byref(dr),
                                 C.byref(dl), C.byref(rows), C.byref(nnz), C.byref(ok)))
    return bool(ok.value), rows.value, nnz.value, dk.value, dr.value, dl.value


def ms(fn, repeat=1):
    out = []
    for _ in range(repeat):
        capi.check(capi.lib().xf_stream_sync(None))
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), r


def next_block(make, a_args, b_args):
    """median over five fresh filters of: block B on a filter that has seen block A; the last
    filter and its result come back for the read-only call"""
    out = []
    for _ in range(5):
        flt = make()
        flt.filter_dev(*a_args)
        t, r = ms(lambda: flt.filter_dev(*b_args))
        out.append(t)
    return statistics.median(out), flt, r


def group_of_one():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    # (RCCL when it comes up: the rank's slice to itself is then a copy on the device)
    return capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_AUTO, device=-1)


def leg(name, zipf, block_mb, group):
    rng = np.random.RandomState(7)
    cap = block_mb << 20
    a, b = block_text(rng, cap, zipf), block_text(rng, cap, zipf)
    ing_a, ing_b = capi.Ingest(cap), capi.Ingest(cap)
    ok, Ra, Na, ka, ra, la = ing_a.block_dev(a)
    assert ok
    ing_b.block_dev(b)                                   # (warm: code objects, first launches)
    t_tok, (ok, Rb, Nb, kb, rb, lb) = ms(lambda: staged_block(ing_b, b), 5)
    assert ok
    capi.Admit(10, 2).filter_dev(kb, rb, Rb, Nb)          # (warm, on a filter of its own)
    flt = capi.Admit(26, 2)
    t_fresh, ra_out = ms(lambda: flt.filter_dev(ka, ra, Ra, Na))
    t_next, rb_out = ms(lambda: flt.filter_dev(kb, rb, Rb, Nb))
    t_rep, rb_rep = ms(lambda: flt.filter_dev(kb, rb, Rb, Nb), 5)
    t_ro, _ = ms(lambda: flt.filter_dev(kb, rb, Rb, Nb, update=False), 5)
    # the shared filter on a group of one beside the plain one
    capi.Admit(10, 2, group=group).filter_dev(kb, rb, Rb, Nb)          # (warm)
    A_, B_ = (ka, ra, Ra, Na), (kb, rb, Rb, Nb)
    t_pn, _, kept_p = next_block(lambda: capi.Admit(26, 2), A_, B_)
    t_sn, sh, kept_s = next_block(lambda: capi.Admit(26, 2, group=group), A_, B_)
    assert kept_p[2] == kept_s[2] == rb_out[2]
    t_sro, _ = ms(lambda: sh.filter_dev(kb, rb, Rb, Nb, update=False), 5)
    del sh
    warm = capi.Sharded(model="lr", capacity=1 << 12)
    warm.compile_dev(ka, ra, la, min(Ra, 100), 100 * NNZ if Ra >= 100 else 0)
    st = capi.Sharded(model="lr", capacity=30_000_000)
    t_kb1, mb = ms(lambda: st.compile_dev(kb, rb, lb, Rb, Nb))
    st.step(mb)
    st.check()
    t_kb2, _ = ms(lambda: st.compile_dev(kb, rb, lb, Rb, Nb), 5)
    return {"stream": name, "block_bytes": len(b), "rows": Rb, "nnz": Nb,
            "kept_fresh": ra_out[2], "nnz_a": Na, "kept_next": rb_out[2], "kept_repeat": rb_rep[2],
            "tokenise_ms": t_tok, "admit_fresh_ms": t_fresh, "admit_next_ms": t_next,
            "admit_repeat_ms": t_rep, "admit_readonly_ms": t_ro, "key_build_first_ms": t_kb1,
            "key_build_again_ms": t_kb2, "plain_next5_ms": t_pn, "shared_next5_ms": t_sn,
            "plain_readonly_ms": t_ro, "shared_readonly_ms": t_sro,
            "shared_transport": group.transport}


if __name__ == "__main__":
    capi.require_gpu()
    block_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    group = group_of_one()
    with open(sys.argv[1], "a") as out:
        for name, zipf in (("uniform", None), ("zipf1.1", 1.1)):
            rec = leg(name, zipf, block_mb, group)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
