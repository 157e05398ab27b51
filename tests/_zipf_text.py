"""The generated click-data text of the worker tests (tests/test_gpu_negsample.py,
tests/test_gpu_evict_replay.py, tests/test_evict_cpu.py): here, because those files need a GPU to
import and the CPU tests form the same text."""
import numpy as np

FIELDS = 18          # tests/test_gpu_admit.py's FIELDS


def zipf_text(seed, nbytes, positives=0.05):
    """tests/test_gpu_admit.py's zipf_text with the share of positive rows as a parameter: click
    data — field0 in [0, FIELDS), values of a few digits, 300 hot fids (Zipf 1.1) and, one token in
    a thousand, a fid from a large space"""
    rng = np.random.RandomState(seed)
    vals = ["1", "0.5", "2", "-1.25", "0.25", "3.5", "-0.75", "", "0.125", "1.5"]
    rows = nbytes // 30 + 1
    ntok = rng.randint(3, 15, size=rows)
    n = int(ntok.sum())
    p = 1.0 / np.arange(1, 301) ** 1.1
    fid = rng.choice(300, size=n, p=p / p.sum())
    rare = rng.rand(n) < 0.001
    fid[rare] = 1000 + rng.randint(0, 400, size=int(rare.sum())) * 7 + seed % 7 * 3000
    f, vi = rng.randint(0, FIELDS, size=n), rng.randint(0, len(vals), size=n)
    lab = rng.rand(rows) < positives
    toks = ["%d:%d:%s" % (f[i], fid[i], vals[vi[i]]) for i in range(n)]
    lines, size, at = [], 0, 0
    for r in range(rows):
        if size >= nbytes:
            break
        line = ("%d\t" % lab[r] + " ".join(toks[at:at + ntok[r]]) + "\n").encode()
        at += ntok[r]
        lines.append(line)
        size += len(line)
    return b"".join(lines)
