"""One admission filter shared by the ranks of a group, on the GPU (xf_admit_create_shared).  The
ranks are spawned processes on one GPU over the host transport (tests/test_gpu_sharded_modes.py's
discipline: at most three, the parent waits for each with a timeout, nothing is retried).  After
every apply each rank dumps its range of the counters and its filtered arrays; the parent judges
them bit for bit against tests/_admit_shared_checker.py — ONE restated filter counting the
concatenation of the ranks' minibatches.  Then: the counters do not depend on the world size, the
counter file moves between world sizes, a bad apply fails on every rank, and the worker end to end
(scripts/local.sh 2 2 xflow_lr ... admit_shared=1) against the restatement feeding the oracle's
rank-ordered schedule."""
import multiprocessing as mp
import os
import re
import subprocess
import traceback

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi

from . import _admit_checker as A
from . import _admit_shared_checker as S
from .test_gpu_admit import same, zipf_text
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu

_TIMEOUT = 150      # seconds the parent waits for a rank's report
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(build.LIBDIR, "xflow_lr")
GRID = [(world, N, h, L) for world in (1, 2, 3) for N in (1, 2, 255) for h in (1, 3) for L in (2, 10)]
STREAM = (10, 2, 3)                 # L, N, h of the filter that takes S.global_stream()


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def _spawn(target, argsets):
    """one process per argument set; the parent waits for each report with a timeout and fails on
    the first error (the others are ended: a rank whose peer has failed waits in a collective)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=target, args=a + (q,)) for a in argsets]
    for p in ps:
        p.start()
    try:
        res = []
        for _ in ps:
            r = q.get(timeout=_TIMEOUT)     # (rank, None or what it found | a traceback)
            assert not isinstance(r[1], str), r[1]
            res.append(r)
        for p in ps:
            p.join(timeout=60)
        return res
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)


def _group(rank, world, port):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)


def _apply(a, mb, t, update, out, tag):
    """one apply of this rank's minibatch; the filtered arrays and the range go to out[tag_*]"""
    rp, ks = mb
    fg, vs = S.companions(ks, t)
    got = list(a.apply(rp, ks, fgid=fg, values=vs, update=update))
    out[tag + "_rp"], out[tag + "_keys"] = got[0], got[1]
    if fg is not None:
        out[tag + "_fgid"] = got[2]
    if vs is not None:
        out[tag + "_vals"] = got[-1]
    out[tag + "_ctr"] = a.export()


def _stream(a, world, rank):
    for mb in S.global_stream():
        a.apply(*S.deal(mb, world)[rank])


# ------------------------------------------------------------------ 1. the grid
def _grid_rank(rank, world, port, outdir, q):
    try:
        g = _group(rank, world, port)
        for N, h, L in sorted({p[1:] for p in GRID}):
            a = capi.Admit(L, N, h, S.SEED, group=g)
            assert (a.first_slot, a.n_slots) == S.admit_range(L, world, rank)
            out = {}
            for t, (name, update, parts) in enumerate(S.sequence(world, N, h, L)):
                _apply(a, parts[rank], t, update, out, "t%d" % t)
            out["stats"] = np.array(a.stats(), np.int64)
            np.savez(os.path.join(outdir, "w%d_N%d_h%d_L%d_rank%d.npz" % (world, N, h, L, rank)), **out)
            del a
        # the same global stream on this world size
        L, N, h = STREAM
        a = capi.Admit(L, N, h, S.SEED, group=g)
        _stream(a, world, rank)
        out = {"ctr": a.export()}
        if world == 3:          # the counter file: saved by three ranks, and a one-worker file loaded
            a.save(os.path.join(outdir, "by3.admit"))
            b = capi.Admit(L, N, h, S.SEED, group=g)
            b.load(os.path.join(outdir, "plain.admit"))
            out["loaded"] = b.export()
            c = capi.Admit(L, N + 1, h, S.SEED, group=g)
            try:
                c.load(os.path.join(outdir, "plain.admit"))
                out["other_params"] = np.array("loaded")
            except capi.XFError as e:
                out["other_params"] = np.array(str(e))
            del b, c
        np.savez(os.path.join(outdir, "w%d_stream_rank%d.npz" % (world, rank)), **out)
        g.barrier()
        del a
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


_runs = {}


@pytest.fixture(scope="module")
def outdir(tmp_path_factory):
    return tmp_path_factory.mktemp("admit_shared")


def run_world(outdir, world):
    """every grid point and the global stream on `world` ranks, once; the ranks' dumps"""
    if world not in _runs:
        if world == 3:          # the file of a plain one-worker filter after the same stream
            L, N, h = STREAM
            p = capi.Admit(L, N, h, S.SEED)
            for mb in S.global_stream():
                p.apply(*mb)
            p.save(str(outdir / "plain.admit"))
            _runs["plain"] = p.export()
        port = free_port()
        _spawn(_grid_rank, [(r, world, port, str(outdir)) for r in range(world)])
        _runs[world] = True
    return lambda name, r: np.load(str(outdir / ("w%d_%s_rank%d.npz" % (world, name, r))))


@pytest.mark.parametrize("world,N,h,L", GRID, ids=["w%d-N%d-h%d-L%d" % g for g in GRID])
def test_counters_and_filtered_arrays(outdir, world, N, h, L):
    dump = run_world(outdir, world)
    got = [dump("N%d_h%d_L%d" % (N, h, L), r) for r in range(world)]
    seq = S.sequence(world, N, h, L)
    seen, kept = [0] * world, [0] * world
    for t, ((name, update, parts), (ctr, ranks)) in enumerate(zip(seq, S.expected(seq, N, h, L))):
        tag = "t%d_" % t
        for r in range(world):
            first, n = S.admit_range(L, world, r)
            assert got[r][tag + "ctr"].shape == (n,), (name, r)
            rp, ks, fg, vs, keep = ranks[r]
            same(got[r][tag + "rp"], rp)
            same(got[r][tag + "keys"], ks)
            assert (tag + "fgid" in got[r]) == (fg is not None)
            assert (tag + "vals" in got[r]) == (vs is not None)
            if fg is not None:
                same(got[r][tag + "fgid"], fg)
            if vs is not None:
                same(got[r][tag + "vals"], vs)
            if N == 1 and update:                                # the identity on every rank
                same(got[r][tag + "rp"], parts[r][0].astype(np.uint32))
                same(got[r][tag + "keys"], parts[r][1])
            if update:
                seen[r] += len(parts[r][1])
                kept[r] += int(keep.sum())
        same(np.concatenate([got[r][tag + "ctr"] for r in range(world)]), ctr)
    for r in range(world):                                       # stats stay per rank
        assert tuple(got[r]["stats"]) == (seen[r], kept[r])


# ------------------------------------------------------------------ 2. world independence, files
def test_the_counters_do_not_depend_on_the_world_size(outdir):
    L, N, h = STREAM
    flt = A.Filter(L, N, h, S.SEED)
    for _, ks in S.global_stream():
        flt.count(ks)
    assert 0 < (flt.c == N).sum() < 1 << L
    for world in (1, 2, 3):
        dump = run_world(outdir, world)
        same(np.concatenate([dump("stream", r)["ctr"] for r in range(world)]), flt.c)


def test_the_counter_file_moves_between_world_sizes(outdir):
    dump = run_world(outdir, 3)
    plain = _runs["plain"]
    by3 = open(str(outdir / "by3.admit"), "rb").read()
    assert by3 == open(str(outdir / "plain.admit"), "rb").read()
    L, N, h = STREAM
    one = capi.Admit(L, N, h, S.SEED)
    one.load(str(outdir / "by3.admit"))                          # three ranks -> one worker
    same(one.export(), plain)
    same(np.concatenate([dump("stream", r)["loaded"] for r in range(3)]), plain)   # ... and back
    for r in range(3):
        assert "was saved with" in str(dump("stream", r)["other_params"])


# ------------------------------------------------------------------ 3. errors
def _error_rank(rank, port, outdir, q):
    try:
        g = _group(rank, 2, port)
        a = capi.Admit(10, 2, 3, S.SEED, group=g)
        rng = np.random.RandomState(rank)
        keys = S.pool()[rng.randint(0, 3000, size=600)]
        rowptr = np.arange(0, 601, 6, dtype=np.uint64)
        msgs = []

        def refused(f):
            try:
                f()
                msgs.append("")
            except capi.XFError as e:
                msgs.append(str(e))

        refused(lambda: a.apply(rowptr, keys, update=rank == 0))        # the flags differ
        bad = rowptr.copy()
        if rank == 1:
            bad[3], bad[4] = bad[4], bad[3]                             # offsets descend on rank 1
        refused(lambda: a.apply(bad, keys))
        d = a.apply_dev(rowptr, keys, update=False)                     # (device arrays to point at)
        # 2^31 nonzeros x 3 hashes cannot be routed: refused before anything is read
        refused(lambda: a.filter_dev(d.d_keys, d.d_rowptr, d.R if rank else 1,
                                     d.NNZ if rank else 1 << 31, update=False))
        # ... and the ranks are still in step: nothing was counted so far, a good apply counts
        assert not a.export().any()
        rp, ks = a.apply(rowptr, keys)
        np.savez(os.path.join(outdir, "err_rank%d.npz" % rank), rp=rp, keys=ks, ctr=a.export(),
                 inkeys=keys)
        g.barrier()
        del a
        g.close()
        q.put((rank, msgs))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_a_bad_apply_fails_on_every_rank(outdir):
    port = free_port()
    res = dict(_spawn(_error_rank, [(r, port, str(outdir)) for r in range(2)]))
    for r in range(2):
        flags, args, big = res[r]
        assert re.search(r"rank 1 passes update=0, rank 0 update=1", flags), flags
        assert re.search(r"rank 1 failed its argument checks", args), args
        assert re.search(r"rank 0 failed its argument checks", big), big
    assert "row offsets descend" in res[1][1] and "2^32" in res[0][2]
    got = [np.load(str(outdir / ("err_rank%d.npz" % r))) for r in range(2)]
    flt = A.Filter(10, 2, 3, S.SEED)
    flt.count(np.concatenate([g["inkeys"] for g in got]))
    same(np.concatenate([g["ctr"] for g in got]), flt.c)
    for g in got:
        same(g["keys"], g["inkeys"][flt.keep_mask(g["inkeys"])])


# ------------------------------------------------------------------ 4. the worker, end to end
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("admit_shared_e2e")
    for r, (seed, nbytes) in enumerate(((25, (2 << 20) + (200 << 10)), (26, (1 << 20) + (200 << 10)))):
        (d / ("train-%05d" % r)).write_bytes(zipf_text(seed, nbytes))
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10))
    return d


_refs = {}


def reference(data, recount):
    """the restatement feeding the oracle's rank-ordered schedule: a turn is one block of every
    rank that still has one, counted together and filtered rank by rank; both ranks pull, then push
    in rank order; the second epoch replays the admitted minibatches (recount: filters again)"""
    if recount in _refs:
        return _refs[recount]
    flt = A.Filter(12, 2, 3, 0)                                  # the worker's seed: 0
    blocks = [list(capi.read_blocks(str(data / ("train-%05d" % r)), 1 << 20)) for r in range(2)]
    assert [len(b) for b in blocks] == [3, 2]                    # rank 1's last turn is empty
    stats = [[0, 0], [0, 0]]

    def turn(t):
        mine = [blocks[r][t] if t < len(blocks[r]) else None for r in range(2)]
        flt.count(np.concatenate([b[1] for b in mine if b is not None]))
        out = []
        for r, b in enumerate(mine):
            if b is None:
                out.append(None)
                continue
            rp, keys, labels = b[0], b[1], b[3]
            keep = flt.keep_mask(keys)
            before = np.concatenate([[0], np.cumsum(keep)])
            stats[r][0] += len(keys)
            stats[r][1] += int(keep.sum())
            out.append((before[rp.astype(np.int64)].astype(np.uint64), keys[keep], labels))
        return out

    with O.sum_mode(1):
        s = O.Store(O.OPT_FTRL, 1)
        s.push(np.array([0], np.uint64), np.zeros(1, np.float32))
        first = None
        for epoch in range(2):
            turns = [turn(t) for t in range(3)] if epoch == 0 or recount else first
            first = first or turns
            if epoch == 0:                                       # worth running: kept AND dropped
                assert all(0 < len(mb[1]) < len(blocks[r][t][1])
                           for t, tn in enumerate(turns) for r, mb in enumerate(tn) if mb is not None)
            for tn in turns:
                obs = [O.Batch(*mb) for mb in tn if mb is not None and len(mb[1])]
                pulled = [s.pull(ob.ukeys) for ob in obs]
                grads = [ob.lr_grad(ob.lr_loss(pw)[0]) for ob, pw in zip(obs, pulled)]
                for ob, g in zip(obs, grads):
                    s.push(ob.ukeys, g)
        labs, ps = [], []
        for blk in capi.read_blocks(str(data / "test-00000"), 4 << 20):
            rp, keys, labels = blk[0], blk[1], blk[3]
            keep = flt.keep_mask(keys)
            assert not keep.all()                                # the test file's unseen keys
            before = np.concatenate([[0], np.cumsum(keep)])
            b = O.Batch(before[rp.astype(np.int64)].astype(np.uint64), keys[keep], labels)
            ps.append(b.lr_loss(s.pull(b.ukeys))[1])
            labs.append(labels)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    _refs[recount] = (s, lab, p, O.auc_logloss(lab, p), stats, flt.c.copy())
    return _refs[recount]


def local_sh(data, tmp_path, epochs, *extra):
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          str(data / "train"), str(data / "test"), "0", str(epochs),
                          "transport=host", "block_size_mb=1", "capacity=16384", "admit_count=2",
                          "admit_shared=1", "admit_log2_slots=12", *extra],
                         capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def check_run(lines, pred, ckpt, ref, trained=True):
    s, lab, p, (ll, auc, tp, fp), stats, ctr = ref
    assert O.format_auc_line(ll, auc, tp, fp) in lines, lines
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    want = sorted("rank %d admit_seen = %d admit_kept = %d" % (r, *(stats[r] if trained else (0, 0)))
                  for r in range(2))
    assert sorted(ln for ln in lines if "admit_seen" in ln) == want
    if ckpt:
        one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 15)
        one.load(ckpt)                                           # two shard files -> one table
        for a, e in zip(one.w.export(), s.export()):
            same(a, e)
        saved = capi.Admit(12, 2)
        saved.load(ckpt + ".admit")                              # written by two ranks
        same(saved.export(), ctr)


@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_local_sh_two_workers_share_one_filter(data, tmp_path, ingest):
    ref = reference(data, False)
    ckpt, pred = str(tmp_path / "model"), str(tmp_path / "pred.txt")
    lines = local_sh(data, tmp_path, 2, "ingest=" + ingest, "model_out=" + ckpt, "pred_path=" + pred)
    check_run(lines, pred, ckpt, ref)
    if ingest == "host":                                         # the model file round trip
        pred2 = str(tmp_path / "pred2.txt")
        lines = local_sh(data, tmp_path, 0, "model_in=" + ckpt, "pred_path=" + pred2)
        check_run(lines, pred2, None, ref, trained=False)


def test_local_sh_counts_again_without_the_batch_cache(data, tmp_path):
    ref = reference(data, True)
    assert ref[4] != reference(data, False)[4]                   # (twice the nonzeros were seen)
    ckpt, pred = str(tmp_path / "model"), str(tmp_path / "pred.txt")
    lines = local_sh(data, tmp_path, 2, "ingest=gpu", "cache_batches=0", "model_out=" + ckpt,
                     "pred_path=" + pred)
    check_run(lines, pred, ckpt, ref)
