"""The order of the worker's stages between a block's rows and its minibatch — ingest, split,
negsample, slices, cross, admission, row norm, compile — with every stage on at once, on a real
MI355X.  Every comparison is exact (bytes): the two doors into the chain (host arrays through the
first stage's upload, the tokeniser's device arrays) against each other, the run with the split
against the run on the split's kept file, each stage as the first one on, and a block that loses
every row.  The training file is read in three blocks, the last one partial: the running counts
(the rows read, the rows of the train part) only matter across blocks."""
import numpy as np
import pytest

from xflow_amd import capi

from . import _holdout_checker as H
from . import _negsample_checker as N
from . import _zipf_text as Z

pytestmark = pytest.mark.gpu

EPOCHS = 2
SHARE = 0.25
KEEP = 0.5
ADMIT = dict(admit_count=2, admit_log2_slots=16, admit_hashes=3)
SPLIT = dict(holdout=SHARE, holdout_by=7)
REST = dict(neg_keep=KEEP, progress=1, progress_by=5, cross="2*3", row_norm="l2",
            feature_values="on", **ADMIT)
PRINTED = ("progress epoch ", "progress slices epoch ", "  key = ", "holdout epoch ",
           "holdout groups epoch ")
PROGRESS = ["progress_" + n for n in ("logloss", "auc", "auc_slack", "ctr", "pctr", "rows",
                                      "logloss_first", "auc_first")]
SLICES = ["slices", "slice_rows", "slice_none_rows", "slice_overflow_rows"]
HOLDOUT = ["holdout_" + n for n in ("rows", "logloss", "auc", "auc_slack", "ctr", "pctr",
                                    "logloss_first", "best_epoch", "best_logloss")]
GAUC = ["holdout_" + n for n in ("gauc", "gauc_slack", "macro_auc", "groups", "groups_scored",
                                 "gauc_rows")]
COUNTS = ["rows_trained", "rows_kept", "neg_seen", "neg_kept", "admit_seen", "admit_kept",
          "cross_in", "cross_out", "norm_rows", "norm_rows_scaled", "keys"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def labels_of(path):
    return np.array([ln[:1] == b"1" for ln in open(path, "rb").read().split(b"\n")[:-1]])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """train-00000: generated click text with field ids and values, three 1 MiB blocks, the last
    one partial; kept-00000: the rows the split does not hold, written by the holdout checker;
    test-00000: a few thousand rows"""
    d = tmp_path_factory.mktemp("stage_order")
    (d / "train-00000").write_bytes(Z.zipf_text(61, (2 << 20) + (300 << 10), positives=0.2))
    (d / "test-00000").write_bytes(Z.zipf_text(62, 250000, positives=0.3))
    blocks = list(capi.read_blocks(str(d / "train-00000"), 1 << 20))
    assert len(blocks) == 3 and len(blocks[2][3]) < len(blocks[1][3]) // 2
    m = H.write_split(str(d / "train-00000"), str(d / "kept-00000"), str(d / "held"), 0, 0, SHARE)
    assert len(m) == sum(len(b[3]) for b in blocks) and len(m) // 8 < int(m.sum()) < len(m) // 2
    assert len(labels_of(str(d / "test-00000"))) > 2000
    return d


def bits(v):
    return np.float64(v).tobytes()


def run(data, tag, capfd, metrics, train="train", **params):
    """-> what a run leaves behind, as bytes: the exported table, the prediction file, the printed
    lines of the stages and the named metrics"""
    pred = str(data / ("pred_%s.txt" % tag))
    p = dict(block_size_mb=1, capacity=1 << 18, epochs=EPOCHS, pred_path=pred)
    p.update(params)
    capfd.readouterr()
    x = capi.XFlow(str(data / train), str(data / "test"), **p)
    x.train()
    printed = capfd.readouterr().out
    keys, w, n, z = capi.Table.from_handle(x.tables()[0], 1, capi.OPT_FTRL).export()[:4]
    order = np.argsort(keys)
    return dict(table=b"".join(np.ascontiguousarray(a[order]).tobytes() for a in (keys, w, n, z)),
                nkeys=len(keys), pred=open(pred, "rb").read(),
                lines=[ln for ln in printed.split("\n") if ln.startswith(PRINTED)],
                metrics={n: bits(x.metric(n)) for n in metrics},
                blocks_gpu=x.metric("blocks_gpu"), value=lambda n: x.metric(n))


def same(a, b, what=("table", "pred", "lines", "metrics")):
    for k in what:
        assert a[k] == b[k], k
    assert a["nkeys"] > 100 and len(a["pred"]) > 10000


_all = {}


def all_stages(data, capfd, ingest, cache_batches=1, block_size_mb=1):
    key = (ingest, cache_batches, block_size_mb)
    if key not in _all:
        _all[key] = run(data, "all_%s_%d_%d" % key, capfd, PROGRESS + SLICES + HOLDOUT + GAUC + COUNTS,
                        ingest=ingest, cache_batches=cache_batches, block_size_mb=block_size_mb,
                        **SPLIT, **REST)
    return _all[key]


def kept_rows(data):
    """per epoch that samples: the rows the sampler keeps when it numbers the rows of the TRAIN
    part, in file order across the blocks, under the stream (epoch << 32) | rank 0"""
    labels = labels_of(str(data / "train-00000"))
    m = H.held(0, 0, np.arange(len(labels), dtype=np.uint64), SHARE)
    assert np.array_equal(labels[~m], labels_of(str(data / "kept-00000")))
    train = labels[~m].astype(np.int32)
    return [int(N.Sampler(KEEP, 0).mask(e << 32, 0, train).sum()) for e in range(EPOCHS)], int(m.sum())


# ---- case 1: every stage at once, through both doors
@pytest.mark.parametrize("cache_batches", [1, 0])
def test_every_stage_at_once_both_ingest_paths(data, capfd, cache_batches):
    """host arrays enter through the first stage's upload, the tokeniser's device arrays below it:
    the same table, predictions, printed lines and metrics.  cache_batches=0: the second epoch
    reads the text again — the counts start again, the held list is dropped and rebuilt"""
    host = all_stages(data, capfd, "host", cache_batches)
    gpu_ = all_stages(data, capfd, "gpu_fields", cache_batches)
    assert host["blocks_gpu"] == 0 and gpu_["blocks_gpu"] == (3 if cache_batches else 3 * EPOCHS)
    same(host, gpu_)
    assert len(host["lines"]) >= 4 * EPOCHS
    for head in PRINTED:
        assert sum(ln.startswith(head) for ln in host["lines"]) >= EPOCHS, head
    # the sampler numbers the rows of the train part, on across the blocks
    kept, held = kept_rows(data)
    sampled = kept[:1] if cache_batches else kept
    assert host["value"]("rows_kept") == sum(sampled)
    assert host["value"]("rows_trained") == (EPOCHS * kept[0] if cache_batches else sum(kept))
    assert host["value"]("holdout_rows") == held


# ---- case 2: the order across the split
def test_the_split_comes_first_counts_across_blocks(data, capfd):
    """the all-stage run against the run on the kept file without the split: the sampler sees, and
    numbers, the train part only — whatever the block cuts (the kept file's 1 MiB blocks are not
    the train parts of the full file's: the minibatches differ, the kept rows do not)"""
    full = all_stages(data, capfd, "host")
    kept = run(data, "kept_host", capfd, PROGRESS + SLICES + COUNTS, train="kept", ingest="host",
               **REST)
    for n in ("rows_trained", "rows_kept", "neg_seen", "neg_kept", "progress_rows", "slice_rows"):
        assert full["metrics"][n] == kept["metrics"][n], n


def test_the_split_comes_first_one_block(data, capfd):
    """... and where both files are one block (one 4 MiB buffer) the minibatches are the same: the
    table and the predictions bit for bit, so slices, cross, admission and row norm saw the train
    part only and the held rows passed admission uncounted"""
    full = all_stages(data, capfd, "gpu_fields", 1, 4)
    kept = run(data, "kept_one", capfd, PROGRESS + SLICES + COUNTS, train="kept", ingest="gpu_fields",
               block_size_mb=4, **REST)
    assert full["blocks_gpu"] == kept["blocks_gpu"] == 1
    same(full, kept, ("table", "pred"))
    for n in PROGRESS + SLICES + ["rows_trained", "rows_kept", "neg_seen", "neg_kept"]:
        assert full["metrics"][n] == kept["metrics"][n], n
    head = PRINTED[:3]
    assert [ln for ln in full["lines"] if ln.startswith(head)] == kept["lines"] != []


# ---- case 3: each first stage as the host door
FIRST = {
    "holdout": (dict(holdout=SHARE), HOLDOUT),
    "neg_keep": (dict(neg_keep=KEEP), []),
    "cross": (dict(cross="2*3"), []),
    "admit": (dict(ADMIT), []),
    "row_norm": ({}, []),
}


@pytest.mark.parametrize("first", list(FIRST))
def test_each_first_stage_as_the_host_door(data, capfd, first):
    """exactly that stage and row normalisation behind it: entering below the first stage runs
    the rest of the chain"""
    params, metrics = FIRST[first]
    runs = [run(data, "%s_%s" % (first, ingest), capfd, metrics + COUNTS, ingest=ingest,
                row_norm="l2", feature_values="on", **params) for ingest in ("host", "gpu_fields")]
    assert runs[0]["blocks_gpu"] == 0 and runs[1]["blocks_gpu"] == 3
    same(*runs)
    assert runs[0]["value"]("norm_rows") > 0
    assert len(runs[0]["lines"]) == (EPOCHS if first == "holdout" else 0)


# ---- case 4: a block that loses every row
GONE = 1e-6


@pytest.fixture(scope="module")
def negatives(tmp_path_factory, data):
    d = tmp_path_factory.mktemp("stage_order_negatives")
    (d / "train-00000").write_bytes(Z.zipf_text(63, 200 << 10, positives=0.0))
    (d / "test-00000").write_bytes((data / "test-00000").read_bytes())
    labels = labels_of(str(d / "train-00000"))
    assert len(list(capi.read_blocks(str(d / "train-00000"), 1 << 20))) == 1
    assert len(labels) > 1000 and not labels.any()
    return d


@pytest.mark.parametrize("stages", ["neg_keep", "all"])
@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
def test_a_block_that_loses_every_row(negatives, capfd, ingest, stages):
    """no minibatch for that block, nothing trained, and the run ends clean (with the split on,
    the held part is still kept and validated)"""
    R = len(labels_of(str(negatives / "train-00000")))
    m = H.held(0, 0, np.arange(R, dtype=np.uint64), SHARE) if stages == "all" else np.zeros(R, bool)
    train = np.zeros(R - int(m.sum()), np.int32)
    for e in range(EPOCHS):                                      # on the CPU: no row survives
        assert not N.Sampler(GONE, 0).mask(e << 32, 0, train).any()
    params = dict(SPLIT, **REST) if stages == "all" else {}
    params["neg_keep"] = GONE
    r = run(negatives, "gone_%s_%s" % (stages, ingest), capfd,
            COUNTS + (HOLDOUT if stages == "all" else []), ingest=ingest, **params)
    v = r["value"]
    assert r["blocks_gpu"] == (0 if ingest == "host" else 1)
    assert v("rows_trained") == 0 and v("rows_kept") == 0 and v("neg_kept") == 0
    assert v("neg_seen") == len(train)
    assert set(r["pred"].split(b"\n")[:-1]) <= {b"0.5\t1\t0", b"0.5\t0\t1"}   # nothing was trained
    if stages == "all":
        assert v("holdout_rows") == int(m.sum()) > 100
