"""The GPU tokeniser's field modes (xf_ingest_set_fields, k_tok_emit<FG, VAL>) and ingest=gpu_fields
on a real MI355X.  The oracle is the host parser (pinned to the reference by
tests/golden/ref_parse_*.npz; its values are (float)atof): every comparison is bit for bit, values
as uint32 views (-0.0f and +0.0f differ), no tolerance anywhere.

* the reference's sample files and generated blocks inside the two classes
  (tests/_ingest_fields_cases.py): rowptr, keys, labels, fgid, vals are the host parser's, no
  block is handed back — at text sizes of one tile per workgroup (64 KiB), many (1 MiB) and two
  tiles per workgroup (just over 4 MiB: the span boundary is no launch boundary);
* every token outside a class hands its block back when that class's mode is on and is accepted,
  with today's arrays, when it is off;
* the worker: valued LR, valued canonical FM, field-aware FM without and with values train the
  model of ingest=host from text tokenised on the GPU — metrics, tables, prediction file.

The issue lists 0.000000000000001 among the values inside the class.  It holds 16 digits, one more
than the class (1 .. 15) and the host's direct conversion take, so it is tested where the class
puts it: with the 16-digit defect, handed back when values are on; .000000000000001 (15 digits,
nf = 15) covers that end of the table inside the class."""
import os

import numpy as np
import pytest

from xflow_amd import capi

from . import _ingest_fields_cases as cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = {"fg": (True, False), "val": (False, True), "fg+val": (True, True)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


@pytest.fixture(scope="module")
def ing():
    return capi.Ingest(1 << 23)


_host = {}


def host(text, values=True):
    """the host parser's (rowptr, keys, fgid, labels, vals) of a block, computed once per text
    (values=False: vals is None — the parser reads no third field, so none can fail it)"""
    k = (len(text), hash(text), values)
    if k not in _host:
        out = capi.parse_text_block(text, values=values)
        _host[k] = out if values else out + (None,)
    return _host[k]


def same_as_host(ing, text, fg, val):
    ing.fields(fgid=fg, values=val)
    ok, rp, ks, lb, gfg, gvs = ing.block_fields(text)
    assert ok, "a block inside the classes was handed back"
    hrp, hks, hfg, hlb, hvs = host(text, val)
    assert np.array_equal(rp.astype(np.uint64), hrp)
    assert np.array_equal(ks, hks) and np.array_equal(lb, hlb)
    assert (gfg is not None) == fg and (gvs is not None) == val
    if fg:
        assert gfg.dtype == np.int32 and np.array_equal(gfg, hfg)
    if val:
        assert gvs.dtype == np.float32
        assert np.array_equal(gvs.view(np.uint32), hvs.view(np.uint32))
    return len(lb), len(ks)


@pytest.mark.parametrize("name,cap", [("small_train-00000", 1000), ("small_train-00000", 4096),
                                      ("small_train-00000", 2097152), ("small_test-00000", 4096)])
def test_sample_files_block_for_block(ing, name, cap):
    rows = 0
    for t in capi.read_text_blocks(os.path.join(GOLD, name), cap):
        rows += same_as_host(ing, t, True, True)[0]
    assert rows == 200


@pytest.fixture(scope="module")
def generated():
    text, fg, vs = cases.gen_fields_text(7, (4 << 20) + 4096)
    assert 4 << 20 < len(text) < 1 << 23          # more than 1024 tiles: two per workgroup
    ends = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    return text, fg, vs, ends


def _texts(generated):
    text, _, _, ends = generated
    cut = lambda n: text[:int(ends[np.searchsorted(ends, n)]) + 1]
    # 64 KiB, 1 MiB, the whole text (> 4 MiB); without the final newline; three prefixes that end
    # at other line ends (other lengths modulo 16 and 4096)
    return [cut(64 << 10), cut(1 << 20), text, text[:-1], cut(5000), cut((1 << 20) + 12345),
            cut(3 << 20)]


@pytest.mark.parametrize("mode", list(MODES))
def test_generated_blocks_inside_the_classes(ing, generated, mode):
    fg, val = MODES[mode]
    text, efg, evs, _ = generated
    for t in _texts(generated):
        R, N = same_as_host(ing, t, fg, val)
        assert R == t.count(b"\n") + (0 if t.endswith(b"\n") else 1) and N > R
    # ... and the host parser's values are the class's own: float32(+-m / 10^nf), decimal fgid
    hfg, hvs = host(text)[2], host(text)[4]
    assert np.array_equal(hfg, efg) and np.array_equal(hvs.view(np.uint32), evs.view(np.uint32))


def test_mode_none_is_the_tokeniser_of_today(ing, generated):
    for t in _texts(generated)[:3]:
        ing.fields(False, False)
        ok, rp, ks, lb, fg, vs = ing.block_fields(t)
        ok2, rp2, ks2, lb2 = ing.block(t)
        assert ok and ok2 and fg is None and vs is None
        assert np.array_equal(rp, rp2) and np.array_equal(ks, ks2) and np.array_equal(lb, lb2)
        hrp, hks, _, hlb, _ = host(t)
        assert np.array_equal(rp.astype(np.uint64), hrp) and np.array_equal(ks, hks)
        assert np.array_equal(lb, hlb)


GOOD = b"0\t1:22:0.5 3:4:1\n1\t7:abc:-2.25\r\n"


def _placements(bad, at, filler):
    """the defect's line alone; first, in the middle and last in a larger good block; and behind
    filler so that a 4 KiB tile boundary falls right behind the byte at offset `at` of the line"""
    pre = filler[:filler.index(b"\n", 5000) + 1]
    pad = (-(len(pre) + at + 1)) % 4096
    pre += cases.pad_line(pad if pad >= 8 else pad + 4096)
    assert (len(pre) + at + 1) % 4096 == 0
    post = filler[:filler.index(b"\n", 3000) + 1]
    return [bad, bad + GOOD, GOOD + bad + GOOD, GOOD + bad, pre + bad + post, GOOD + bad[:-1]]


@pytest.fixture(scope="module")
def filler():
    return cases.gen_fields_text(1, 16 << 10)[0]


DEFECTS = [("val", v) for v in cases.VALUE_DEFECTS] + [("fg", f) for f in cases.FIELD0_DEFECTS]


@pytest.mark.parametrize("kind,field", DEFECTS, ids=["%s=%s" % (k, f.decode()) for k, f in DEFECTS])
def test_tokens_outside_a_class_hand_the_block_back(ing, filler, kind, field):
    if kind == "val":       # the tile boundary inside the third field (behind its first byte)
        bad, at = b"1\t12:22:" + field + b" 3:4:1\n", 8
    else:                   # ... behind field0's first byte (behind the tab for the empty one)
        bad, at = b"1\t" + field + b":22:0.5 3:4:1\n", 2
    on = [m for m in MODES.values() if m[0 if kind == "fg" else 1]]
    off = [m for m in ((False, False),) + tuple(MODES.values()) if not m[0 if kind == "fg" else 1]]
    for text in _placements(bad, at, filler):
        for fg, val in on:
            ing.fields(fg, val)
            assert not ing.block_fields(text)[0], (field, fg, val, len(text))
            same_as_host(ing, GOOD, fg, val)       # (the object still takes a good block)
        for fg, val in off:
            same_as_host(ing, text, fg, val)
    # the same line with the defect as the LAST token of its line (the field ends at '\n')
    last = b"1\t3:4:1 " + bad[2:bad.index(b" ")] + b"\n"
    for fg, val in on:
        ing.fields(fg, val)
        assert not ing.block_fields(GOOD + last + GOOD)[0]
    for fg, val in off:
        same_as_host(ing, GOOD + last + GOOD, fg, val)


def test_a_cr_in_mid_line(ing):
    """a CR that is not the line's last byte is a byte of the value to atof: the tokeniser may take
    the block (with the host's value) or hand it back"""
    text = b"0\t1:2:0.5\r 3:4:1\n"
    ing.fields(True, True)
    ok, rp, ks, lb, fg, vs = ing.block_fields(text)
    if ok:
        h = host(text)
        assert np.array_equal(vs.view(np.uint32), h[4].view(np.uint32)) and np.array_equal(fg, h[2])
    same_as_host(ing, b"0\t1:2:0.5 3:4:1\r\n1\t5:6:\r\n", True, True)   # (the CR LF that is dropped)
    same_as_host(ing, b"0\t1:2:0.5 3:4:-0\r", True, True)              # (a CR before the block's end)


# ------------------------------------------------------------------------------------ the worker
CONFIGS = {
    "lr+values": dict(model=0, feature_values="on"),
    "canonical+values": dict(model=1, k=4, fm_mode="canonical", feature_values="on"),
    "field_aware": dict(model=1, k=4, fm_mode="field_aware", fields=18),
    "field_aware+values": dict(model=1, k=4, fm_mode="field_aware", fields=18, feature_values="on"),
}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_fields")
    quirky = cases.worker_text(11, (2 << 20) + (100 << 10), quirks=True)
    clean = cases.worker_text(11, (2 << 20) + (100 << 10), quirks=False)
    assert 2 << 20 < len(clean) < len(quirky) < 3 << 20           # three 1 MiB blocks
    q = quirky.index(b"1e-1")
    assert 1 << 20 < q < (2 << 20) - 4096 and quirky.index(b"\ta:80") - q < 200   # the middle block
    (d / "quirky-00000").write_bytes(quirky)
    (d / "clean-00000").write_bytes(clean)
    (d / "test-00000").write_bytes(cases.worker_text(12, 40 << 10, quirks=False))
    return d


def _run(d, tag, train, ingest, params):
    pred = str(d / ("pred_%s" % tag))
    vdim = params.get("k", 10) * (params.get("fields", 1) if params.get("fm_mode") == "field_aware"
                                  else 1)
    x = capi.XFlow(str(d / train), str(d / "test"), epochs=3, block_size_mb=1, capacity=1 << 16,
                   ingest=ingest, pred_path=pred, **params)
    x.train()
    out = {m: x.metric(m) for m in ("logloss_ref", "auc", "rows_trained", "keys", "blocks_gpu",
                                    "blocks_host")}
    wh, vh = x.tables()
    tabs = [capi.Table.from_handle(wh, 1).export()]
    if params["model"] == 1:
        tabs.append(capi.Table.from_handle(vh, vdim).export())
    return out, tabs, open(pred).read()


def _same_model(a, b):
    (ma, ta, pa), (mb, tb, pb) = a, b
    for m in ("logloss_ref", "auc", "rows_trained", "keys"):
        assert ma[m] == mb[m], (m, ma[m], mb[m])
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert pa == pb and len(pa) > 0


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_worker_trains_the_model_of_the_host_parser(data, cfg):
    """three epochs over three 1 MiB blocks; the middle one holds values 1e-1 and +2 and a field0 of
    "a": handed back to the host parser (with its values), the other two tokenised on the GPU"""
    p = CONFIGS[cfg]
    h = _run(data, cfg + "_h", "quirky", "host", p)
    g = _run(data, cfg + "_g", "quirky", "gpu_fields", p)
    assert h[0]["blocks_gpu"] == 0 and h[0]["rows_trained"] > 0
    assert g[0]["blocks_gpu"] >= 2 and g[0]["blocks_host"] == 1, g[0]
    _same_model(h, g)
    c = _run(data, cfg + "_c", "clean", "gpu_fields", p)
    assert c[0]["blocks_host"] == 0 and c[0]["blocks_gpu"] >= 3, c[0]


def test_fgid_out_of_range_is_the_same_error(data, tmp_path):
    """fgid = fields in a block the tokeniser accepts: the device range check's error, as with the
    host parser"""
    text = cases.worker_text(5, 30 << 10, quirks=False)
    cutat = text.index(b"\n", len(text) // 2) + 1
    text = text[:cutat] + b"1\t3:5:1 18:6:0.5\n" + text[cutat:]
    (tmp_path / "train-00000").write_bytes(text)
    ing = capi.Ingest(1 << 20).fields(True, True)
    assert ing.block_fields(text)[0]                   # (inside both classes)
    for ingest in ("host", "gpu_fields"):
        x = capi.XFlow(str(tmp_path / "train"), str(data / "test"), epochs=1, block_size_mb=1,
                       capacity=1 << 16, ingest=ingest, pred_path=str(tmp_path / "p"),
                       **CONFIGS["field_aware"])
        with pytest.raises(capi.XFError, match=r"fgid .* outside"):
            x.train()


@pytest.mark.parametrize("model", [0, 1])
def test_gpu_fields_with_a_model_that_needs_no_field_is_ingest_gpu(data, model):
    p = dict(model=model) if model == 0 else dict(model=1, k=4)
    a = _run(data, "plain%d_gpu" % model, "quirky", "gpu", p)
    b = _run(data, "plain%d_gf" % model, "quirky", "gpu_fields", p)
    assert a[0]["blocks_gpu"] == b[0]["blocks_gpu"] >= 3 and b[0]["blocks_host"] == 0
    _same_model(a, b)
