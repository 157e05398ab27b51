"""Value binning, the host side (xf_bin_host.cc; no GPU): the code of a value, the cut of a field's
counts, the key function and the parser, each with == against tests/_bin_checker.py."""
import numpy as np
import pytest

from xflow_amd import capi

from . import _bin_checker as B

F32 = np.float32


def _values():
    fmax = np.finfo(F32).max
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x80000001, 0x807fffff,
                     0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff], np.uint32)
    named = np.array(list(range(1, 18)) + [np.nextafter(F32(1), F32(0)), 1.0,
                                           np.nextafter(F32(1), F32(2)), fmax, -fmax, np.inf,
                                           -np.inf], F32)
    rnd = np.random.RandomState(1).randint(0, 1 << 32, size=4000, dtype=np.uint64)
    return np.concatenate([bits, named.view(np.uint32), rnd.astype(np.uint32)])


def test_code_against_the_restatement():
    bits = _values()
    want = B.code(bits.view(F32))
    got = np.array([capi.bin_code(v) for v in bits.view(F32)])
    assert capi.bin_code(3) == capi.bin_code(3.0) == B.code([3.0])[0]      # (an int is a value)
    assert np.array_equal(got, want)
    assert capi.bin_code(F32(np.inf)) == 4088 and capi.bin_code(-0.0) == capi.bin_code(0.0) == 2048
    assert len({capi.bin_code(float(i)) for i in range(1, 16)}) == 15
    nan = (bits & 0x7fffffff) > 0x7f800000
    assert nan.sum() >= 4 and (got[nan] == 4095).all() and (got[~nan] <= 4088).all()


def test_code_is_monotone():
    v = np.sort(_values().view(F32)[~np.isnan(_values().view(F32))])
    c = np.array([capi.bin_code(float(x)) for x in v])
    assert (np.diff(c) >= 0).all() and c[0] == 7 and c[-1] == 4088


def _count_vectors():
    rng = np.random.RandomState(2)
    z = np.zeros(4096, np.uint64)
    one = z.copy()
    one[2100] = 12345
    last = z.copy()
    last[4094] = 77
    few = z.copy()
    few[[5, 2048, 3000]] = (10, 1, 30)
    few[4095] = 9                                                 # NaNs: left out of T
    rnd = rng.randint(0, 1000, size=4096).astype(np.uint64) * (rng.rand(4096) < 0.1)
    big = z.copy()
    big[[100, 200]] = ((1 << 55) + 3, (1 << 55) - 4)              # T = 2^56 - 1: the widest product
    return [("zero", z), ("one_code", one), ("code_4094", last), ("few_codes", few),
            ("random", rnd.astype(np.uint64)), ("wide", big)]


@pytest.mark.parametrize("bins", [2, 3, 255])
@pytest.mark.parametrize("name,counts", _count_vectors(), ids=[n for n, _ in _count_vectors()])
def test_lut_against_python_ints(name, counts, bins):
    got, want = capi.bin_lut(counts, bins), B.lut(counts, bins)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert got[4095] == bins and got[:4095].max() <= bins - 1 and (np.diff(got[:4095].astype(int)) >= 0).all()
    if name == "few_codes" and bins == 255:
        assert len(set(got[:4095].tolist())) == 4                 # fewer distinct codes than bins


def test_lut_refuses_2_to_the_56():
    c = np.zeros(4096, np.uint64)
    c[[1, 2]] = (1 << 55, 1 << 55)
    assert B.lut(c, 2) is None
    with pytest.raises(capi.XFError, match=r"2\^56 or more fitted nonzeros"):
        capi.bin_lut(c, 2)
    c[4095], c[2] = 1 << 60, (1 << 55) - 1                        # (NaNs do not count)
    assert np.array_equal(capi.bin_lut(c, 2), B.lut(c, 2))


def test_key_known_answers():
    for k, f, b in ((0, 0, 0), (0x0123456789abcdef, 13, 31), (2**64 - 1, 2**31 - 1, 255)):
        assert capi.bin_key(k, f, b) == B.key(k, f, b)
    assert B.key(0, 0, 0) == B.mix64(B.mix64(B.SALT)) and capi.bin_key(5, 1, 2) != capi.bin_key(5, 2, 1)
    ks = np.arange(7, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
    assert [int(x) for x in B.mix64_np(ks)] == [B.mix64(int(x)) for x in ks]


REFUSED = [("13:32,13:16", "listed twice"), ("13:1", r"bins lies in 2 \.\. 255"),
           ("13:256", r"bins lies in 2 \.\. 255"), (",".join("%d:4" % i for i in range(65)),
                                                    "more than 64 pairs"),
           ("13:32,,14:32", "is not a pair FIELD:BINS"), ("", "the bin spec is empty"),
           ("-1:32", "is not a pair FIELD:BINS"), ("13:32,", "is not a pair FIELD:BINS")]


@pytest.mark.parametrize("spec,msg", REFUSED, ids=["duplicate", "bins1", "bins256", "pairs65",
                                                   "empty_item", "empty", "negative", "trailing"])
def test_parser_refusals(spec, msg):
    with pytest.raises(capi.XFError, match=msg):
        capi.bin_parse(spec)


def test_parser_and_create_take_a_good_spec():
    spec = ",".join("%d:%d" % (3 * i, 2 + i) for i in range(64))
    assert capi.bin_parse(spec) == [(3 * i, 2 + i) for i in range(64)]
    assert capi.Bin(spec).params() == capi.bin_parse(spec)      # (nothing touches the device)
    with pytest.raises(capi.XFError, match="listed twice"):
        capi.Bin([(4, 8), (4, 9)])
