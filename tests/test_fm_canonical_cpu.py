"""Canonical FM without a GPU: the numpy checker of tests/_fmc_checker.py against Rendle's
pairwise form and against autograd, and the fm_mode parameter of the worker's C surface."""
import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _fmc_checker as F


def _batch(rng, R, max_len, nkeys, k, repeats=True, empty=True):
    lens = rng.randint(0 if empty else 1, max_len + 1, size=R)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(lens.sum())
    if repeats:
        fid = rng.randint(0, nkeys, size=n)
    else:                                    # distinct keys within every row
        fid = np.concatenate([rng.choice(nkeys, size=l, replace=False) for l in lens]) \
            if n else np.zeros(0, np.int64)
    labels = rng.randint(0, 2, size=R).astype(np.int32)
    U = nkeys
    wu = (rng.randn(U) * 0.1).astype(np.float32)
    vu = (rng.randn(U, k) * 0.1).astype(np.float32)
    return rowptr, fid.astype(np.int64), labels, wu, vu


@pytest.mark.parametrize("k", [1, 4, 10, 16, 64])
def test_y2_is_the_pairwise_interaction(k):
    rng = np.random.RandomState(k)
    rowptr, uidx, labels, wu, vu = _batch(rng, 60, 12, 40, k, repeats=False)
    _, _, _, T, Q = F.forward(rowptr, uidx, labels, wu, vu)
    y2 = 0.5 * (T - Q)
    for r in range(len(rowptr) - 1):
        V = vu[uidx[rowptr[r]:rowptr[r + 1]]].astype(np.float64)
        brute = sum(float(V[i] @ V[j]) for i in range(len(V)) for j in range(i + 1, len(V)))
        assert abs(np.float32(y2[r]) - brute) <= 1e-6 * (T[r] + Q[r]) + 1e-30, (r, y2[r], brute)
    # empty rows: no interaction, no linear term
    empty = np.diff(rowptr) == 0
    assert np.all(y2[empty] == 0)


@pytest.mark.parametrize("k,seed", [(3, 0), (10, 1), (16, 2)])
def test_gradients_equal_autograd(k, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(seed)
    rowptr, uidx, labels, wu, vu = _batch(rng, 80, 9, 25, k)   # repeated keys, empty rows
    assert (np.diff(rowptr) == 0).any()
    R, U = len(rowptr) - 1, len(wu)
    loss, _, S, _, _ = F.forward(rowptr, uidx, labels, wu, vu)
    gw, gv = F.gradient(rowptr, uidx, U, loss, S, vu)

    w = torch.tensor(wu.astype(np.float64), requires_grad=True)
    v = torch.tensor(vu.astype(np.float64), requires_grad=True)
    row = torch.tensor(F.rows_of(rowptr))
    ui = torch.tensor(uidx)
    Vn = v[ui]                                           # factors gathered per nonzero
    Sr = torch.zeros(R, k, dtype=torch.float64).index_add(0, row, Vn)
    Qr = torch.zeros(R, dtype=torch.float64).index_add(0, row, (Vn * Vn).sum(1))
    y2 = 0.5 * ((Sr * Sr).sum(1) - Qr)
    wx = torch.zeros(R, dtype=torch.float64).index_add(0, row, w[ui])
    y = torch.tensor(labels.astype(np.float64))
    L = torch.nn.functional.binary_cross_entropy_with_logits(wx + y2, y, reduction="mean")
    L.backward()
    for got, want in ((gw, w.grad.numpy()), (gv, v.grad.numpy())):
        tol = 1e-5 * (np.abs(want) + np.sqrt(np.mean(want * want)))
        bad = np.abs(got.astype(np.float64) - want) > tol
        assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])


def test_canonical_forward_differs_from_the_reference_form():
    """the reference's pooled term (sum_f sum_j v)^2 - sum v^2 is not the canonical one"""
    rng = np.random.RandomState(5)
    rowptr, uidx, labels, wu, vu = _batch(rng, 30, 8, 20, 8, repeats=False, empty=False)
    _, _, S, T, Q = F.forward(rowptr, uidx, labels, wu, vu)
    pooled = np.array([float(vu[uidx[rowptr[r]:rowptr[r + 1]]].astype(np.float64).sum()) ** 2
                       for r in range(len(rowptr) - 1)]) - Q
    assert np.max(np.abs(pooled - 0.5 * (T - Q))) > 1e-3


def test_fm_mode_parameter_of_the_worker():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    x.set("fm_mode", "canonical")
    x.set("fm_mode", "reference")
    rc = capi.lib().XFSetParam(x.h, b"fm_mode", b"bogus")
    assert rc == capi.XF_OK + 1                        # XF_EINVAL
    msg = capi.lib().xf_last_error().decode()
    assert "reference" in msg and "canonical" in msg, msg
    assert (capi.FM_REFERENCE, capi.FM_CANONICAL) == (0, 1)
