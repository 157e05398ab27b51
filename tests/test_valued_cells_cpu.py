"""The edge streams of the valued cells tests (tests/_valued_cells_cases.py) under the checker of
tests/_valued_checker.py alone, no GPU: every fp64 sum the checker forms — row sums of w x, key
sums of loss x — is formed over its addends in ascending and in descending order, and NO sum may
differ.  That is the condition under which tests/test_gpu_valued_cells.py may compare the GPU's
cell kernels (whose LDS atomics land in any order) with the checker bit for bit.  A stream that
fails here is changed; the rule is not."""
import numpy as np
import pytest

from . import _valued_cells_cases as Cs
from . import _valued_checker as V


@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("name", Cs.EDGES)
def test_every_sum_of_the_edge_streams_is_exact(name, opt):
    mbs, aged, _ = Cs.edge(name)
    audit = []
    losses, ws, pctr = Cs.run_checker(opt, mbs, aged, audit)
    rowptr, keys, vals, labels = mbs[-1]
    V.lr_step(ws, rowptr, keys, vals, labels, audit)         # the replay the GPU test makes
    V.assert_exact(audit)
    d = V.disagreements(audit)
    assert set(d) == {"wx", "gw"} and all(n > 0 for n, _ in d.values()), d
    for (rp, _, _, lab), loss in zip(mbs, losses):
        assert loss.dtype == np.float32 and loss.shape == (len(rp) - 1,) == lab.shape


def test_the_streams_hit_the_edges_they_are_named_for():
    """what can be said without the GPU's cells: rows per window, entries per block and chunk"""
    (rp, keys, vals, _), = Cs.edge("two_windows")[0][:1]
    assert len(rp) - 1 == Cs.WIN_MAX + 100 and np.diff(rp.astype(np.int64)).min() >= 1 \
        and np.diff(rp.astype(np.int64)).max() <= 3
    for rp, keys, vals, _ in Cs.edge("split_chunk")[0]:
        cnt = np.unique(keys, return_counts=True)[1]
        assert 45000 <= len(keys) <= 55000 and 2048 < len(cnt) <= 5001
        assert (cnt == 9000).sum() >= 1 and cnt.max() > Cs.SLICE_MAX   # overfills a work item
    assert all(0 < len(m[1]) < Cs.BLK for m in Cs.edge("below_blk")[0])
    assert all(len(m[1]) % Cs.BLK == 1 and len(m[1]) > Cs.BLK for m in Cs.edge("blk_plus_one")[0])
    assert Cs.empty()[0].tolist() == [0] and len(Cs.empty()[3]) == 0
    assert len(Cs.empty_rows()[3]) == 3 and len(Cs.empty_rows()[1]) == 0
    rp, keys, vals, _ = Cs.edge("twice_in_row")[0][0]
    a = int(rp[1])
    assert keys[a] == keys[a + 2] and vals[a] != vals[a + 2] and int(rp[2]) - a == 3
    (rp, keys, vals, _), = Cs.edge("fresh_grow")[0]
    distinct = len(np.unique(keys))
    assert distinct * 10 > Cs.edge("fresh_grow")[2] * 6 and distinct < len(keys) // 2
