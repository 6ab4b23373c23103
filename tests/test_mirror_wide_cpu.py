"""The wide mirror finish's bound on the model (mirror_wide_ref.py): sound however the rows fall to the workgroups. No engine code."""
import numpy as np
import pytest

import mirror_wide_ref as W


@pytest.mark.parametrize("n_lists,c,seed", [(1, 1024, 0), (3, 1024, 1), (17, 1024, 2), (17, 4096, 3), (512, 1024, 4), (512, 4096, 5), (80, 4096, 6)])
def test_every_key_that_is_no_candidate_is_at_least_the_bound(n_lists, c, seed):
    """Lists cut from a full key array as a pass cuts them (a workgroup owns up to 200 rows and lists its 64 smallest keys)."""
    rng = np.random.default_rng(seed)
    dist = np.where(rng.random((n_lists, 200)) < 0.3, np.float32(0.25), rng.random((n_lists, 200), dtype=np.float32))   # ties: the row decides
    owned = W.keys_of(dist, np.arange(dist.size).reshape(dist.shape) + 5)
    owned[rng.random(dist.shape) < rng.random((n_lists, 1))] = W.PAD           # workgroups of every size, some below 64 rows
    keys = owned[owned != W.PAD]
    cand, b, source = W.select_model(np.sort(owned, axis=1)[:, :W.KP], c)
    rest = np.setdiff1d(keys, cand)
    assert len(cand) <= c and len(rest) == len(keys) - len(cand) and (len(rest) == 0 or rest.min() >= b)
    assert (source == W.ALL) == (b == W.PAD) and (b != W.PAD or len(cand) == len(keys))
