"""The steering helper (tests/steering.py) against the oracle alone, no GPU:
the steered inputs give the chosen residues, and for every output row they
reach fold96's rare branches -- `w >= p`, `u >> 32 == 1`, and every `t >> 32`
the code's sums can take -- at least once.  These are conditions the GPU tests
(tests/test_gpu_boundaries.py) rely on, checked for every code they use."""
import numpy as np
import pytest

import steering as ST
from oracle import oracle_c as OC

P = ST.P


def _check(coeff, x, tg, mask, n=None):
    out = OC.apply_matrix(coeff[:, :n] if n else coeff, list(x[:n] if n else x))
    for i in range(coeff.shape[0]):
        cols = mask[i]
        assert cols.sum() >= mask.shape[1] // 2, "every row is steered in most columns"
        assert np.array_equal(out[i][cols], tg[i][cols]), f"row {i}: the oracle's output is not the target"
        th_ok, u_ok, w_ok = ST.reachable(coeff[i], n)
        br = [ST.fold_branches(V) for V in ST.exact_sums(coeff[i], x[:, cols], n)]
        assert np.array_equal(np.array([b[3] for b in br], dtype=np.uint32), tg[i][cols]), "the restated fold"
        assert {b[0] for b in br} == th_ok, (i, {b[0] for b in br})
        assert not u_ok or sum(b[1] for b in br) >= 1, f"row {i}: u >> 32 == 1 never taken"
        assert not w_ok or sum(b[2] for b in br) >= 1, f"row {i}: w >= p never taken"
        # the last three columns (past the last whole vector) carry 0..4
        assert set(tg[i][-ST.TAIL_COLUMNS:].tolist()) <= set(range(5))


def test_target_set():
    tg = ST.targets(3)
    assert tg.shape == (3, ST.NCOLS) and ST.NCOLS % 4 == 3 and ST.NCOLS == 86 * 64 + 3
    want = set(range(41)) | set(range(P - 40, P)) | set(range(2**31 - 2, 2**31 + 3))
    for i in range(3):
        vals, counts = np.unique(tg[i][:-3], return_counts=True)
        assert set(vals.tolist()) == want and (counts == 64).all()
    assert (tg[0] != tg[1]).sum() >= ST.NCOLS - 3 and int(tg.max()) < P


@pytest.mark.parametrize("V", [0, 1, P - 1, P, P + 4, 2**32 - 1, 2**32, 2**64 - 1, 2**64, 25 * P + 3,
                               (2**32 - 1) * (2**32 - 1) * 112, 300 * 2**64 + 2**64 - 1])
def test_fold_branches_restates_the_fold(V):
    assert ST.fold_branches(V)[3] == V % P


@pytest.mark.parametrize("need,total", sorted(set(ST.ENCODE_CODES + ST.BYTE_CODES)))
def test_steered_columns_reach_every_branch(need, total):
    _check(*ST.encode_case(need, total))


@pytest.mark.parametrize("need,total", ST.BYTE_CODES)
def test_canonical_steering_for_the_byte_path(need, total):
    """The byte path's symbols come out of MapToGF: every input below p."""
    coeff, x, tg, mask = ST.encode_case(need, total, canonical=True)
    assert int(x.max()) < P
    _check(coeff, x, tg, mask)


@pytest.mark.parametrize("need,total,n", ST.PREFIXES)
def test_prefix_steering_reaches_the_running_residue_folds(need, total, n):
    """The partial sum over inputs 0..n-1 (what the wide kernels fold after n
    inputs) is steered; the inputs past n stay random."""
    coeff, x, tg, mask = ST.encode_case(need, total, prefix=n)
    _check(coeff, x, tg, mask, n)


@pytest.mark.parametrize("need,total,n", ST.BYTE_PREFIXES)
def test_canonical_prefix_steering_for_the_wide_byte_kernels(need, total, n):
    coeff, x, tg, mask = ST.encode_case(need, total, prefix=n, canonical=True)
    assert int(x.max()) < P
    _check(coeff, x, tg, mask, n)


def test_steering_a_reconstruct_matrix_and_chosen_inputs():
    """Any matrix with an invertible block: a 2-row reconstruct matrix of 4/6
    steered through inputs 1 and 3."""
    cw = OC.parity_matrix(4, 2)
    have = [1, 2, 4, 5]
    rc, inv = OC.invert_matrix(cw[have])
    assert rc == 0
    coeff = np.ascontiguousarray(inv[[0, 3]])
    tg = ST.targets(2)
    x = ST.steer(coeff, tg, np.random.default_rng(3), steer_inputs=[1, 3])
    _check(coeff, x, tg, ST.steered_rows(2, 4, tg.shape[1]))
