"""Steered inputs: columns whose output rows are chosen residues of GF(p).

Every data kernel ends in fold96 (slime_amd/csrc/gfp.hpp) plus one conditional
subtract of p.  Its two rare branches (`u >> 32 == 1`, `w >= p`) are taken only
when a row's residue is one of a few dozen small values, which random data
reaches with probability about 2^-30 a column.  For a coefficient matrix with
an invertible r x r block, r of the inputs of a column can be SOLVED so that r
output rows equal chosen residues: steer() does that with the oracle's matrix
inverse and apply_matrix.  Steering only chooses inputs; what a kernel must
compute on them always comes from the oracle applied to those inputs.

fold_branches() restates fold96's three steps over Python integers.  It is a
coverage precondition (tests/test_steering.py: the steered set really reaches
the branches) and never an expectation.
"""
import numpy as np

from oracle import oracle_c as OC

P = 2**32 - 5
COLS_PER_TARGET = 64
# The residues next to 0 and p (the fold's two rare branches live in 0..39), and
# the values around 2^31 (the sign bit of every 32-bit compare).
TARGET_VALUES = np.array(list(range(41)) + list(range(P - 40, P)) + list(range(2**31 - 2, 2**31 + 3)),
                         dtype=np.uint32)
TAIL_COLUMNS = 3
NCOLS = TARGET_VALUES.size * COLS_PER_TARGET + TAIL_COLUMNS  # 5507: L % 4 == 3
assert NCOLS % 4 == 3


def targets(rows: int, values=TARGET_VALUES, per: int = COLS_PER_TARGET, tail: int = TAIL_COLUMNS) -> np.ndarray:
    """rows x (len(values) * per + tail) residues: `per` columns per value, row i
    rolled by i values so that the rows of one column hit different targets,
    then `tail` columns of 0..4 (the columns past the last whole vector)."""
    base = np.repeat(np.asarray(values, dtype=np.uint32), per)
    out = np.empty((rows, base.size + tail), dtype=np.uint32)
    for i in range(rows):
        out[i, :base.size] = np.roll(base, i * per)
        out[i, base.size:] = (np.arange(tail) + i) % 5
    return out


def steered_rows(rows: int, k: int, ncols: int, prefix=None) -> np.ndarray:
    """rows x ncols bool: which output rows steer() steers in which column.  A
    matrix with more rows than (prefix) inputs steers r = min(inputs, rows) of
    them; column c steers rows (c + i) % rows, i < r, so every row gets its
    share of every target."""
    n = k if prefix is None else prefix
    r = min(n, rows)
    mask = np.zeros((rows, ncols), dtype=bool)
    for g in range(rows if r < rows else 1):
        cols = np.arange(g, ncols, rows) if r < rows else np.arange(ncols)
        mask[[(g + i) % rows for i in range(r)], cols[:, None]] = True
    return mask


def _sub_mod(a, b):
    """(a - b) mod p of canonical uint32 arrays."""
    return ((a.astype(np.uint64) + P - b.astype(np.uint64)) % P).astype(np.uint32)


def _invertible_block(coeff, row_set, n, steer_inputs):
    """r input indices below n whose block with row_set is invertible, and its inverse."""
    r = len(row_set)
    tries = [list(steer_inputs)] if steer_inputs is not None else \
        [[(s + i) % n for i in range(r)] for s in [n - r] + list(range(n))]
    for cols in tries:
        rc, inv = OC.invert_matrix(coeff[np.ix_(row_set, cols)] % P)
        if rc == 0:
            return cols, inv
    raise ValueError("no invertible block among the steerable inputs")


def steer(coeff, targets, rng, steer_inputs=None, prefix=None, canonical=False, lift=True) -> np.ndarray:
    """k x ncols uint32 inputs whose steered output rows equal `targets`
    (rows x ncols canonical residues; steered_rows() says which rows those are).

    The unsteered inputs are random over the whole uint32 range (non-canonical
    values included; canonical=True draws them below p, for symbols that come
    out of MapToGF).  The steered inputs -- steer_inputs, by default the last
    r = min(inputs, rows) of them -- are solved: x_S = inv(C[R,S]) (t - C[R,rest] x_rest),
    with the oracle's invert_matrix and apply_matrix.  prefix=n steers the
    partial sum over inputs 0..n-1 (the running residue a kernel folds after
    n inputs) and leaves inputs n.. random.  lift: every other solved input
    below 5 is given as its non-canonical representative x + p."""
    coeff = np.ascontiguousarray(coeff, dtype=np.uint32)
    rows, k = coeff.shape
    tg = np.asarray(targets, dtype=np.uint32)
    assert tg.shape[0] == rows and int(tg.max()) < P
    ncols = tg.shape[1]
    n = k if prefix is None else prefix
    assert 1 <= n <= k
    r = min(n, rows)
    hi = P if canonical else 2**32
    x = rng.integers(0, hi, size=(k, ncols), dtype=np.uint64).astype(np.uint32)
    mask = steered_rows(rows, k, ncols, prefix)
    groups = rows if r < rows else 1
    for g in range(groups):
        cols = np.arange(g, ncols, groups)
        row_set = [(g + i) % rows for i in range(r)] if r < rows else list(range(rows))
        assert mask[row_set][:, cols].all()
        S, inv = _invertible_block(coeff, row_set, n, steer_inputs)
        rest = [j for j in range(n) if j not in S]
        rhs = [np.ascontiguousarray(tg[i, cols]) for i in row_set]
        if rest:
            part = OC.apply_matrix(coeff[np.ix_(row_set, rest)], [np.ascontiguousarray(x[j, cols]) for j in rest])
            rhs = [_sub_mod(t, q) for t, q in zip(rhs, part)]
        sol = OC.apply_matrix(inv, rhs)
        for j, v in zip(S, sol):
            if lift and not canonical:
                v = np.where((v < 5) & (cols % 2 == 1), v + np.uint32(P), v).astype(np.uint32)
            x[j, cols] = v
    return x


def exact_sums(coeff_row, x, n=None) -> list:
    """The exact integers sum_j c_j x_j (j < n) of every column, as Python ints:
    what a kernel's 96-bit accumulator holds before the fold."""
    n = len(coeff_row) if n is None else n
    lo = np.zeros(x.shape[1], dtype=np.uint64)
    hi = np.zeros(x.shape[1], dtype=np.uint64)
    for j in range(n):
        prod = np.uint64(int(coeff_row[j])) * x[j].astype(np.uint64)  # < 2^64: exact
        lo = lo + prod  # wraps
        hi += lo < prod
    return [(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())]


def fold_branches(V: int):
    """fold96's three steps over a Python integer V < 2^96:
    (t >> 32, u >> 32 == 1, w >= p, residue)."""
    lo, hi = V & (2**64 - 1), V >> 64
    l, m = lo & 0xFFFFFFFF, lo >> 32
    t = m * 5 + l + hi * 25
    u = (t >> 32) * 5 + (t & 0xFFFFFFFF)
    w = (u & 0xFFFFFFFF) + (u >> 32) * 5
    assert w < 2**32
    return t >> 32, u >> 32 == 1, w >= P, w - P if w >= P else w


def reachable(coeff_row, n=None):
    """What the fold of V = sum_j c_j x_j (j < n) can reach over uint32 inputs:
    (the t >> 32 values, whether u >> 32 == 1 can happen, whether w >= p can).
    A sum that can pass 2^64 reaches everything.  Below that hi = 0 and
    t = 5m + l with m up to max V >> 32 and l free: with m able to pass 2^31
    (3/5's first row, whose coefficients add up to p - 3) t >> 32 goes up to
    (5 max m + 2^32 - 1) >> 32 and both rare branches are open.  1/2's one
    coefficient is 1: V = t = u = w is the input itself, and only a
    non-canonical input reaches w >= p."""
    n = len(coeff_row) if n is None else n
    vmax = sum(int(c) for c in coeff_row[:n]) * (2**32 - 1)
    if vmax >= 2**64:
        return set(range(6)), True, True
    if vmax < 2**32:
        return {0}, False, vmax >= P
    if vmax >> 32 >= 2**31:
        return set(range(((vmax >> 32) * 5 + 2**32 - 1 >> 32) + 1)), True, True
    raise NotImplementedError("a sum this small: work out its reach before using it")


# The codes the boundary tests steer, and the prefixes (running-residue folds
# after 16, 32 and 48 inputs) of those with k > 16.
ENCODE_CODES = [(1, 2), (3, 5), (4, 6), (8, 12), (10, 14), (16, 20), (17, 20), (24, 32), (33, 50), (64, 80)]
BYTE_CODES = [(4, 6), (8, 12), (10, 14), (6, 14), (17, 20), (33, 50)]
PREFIXES = [(need, total, n) for need, total in ENCODE_CODES for n in (16, 32, 48) if n < need]
BYTE_PREFIXES = [(need, total, n) for need, total in BYTE_CODES for n in (16, 32) if n < need]

_cases = {}


def encode_case(need: int, total: int, prefix=None, canonical=False):
    """(coeff, x, targets, mask) of one code's parity rows, steered; computed once and read-only."""
    key = (need, total, prefix, canonical)
    if key not in _cases:
        coeff = OC.parity_matrix(need, total - need)[need:]
        tg = targets(total - need)
        rng = np.random.default_rng([need, total, prefix or 0, int(canonical)])
        x = steer(coeff, tg, rng, prefix=prefix, canonical=canonical)
        mask = steered_rows(total - need, need, tg.shape[1], prefix)
        for a in (coeff, x, tg, mask):
            a.setflags(write=False)
        _cases[key] = (coeff, x, tg, mask)
    return _cases[key]
