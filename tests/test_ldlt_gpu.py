"""The blocked, multi-workgroup L D L^T of ms-slam_amd/csrc/ldlt_blocked.h alone, through msorb_ldlt_solve.

Matrices: symmetric positive definite and block-banded as a reduced camera system is: random 6 x 6 blocks within a band of four
blocks and one block pair that joins the first block with the last (a closed loop: fill far from the band), zero elsewhere, the
diagonal lifted to dominance.  Sizes: around the panel width NB and the trailing tile edge T (msorb_ldlt_block_sizes), the first
size msorb_local_ba refuses (774), a loop-closing size (1206) and one large one (3078).

Bound.  Up to n = 800 the host variants are the column-by-column L D L^T of tests/local_ba_cases.py, the same on the reversed
ordering, and LAPACK's LU; above, LAPACK only: LU, Cholesky, Cholesky of the reversed ordering.  The device's x lies within 16
times the largest distance between those variants on that matrix, relative to max |x|: the factor and the reason of DESIGN section
10 (the device's order is one more order).  The device goes through the subtractions of the column-by-column factorisation in the
same order, so against that variant it agrees to the last bit, which is asserted where that variant is computed (n <= 800).

Measured on an MI355X: DESIGN.md section 16."""
import numpy as np
import pytest

import local_ba_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678


def banded_spd(n, seed, band=4):
    rng = np.random.default_rng(seed)
    nb = (n + 5) // 6
    A = np.zeros((6 * nb, 6 * nb))
    for i in range(nb):
        for j in range(max(0, i - band), i + 1):
            B = rng.uniform(-1, 1, (6, 6))
            A[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
    if nb > 2 * band:
        A[6 * (nb - 1):, :6] = rng.uniform(-1, 1, (6, 6))
    A = np.tril(A)[:n, :n]
    A = A + np.tril(A, -1).T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(1) + 1.0
    return A, rng.uniform(-1, 1, n)


def _chol_solve(A, b):
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def host_variants(A, b):
    n = len(b)
    rev = np.arange(n)[::-1]
    Ar, br = np.ascontiguousarray(A[np.ix_(rev, rev)]), b[rev]
    if n <= 800:
        x0, x1 = np.zeros(n), np.zeros(n)
        assert lc.ldlt_solve(A.copy(), b, x0) and lc.ldlt_solve(Ar.copy(), br, x1)
        return [x0, x1[rev], np.linalg.solve(A, b)]
    return [np.linalg.solve(A, b), _chol_solve(A, b), _chol_solve(Ar, br)[rev]]


_cache = {}


def problem(n):
    if n not in _cache:
        A, b = banded_spd(n, 1000 + n)
        _cache[n] = (A, b, host_variants(A, b))
    return _cache[n]


def sizes(msorb_mod):
    NB, T = msorb_mod.ldlt_block_sizes()
    return sorted({1, 5, 6, NB - 1, NB, NB + 1, 2 * NB + 7, 774, 1206, 2 * NB + T - 1, 2 * NB + T + 1, 3078})


def test_block_sizes(msorb_mod):
    NB, T = msorb_mod.ldlt_block_sizes()
    assert NB % 6 == 0 and NB > 0 and T > 0
    assert msorb_mod.bundle_adjustment_capacity() == 1024


def test_against_the_host_variants(msorb_mod):
    worst = 0.0
    for n in sizes(msorb_mod):
        A, b, xs = problem(n)
        x, ok = msorb_mod.ldlt_solve(np.tril(A), b)       # only the lower triangle is given
        scale = np.abs(xs[0]).max()
        spread = max(np.abs(xs[a] - xs[c]).max() for a in range(3) for c in range(a + 1, 3)) / scale
        dist = max(np.abs(x - v).max() for v in xs[:1]) / scale
        ratio = dist / spread if spread else (0.0 if dist == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"n={n}: device - variant 0 = {dist:.3e}, spread of the host variants {spread:.3e}, ratio {ratio:.3f}, "
              f"entries that differ from variant 0: {int(np.sum(x != xs[0]))}")
        assert ok
        assert dist <= 16 * spread, n
        if n <= 800:                                          # the same subtractions in the same order as variant 0
            assert np.array_equal(x, xs[0]), n
    print(f"largest ratio {worst:.3f} (bound 16)")


def test_a_pivot_that_is_not_positive(msorb_mod):
    NB, _ = msorb_mod.ldlt_block_sizes()
    n = 3 * NB + 6
    A, b = banded_spd(n, 77)
    for j in (7, NB + 5, n - 1):                            # the first panel, the second, the last column
        B = A.copy()
        B[j, j] = -1.0
        assert np.linalg.eigvalsh(B[:j, :j]).min(initial=1.0) > 0    # every pivot before it is positive
        assert not lc.ldlt_solve(B.copy(), b, np.zeros(n))
        x = np.full(n, SENTINEL)
        x2, ok = msorb_mod.ldlt_solve(B, b, x)
        assert not ok and x2 is x and (x == SENTINEL).all(), j
    x, ok = msorb_mod.ldlt_solve(A, b, np.full(n, SENTINEL))          # and the flag does not stick
    assert ok and np.abs(x - np.linalg.solve(A, b)).max() < 1e-12


@pytest.mark.parametrize("n", [774, 1206])
def test_two_calls_return_the_same_bits(msorb_mod, n):
    A, b, _ = problem(n)
    x0, ok0 = msorb_mod.ldlt_solve(A, b)
    x1, ok1 = msorb_mod.ldlt_solve(A, b)
    assert ok0 and ok1 and x0.tobytes() == x1.tobytes()
