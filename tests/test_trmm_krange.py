"""The per-tile K range of gemmul8_trmm's residue GEMMs (tile_krange, csrc/oz2_gemm_common.hpp) against brute force, on a host mirror of the rule
(trmm_util.tile_krange): with 256-row tiles and 128-wide K-steps over kp = ka padded to 256, a tile may skip a K-step only if the materialised
M = op(Atri) is structurally zero in all of the tile's rows (side L: the A operand, rows of M) or columns (side R: the B operand, columns of M) there.

  * the range contains every K-step that holds a structural non-zero of the tile;
  * it is minimal to one K-step: it begins at the first such K-step and ends at the last one, except that it is never shorter than the two K-steps of the
    256-wide block the diagonal crosses (at most one K-step of slack at an end, only where ka is not a multiple of 128 there);
  * its length summed over a square tile grid is T^2 (T + 1) of the rectangle's 2 T^3: the (T + 1) / (2 T) of the documentation.
No GPU."""
import itertools

import numpy as np
import pytest

import trmm_util as tu

KAS = [1, 127, 128, 129, 255, 256, 257, 511, 600, 1100]
CASES = list(itertools.product("LR", "LU", "NTC"))


def _structure(ka, uplo, trans, diag):
    """boolean ka x ka mask of the entries of M = op(Atri) that can be non-zero: built from a matrix with no zero entry, through the helpers the GPU tests use"""
    A = np.full((ka, ka), 2.0 + 1.0j)
    M = tu.materialise(A, uplo, trans, diag)
    assert (M[np.diag_indices(ka)] == (1 if diag == "U" else M[0, 0])).all()
    return M != 0


@pytest.mark.parametrize("ka", KAS)
@pytest.mark.parametrize("diag", "NU")
def test_every_tile_range_covers_the_nonzero_k_steps_and_no_more_than_one_beyond(ka, diag):
    kp = (ka + 255) // 256 * 256
    KT, T = kp // 128, kp // 256
    seen = set()
    for side, uplo, trans in CASES:
        kr = tu.krange_of(side, uplo, trans)
        seen.add(kr)
        S = np.zeros((kp, kp), bool)
        S[:ka, :ka] = _structure(ka, uplo, trans, diag)
        if side == "R":
            S = S.T   # the B operand's logical element (j, kk) is M(kk, j)
        # S[r, kk]: rows of the ranged operand x the inner dimension
        for t in range(T):
            k0, k1 = tu.tile_krange(kr, KT, t if side == "L" else 0, 0 if side == "L" else t)
            assert 0 <= k0 < k1 <= KT
            live = [ks for ks in range(KT) if S[256 * t:256 * t + 256, 128 * ks:128 * ks + 128].any()]
            assert live, (side, uplo, trans, t)   # every tile-row of a square operand holds its diagonal
            assert k0 <= live[0] and live[-1] < k1, (side, uplo, trans, t, (k0, k1), live)
            assert live[0] - k0 <= 1 and k1 - 1 - live[-1] <= 1, (side, uplo, trans, t, (k0, k1), live)
            if ka % 256 == 0:
                assert (k0, k1) == (live[0], live[-1] + 1)   # no slack without padding
            # the other dimension's tile index does not enter
            assert tu.tile_krange(kr, KT, t if side == "L" else 5, 7 if side == "L" else t) == (k0, k1)
    assert seen == {tu.KR_A_LOWER, tu.KR_A_UPPER, tu.KR_B_HIGH, tu.KR_B_LOW}


def test_the_four_cases_are_the_documented_intervals():
    KT = 12
    for t in range(6):
        assert tu.tile_krange(tu.KR_A_LOWER, KT, t, 99) == (0, min(KT, 2 * (t + 1)))
        assert tu.tile_krange(tu.KR_A_UPPER, KT, t, 99) == (2 * t, KT)
        assert tu.tile_krange(tu.KR_B_HIGH, KT, 99, t) == (2 * t, KT)
        assert tu.tile_krange(tu.KR_B_LOW, KT, 99, t) == (0, min(KT, 2 * (t + 1)))
    assert tu.tile_krange(0, KT, 3, 4) == (0, KT)
    # which case a call takes: M lower <=> (uplo L and N) or (uplo U and T / C)
    assert [tu.krange_of("L", u, t) for u, t in itertools.product("LU", "NTC")] == [1, 2, 2, 2, 1, 1]
    assert [tu.krange_of("R", u, t) for u, t in itertools.product("LU", "NTC")] == [3, 4, 4, 4, 3, 3]


@pytest.mark.parametrize("T", [1, 2, 3, 5, 8, 32])
def test_k_steps_summed_over_a_square_tile_grid_equal_the_closed_form(T):
    KT = 2 * T
    for kr in (tu.KR_A_LOWER, tu.KR_A_UPPER, tu.KR_B_HIGH, tu.KR_B_LOW):
        total = 0
        for tm, tn in itertools.product(range(T), range(T)):
            k0, k1 = tu.tile_krange(kr, KT, tm, tn)
            total += k1 - k0
        assert total == T * T * (T + 1)
        assert total / (T * T * KT) == (T + 1) / (2 * T)
    if T == 32:
        assert round((T + 1) / (2 * T), 2) == 0.52
