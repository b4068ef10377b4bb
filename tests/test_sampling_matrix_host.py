"""CPU half of the sampler forward matrix: the rotation covers what it claims, the coordinates reach the edges they are meant to, and the
yardstick -- the fp32 oracle's worst error against the fp64 oracle on each cell's inputs -- is a number a factor can be applied to."""
import pytest
import torch

import sampling_cases as SC


def test_matrix_rotation_covers_every_value_at_every_level_count():
    cells = SC.matrix_cells()
    assert len(cells) == 30 and len(set(c[:3] for c in cells)) == 30                   # the full cross L x storage x taps
    for L in range(1, 6):
        mine = [c for c in cells if c[0] == L]
        assert {c[3] for c in mine} == set(SC.C_LIST) and {c[4] for c in mine} == set(SC.P_LIST) and {c[5] for c in mine} == set(SC.N_LIST)
    for name in SC.DTYPES:                                                              # every storage type sees a second c0 trip and P > 4
        mine = [c for c in cells if c[1] == name]
        assert any(c[3] > 64 for c in mine) and any(c[4] > 4 for c in mine) and any(c[4] < 4 for c in mine)
    assert SC.PIPE_BP * SC.PIPE_Q > 8192 and (SC.PIPE_BP * SC.PIPE_Q) % 2 == 1
    assert all(P <= 4 and C <= 64 for _, P, C, _ in SC.PIPE_CASES)


@pytest.mark.parametrize('cell', SC.matrix_cells(), ids=SC.cell_id)
def test_fp32_oracle_error_is_a_usable_yardstick(cell):
    L, name, _, C, P, N = cell
    feats, loc, wts, ref, e32 = SC.cell_case(L, C, P, N, name)
    assert ref.dtype == torch.float64 and ref.shape == (SC.BP, SC.Q, C, P) and torch.isfinite(ref).all()
    print('%s: fp32 oracle vs fp64 %.3e, max |ref| %.2f' % (SC.cell_id(cell), e32, ref.abs().max().item()))
    assert 0 < e32 and SC.FACTOR * e32 < SC.TOL               # non-zero (a ratio exists) and the factor stays inside the project's bound
    # between a fraction of an fp32 ulp (6e-8) of the outputs' scale and one rounding per term of 4 L + 4: summation order, nothing else
    assert 1e-8 < e32 / ref.abs().max().item() < (4 * L + 4) * 6e-8
    # the inputs reach what they are meant to: both ends of the view clamp, a point inside and one wholly outside every level
    z = loc[..., 2] * (N - 1)
    if N > 1:
        assert (z > N - 0.5).any() and (z < -0.5).any()
    x, y = loc[..., 0], loc[..., 1]
    assert ((x > 0) & (x < 1) & (y > 0) & (y < 1)).any() and ((x < -1) | (x > 2)).any() and (x == 0).any() and (y == 1).any()
    if name != 'fp32':
        assert all(f.dtype == SC.DTYPES[name] for f in feats)


@pytest.mark.parametrize('case', SC.PIPE_CASES, ids=lambda c: 'L%d-P%d-C%d-%s' % c)
def test_pipelined_cases_yardstick(case):
    feats, loc, wts, ref, e32 = SC.pipe_case(*case)
    print('pipelined L%d P%d C%d %s: fp32 oracle vs fp64 %.3e' % (*case, e32))
    assert 0 < e32 and SC.FACTOR * e32 < SC.TOL and ref.shape[0] * ref.shape[1] == 8193
