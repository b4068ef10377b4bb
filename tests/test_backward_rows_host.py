"""What tests/backward_rows_cases.py promises, checked without a device: its fp64 references are torch.autograd's gradients, the integer
leg's sums are exact in fp32, the relu LayerNorm cases zero almost nothing, and the row lists straddle the kernels' constants as
csrc/backward_ops.hip states them today."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import backward_rows_cases as C

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sparsebev_amd', 'csrc', 'backward_ops.hip')


def close(a, b):
    return C.rel_err(a, b) < 1e-12


@torch.enable_grad()
@pytest.mark.parametrize('M,N', [(1, 1), (17, 10), (65, 63), (900, 256)])
def test_bias_reference_is_autograd_of_linear_relu(M, N):
    g = torch.Generator().manual_seed(M + N)
    K = 7
    x, w = torch.randn(M, K, generator=g).double(), torch.randn(N, K, generator=g).double()
    b = torch.randn(N, generator=g).double().requires_grad_(True)
    gy = torch.randn(M, N, generator=g)
    z = F.linear(x, w, b)
    z.retain_grad()
    y = z.relu()
    y.backward(gy.double())
    dZ, db = C.bias_relu_ref(gy, y.detach())
    assert close(dZ, z.grad) and close(db, b.grad)
    before = torch.randn(N, generator=g)
    assert close(C.bias_relu_ref(gy, y.detach(), before)[1], b.grad + before.double())
    # no mask: the plain column sum
    b.grad = None
    F.linear(x, w, b).backward(gy.double())
    dZ, db = C.bias_relu_ref(gy)
    assert torch.equal(dZ, gy.double()) and close(db, b.grad)


@torch.enable_grad()
@pytest.mark.parametrize('M,N', [(1, 4), (5, 8), (33, 252), (17, 256), (5, 1024)])
@pytest.mark.parametrize('relu', [0, 1])
def test_layer_norm_reference_is_autograd(M, N, relu):
    c = C.ln_case(M, N, relu)
    x, w, b = (c[k].double().requires_grad_(True) for k in ('X', 'gamma', 'beta'))
    y = F.layer_norm(x, [N], w, b, eps=C.EPS)
    (y.relu() if relu else y).backward(c['dY'].double())
    r = C.layer_norm_ref(c['dY'], c['X'], c['gamma'], c['beta'], relu)
    assert close(r['dX'], x.grad) and close(r['dgamma'], w.grad) and close(r['dbeta'], b.grad)
    acc = C.layer_norm_ref(c['dY'], c['X'], c['gamma'], c['beta'], relu, c['dgamma_before'], c['dbeta_before'])
    assert close(acc['dgamma'], w.grad + c['dgamma_before'].double()) and close(acc['dbeta'], b.grad + c['dbeta_before'].double())
    assert close(r['mean'], c['X'].double().mean(1)) and close(r['rstd'], (c['X'].double().var(1, unbiased=False) + C.EPS).rsqrt())


def test_group_references_are_sums_of_the_single_ones():
    groups = C.ln_group_case(17)
    for grp in groups:
        dg, db, refs = C.ln_group_ref(grp)
        one = torch.cat([dY for dY, _ in grp['segs']]), torch.cat([X for _, X in grp['segs']])      # the segments stacked: one LayerNorm call
        r = C.layer_norm_ref(*one, grp['gamma'], grp['beta'], grp['relu'], *((grp['dgamma_before'], grp['dbeta_before']) if grp['accumulate'] else ()))
        assert close(dg, r['dgamma']) and close(db, r['dbeta']) and len(refs) == len(grp['segs'])
    for segs, out0 in C.colsum_group_case(17, 'real'):
        assert close(C.colsum_group_ref(segs, out0), torch.cat(segs).double().sum(0) + out0.double())
    case = C.gemm_case(10, 256, 37, 'real')
    A, B, C0, _ = case
    assert close(C.gemm_ref(case, 3, 1), torch.cat(A[:3], 1).double() @ torch.cat(B[:3], 0).double() + C0.double())
    assert C.gemm_ref(case, 0, 0).abs().max() == 0
    for ak, bk in C.LAYOUTS:                     # the stored operands read back by the contract's index formulas
        As, Bs = C.stored(A[0], ak, True), C.stored(B[0], bk, False)
        assert As.is_contiguous() and Bs.is_contiguous()
        assert (As[3, 2] if ak else As[2, 3]) == A[0][2, 3] and (Bs[3, 5] if bk else Bs[5, 3]) == B[0][3, 5]


def test_integer_leg_is_exact_in_fp32():
    """every builder asserts its own bound (the sum of absolute values one output adds up stays below 2^24); here every listed shape is
    built once with M or K as the only thing that matters, and the values are checked to be the small integers the bound assumes"""
    for M in C.BIAS_M:
        dY, _, db0 = C.bias_case(M, 10, 'int', False)
        assert dY.abs().max() <= 3 and torch.equal(dY, dY.round()) and db0.abs().max() <= 3
        assert 3 * M + 3 < C.EXACT_LIMIT
    for M in C.COLSUM_GROUP_M:
        for (segs, out0), N, ns in zip(C.colsum_group_case(M, 'int', (3, 65), (8, 1)), (3, 65), (8, 1)):
            assert len(segs) == ns and all(s.shape == (M, N) and s.abs().max() <= 3 and torch.equal(s, s.round()) for s in segs)
        assert 3 * M * max(C.COLSUM_NSEGS) + 3 < C.EXACT_LIMIT
    assert len(C.COLSUM_WIDTHS) == len(C.COLSUM_NSEGS) == len(C.COLSUM_ACC) == 16 and sorted(set(C.COLSUM_NSEGS)) == list(range(1, 9))
    for M, N, K in C.GEMM_MULTI_SHAPES:
        assert 8 * K * 4 + 3 < C.EXACT_LIMIT
    A, B, C0, prods = C.gemm_case(130, 129, 33, 'int')
    assert all(t.abs().max() <= 2 and torch.equal(t, t.round()) for t in A + B) and C0.abs().max() <= 3
    assert all(torch.equal(p, p.round()) and p.abs().max() <= 4 * 33 for p in prods)
    with pytest.raises(AssertionError):
        C.assert_exact(C.EXACT_LIMIT, 'the limit itself')


def test_relu_output_holds_both_zeros_and_denormals():
    _, Y, _ = C.bias_case(17, 10, 'real', True)
    bits = Y.view(torch.int32).view(-1)
    tiny = torch.finfo(torch.float32).tiny
    assert (bits == 0).any() and (bits == -2 ** 31).any()                             # +0 and -0
    assert ((Y > 0) & (Y < tiny)).any() and ((Y < 0) & (Y > -tiny)).any()             # a positive and a negative denormal
    dZ, _ = C.bias_relu_ref(torch.ones_like(Y), Y)
    assert torch.equal(dZ[(Y > 0) & (Y < tiny)], torch.ones(int(((Y > 0) & (Y < tiny)).sum()), dtype=torch.float64))
    assert dZ[Y == 0].abs().max() == 0 and dZ[Y < 0].abs().max() == 0


def test_relu_layer_norm_cases_zero_almost_nothing():
    for M, N in C.ln_shapes():
        c = C.ln_case(M, N, 1)
        assert c['share'] <= C.MAX_ZEROED_SHARE, (M, N, c['share'])
        pre = C.layer_norm_ref(c['dY'], c['X'], c['gamma'], c['beta'], 1)['pre']
        assert c['dY'][pre.abs() < C.NEAR_ZERO].abs().sum() == 0
        assert 0.5 <= c['gamma'].min() and c['gamma'].max() <= 1.5
        assert C.ln_case(M, N, 0)['share'] == 0
    for M in C.LN_GROUP_M:
        for grp in C.ln_group_case(M):
            assert grp['share'] <= C.MAX_ZEROED_SHARE, (M, grp['gamma'].shape[0], grp['share'])
    assert len(C.LN_GROUP_WIDTHS) == len(C.LN_GROUP_NSEGS) == len(C.LN_GROUP_RELU) == len(C.LN_GROUP_ACC) == 8
    assert sorted(C.LN_GROUP_NSEGS) == list(range(1, 9)) and all(n % 4 == 0 and 4 <= n <= 1024 for n in C.LN_GROUP_WIDTHS)


def _constant(name):
    with open(SRC) as f:
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, f.read())
    assert m, name + ' not found in backward_ops.hip'
    return int(m.group(1))


def test_row_lists_straddle_the_kernels_constants():
    """whoever moves ONE_PASS_ROWS or ROW_CHUNK has to move the lists with them"""
    chunk, one_pass = _constant('ROW_CHUNK'), _constant('ONE_PASS_ROWS')
    for rows in (C.BIAS_M, C.LN_M):
        assert one_pass in rows and one_pass + 1 in rows and one_pass - 1 in rows
        assert any(M > one_pass and M % chunk == 1 for M in rows)                     # one row in the last chunk
        assert any(M > one_pass and M % chunk not in (0, 1) for M in rows)            # a partial last chunk of several rows
    assert all(M <= one_pass for M in C.BIAS_M_ONE_PASS) and all(M > one_pass for M in C.BIAS_M_TWO_PASS)
    assert any(M > one_pass and M % chunk == 0 for M in C.BIAS_M_TWO_PASS)            # and a full one
    # the grouped kernels have no second path, but their callers run them at the two-pass row counts too
    assert any(M > one_pass for M in C.COLSUM_GROUP_M) and any(M > one_pass for M in C.LN_GROUP_M)
    assert {M for M, _ in C.bias_shapes()} == set(C.BIAS_M) and {N for _, N in C.bias_shapes()} == set(C.BIAS_N)
    assert {M for M, _ in C.ln_shapes()} == set(C.LN_M) and {N for _, N in C.ln_shapes()} == set(C.LN_N)
