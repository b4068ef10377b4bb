"""What tests/linear_fwd_cases.py promises, checked without a GPU: its fp64 references against the obvious torch compositions, the
integer leg's premise, that the listed cases reach every kernel of the fp32 Linear family -- asked of the library's own path
functions, which launch nothing -- and that the real leg's inputs keep every LayerNorm row well conditioned."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import linear_fwd_cases as C
from sparsebev_amd import _lib


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _close(a, b):
    assert (a - b).abs().max().item() < 1e-12


# ---- the references are the header's contracts ---------------------------------------------------------------------------------------------
def test_references_equal_the_torch_compositions():
    """both orders of ReLU and LayerNorm: the split-K family's ReLU is the Linear's (before the residual), sbev_layer_norm_f32's and the
    LayerNorm prologue's is the LayerNorm's (after it)"""
    g = torch.Generator().manual_seed(1)
    M, N, K = 7, 12, 20
    X, W, b, res = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((M, K), (N, K), (N,), (M, N)))
    gam, bet = torch.rand(N, generator=g, dtype=torch.float64) + 0.5, torch.randn(N, generator=g, dtype=torch.float64)
    lin = F.linear(X, W, b)
    for relu in (False, True):
        act = lin.relu() if relu else lin
        _close(C.linear_ref(X, W, b, res, relu), act + res)
        _close(C.linear_ref(X, W, None, None, relu), F.linear(X, W).relu() if relu else F.linear(X, W))
        _close(C.linear_ref(X, W, b, res, relu, xw=X @ W.t()), act + res)
        _close(C.splitk_ref(X, W, b, res, None, relu), act + res)
        _close(C.splitk_ref(X, W, b, res, (gam, bet), relu), F.layer_norm(act + res, (N,), gam, bet, C.EPS))
        slabs = torch.randn(3, M, N, generator=g, dtype=torch.float64)
        s = slabs[0] + slabs[1] + slabs[2] + b
        s = s.relu() if relu else s
        _close(C.reduce_ref(slabs, b, res, None, relu), s + res)
        _close(C.reduce_ref(slabs, b, res, (gam, bet), relu), F.layer_norm(s + res, (N,), gam, bet, C.EPS))
        ln = F.layer_norm(lin, (N,), gam, bet, C.EPS)
        _close(C.layer_norm_ref(lin, gam, bet, relu, res), (ln.relu() if relu else ln) + res)
        _close(C.layer_norm_ref(lin, gam, bet, relu), ln.relu() if relu else ln)
        for ln_relu in (False, True):
            W2 = torch.randn(5, N, generator=g, dtype=torch.float64)
            b2, res2 = torch.randn(5, generator=g, dtype=torch.float64), torch.randn(M, 5, generator=g, dtype=torch.float64)
            xn = (ln.relu() if ln_relu else ln) + res
            y = F.linear(xn, W2, b2)
            got_xn, got_y = C.ln_linear_ref(lin, gam, bet, ln_relu, res, W2, b2, res2, relu)
            _close(got_xn, xn)
            _close(got_y, (y.relu() if relu else y) + res2)
    # the two orders differ: a test that passes one for the other would fail
    a = C.splitk_ref(X, W, b, res, (gam, bet), True)
    assert (a - F.layer_norm(lin + res, (N,), gam, bet, C.EPS).relu()).abs().max().item() > 1e-2
    x3, w3, b3 = torch.randn(M, 10, generator=g, dtype=torch.float64), torch.randn(N, 3, generator=g, dtype=torch.float64), b
    y, pre = C.lin3_ref(x3, w3, b3, gam, bet)
    _close(pre, F.linear(x3[:, :3], w3, b3))
    _close(y, F.layer_norm(pre, (N,), gam, bet, C.EPS).relu())


# ---- the integer leg's premise ------------------------------------------------------------------------------------------------------------
def _all_linear_cases():
    return [c for p in C.LINEAR_PATHS for c in C.linear_cases(p)] + C.strip_leavers() + [c for g in C.GROUPS.values() for c in g]


def _all_splitk_cases():
    return [c for k in ('REGTILE', 'SPLIT128', 'SPLIT128_RAGGED') for c in C.splitk_cases(k)]


def test_integer_leg_is_exact_at_every_listed_shape():
    Ks = {c.K for c in _all_linear_cases()} | {c.K for c in _all_splitk_cases()} | {c.K for c in C.ln_linear_cases()}
    assert max(Ks) == 4096
    for K in Ks:
        assert C.int_bound(K) < C.EXACT_LIMIT
    assert C.int_bound(32800 // 9) < C.EXACT_LIMIT
    X, W, b, r = C.rows(5, 37, 'int'), C.weights(6, 37, 'int'), C.vector(6, 'int'), C.matrix(5, 6, 'int')
    for t, hi in ((X, 3), (W, 3), (b, 8), (r, 8)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max().item() <= hi
    assert X.abs().max().item() == 3 and b.abs().max().item() > 3          # the ranges are used
    S = C.slabs(3, 8, 5, 'int')
    assert torch.equal(S, S.round()) and S.abs().max().item() <= 1000 and 5 * 1000 + 16 < C.EXACT_LIMIT
    x3, w3, b3 = C.lin3_case(4, 8, 'int')
    assert all(torch.equal(t, t.round()) for t in (x3, w3, b3)) and 27 + 8 < C.EXACT_LIMIT
    # the reference of an integer case is the integer result: the float conversion the device test compares with is exact
    ref = C.linear_ref(X, W, b, r, True)
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    # builders are deterministic and cached
    assert C.rows(5, 37, 'int') is X and torch.equal(C.rows.__wrapped__(5, 37, 'int'), X)
    assert torch.equal(C.rows.__wrapped__(5, 37, 'real'), C.rows(5, 37, 'real'))


# ---- coverage, asked of the library --------------------------------------------------------------------------------------------------------
def _linear_path(lib, c):
    aligned = int(c.yoff % 4 == 0)                # every bias of the sweep is 16-byte aligned
    return lib.sbev_linear_f32_path(c.M, c.N, c.K, c.ldy, int(c.res is not None), aligned)


def test_linear_cases_take_the_path_they_are_listed_under(lib):
    seen = set()
    for c in _all_linear_cases():
        p = _linear_path(lib, c)
        assert p == C.LINEAR_PATHS.index(c.path), (c, p)
        seen.add(p)
        assert c.ldx % 4 == 0 and c.ldw % 4 == 0 and c.ldx >= c.K and c.ldw >= c.K and c.ldy >= c.N, c
    assert seen == set(range(6))
    for p in C.LINEAR_PATHS:
        assert C.linear_cases(p) and all(c.path == p for c in C.linear_cases(p))
    strip = C.LINEAR_PATHS.index('STRIP')
    for c in C.strip_leavers():
        assert c.path != 'STRIP' and _linear_path(lib, c) != strip
        if c.N != C.NOT_STRIP_N:                  # the same shape, plain, is a strip shape: one property each takes it away
            assert lib.sbev_linear_f32_path(c.M, c.N, c.K, c.N, 0, 1) == strip
    assert lib.sbev_linear_f32_path(17, C.NOT_STRIP_N, 256, C.NOT_STRIP_N, 0, 1) != strip
    assert lib.sbev_linear_f32_path(17, C.NOT_STRIP_N + 128, 256, C.NOT_STRIP_N + 128, 0, 1) == strip
    # the listed BIG128 shapes are the tile grids the list claims
    tiles = [((M + 127) // 128, (N + 127) // 128) for M, N in C.BIG_SHAPES]
    assert tiles == [(1, 257), (2, 129), (3, 87), (33, 9)] and (3 * 87) % 8 != 0 and all(a * b >= 256 for a, b in tiles)


def test_splitk_cases_take_the_path_they_are_listed_under(lib):
    seen = set()
    used = ctypes.c_int32(0)
    for c in _all_splitk_cases():
        used.value = -1
        p = lib.sbev_linear_splitk_path(c.M, c.N, c.K, c.splits, ctypes.byref(used))
        assert p == C.SPLITK_PATHS.index(c.path), (c, p)
        seen.add(p)
        want = {'REGTILE_FOLD2': c.splits // 2, 'REGTILE_FOLD1': c.splits}.get(c.path) or C.expected_slabs_split128(c.K, c.splits)
        assert used.value == want and 1 <= used.value <= c.splits, (c, used.value)
        assert c.N % 4 == 0 and c.N <= 1024 and c.ldx % 4 == 0 and c.ldx >= c.K and c.ldw >= c.K, c
    assert seen == set(range(4))
    # the cases the lists single out
    assert lib.sbev_linear_splitk_path(129, 132, 96, 4, ctypes.byref(used)) == C.SPLITK_PATHS.index('SPLIT128') and used.value == 3
    assert lib.sbev_linear_splitk_path(129, 128, 2048, 65, ctypes.byref(used)) == C.SPLITK_PATHS.index('SPLIT128') and used.value == 64
    assert lib.sbev_linear_splitk_path(129, 128, 2048, 64, ctypes.byref(used)) == C.SPLITK_PATHS.index('REGTILE_FOLD2') and used.value == 32
    assert lib.sbev_linear_splitk_path(129, 128, 2048, 3, None) == C.SPLITK_PATHS.index('REGTILE_FOLD1')          # used may be NULL
    for M, splits in ((1, 3), (49, 3), (1, 6)):                       # wave tasks: ceil(M / 48) x N / 128 x splits, no multiple of 4
        assert any(c.M == M and c.N == 128 and c.splits == splits for c in C.splitk_cases('REGTILE'))
        assert ((M + 47) // 48 * splits) % 4 != 0
    folds = {c.path for c in C.splitk_cases('REGTILE')}
    assert folds == {'REGTILE_FOLD1', 'REGTILE_FOLD2'}
    # a K / 32 that `splits` does not divide, in both kernels: a k-step dropped at a split boundary would show
    assert any((c.K // 32) % c.splits for c in C.splitk_cases('REGTILE')) and any((c.K // 32) % c.splits for c in C.splitk_cases('SPLIT128'))


def test_ln_linear_cases_cover_the_fused_launch_and_the_fallback(lib):
    """the header's rule: one launch when K == 256, M <= 2048 and sbev_linear_f32 runs the shape on its small-tile kernel"""
    small = C.LINEAR_PATHS.index('SMALL256')
    fused = lambda c: c.K == 256 and c.M <= C.LN_FUSE_MAX_ROWS and lib.sbev_linear_f32_path(c.M, c.N, c.K, c.N, 0, 1) == small
    cases = C.ln_linear_cases()
    assert any(fused(c) and c.M == 2048 for c in cases) and any(not fused(c) and c.M == 2049 and c.K == 256 for c in cases)
    assert all(fused(c) == (c.M <= 2048 and c.K == 256) for c in cases)
    assert any(c.K != 256 for c in cases)
    grid = {(c.ln_relu, c.ln_add, c.relu, c.res) for c in cases}
    assert len(grid) == 16


def test_every_epilogue_combination_is_listed():
    for k in ('REGTILE', 'SPLIT128', 'SPLIT128_RAGGED'):
        for path in {c.path for c in C.splitk_cases(k)}:
            assert {(c.bias, c.relu, c.res, c.ln) for c in C.splitk_cases(k) if c.path == path} == set(C.EPILOGUE_GRID), path
    assert {(c.bias, c.relu, c.res, c.ln) for c in C.reduce_cases()} == set(C.EPILOGUE_GRID)
    assert {(c.M, c.N) for c in C.reduce_cases()} == set(C.layer_norm_shapes()) and {c.splits for c in C.reduce_cases()} == set(C.RED_SPLITS)
    for p in C.LINEAR_PATHS:
        cs = C.linear_cases(p)
        assert {c.relu for c in cs} == {0, 1} and {c.bias for c in cs} == {True, False}, p
        if p != 'STRIP':
            assert {c.res for c in cs} == {None, 'aligned', 'offset'}, p
            assert {(c.ldy - c.N, c.yoff) for c in cs} >= set(C.LAYOUTS), p
        else:
            assert {c.ldy - c.N for c in cs} == {0, 4} and {c.ldx for c in cs} == {256, 260}


# ---- the real leg stays away from degenerate rows --------------------------------------------------------------------------------------------
def test_no_layer_norm_row_of_the_real_leg_is_nearly_constant():
    worst = float('inf')
    for c in _all_splitk_cases():
        if c.ln:
            X, W, b, res, _, _ = C.splitk_operands(c, 'real', with_ln=False)
            worst = min(worst, C.row_variance(C.splitk_pre_ln(X, W, b, res, c.relu, xw=C.product(c.M, c.N, c.K, 'real'))).min().item())
    for c in C.reduce_cases():
        if c.ln:
            worst = min(worst, C.row_variance(C.reduce_operands(c, 'real', with_ln=False)[-1]).min().item())
    for M, N in C.layer_norm_shapes():
        worst = min(worst, C.row_variance(C.ln_rows(M, N)).min().item())
    for M in C.LNL_M:
        worst = min(worst, C.row_variance(C.rows(M, 256, 'real')).min().item())
    for M in C.LIN3_M:
        for N in C.LIN3_N:
            x, w, b = C.lin3_case(M, N, 'real')
            worst = min(worst, C.row_variance(C.lin3_ref(x, w, b, *C.ln_params(N))[1]).min().item())
    assert worst > C.MIN_LN_VARIANCE, worst


def test_no_real_leg_reference_is_a_cancelled_handful_of_outputs():
    """max |err| / max |ref| measures the kernel only while some output is as large as the terms it sums"""
    worst = float('inf')
    for c in _all_linear_cases():
        assert c.M * c.N >= 5, c
        worst = min(worst, C.linear_operands(c, 'real')[-1].abs().max().item())
    for c in _all_splitk_cases():
        worst = min(worst, C.splitk_operands(c, 'real', with_ln=False)[-1].abs().max().item())
    for c in C.reduce_cases():
        worst = min(worst, C.reduce_operands(c, 'real', with_ln=False)[-1].abs().max().item())
    assert worst > C.MIN_REAL_REF, worst


# ---- argument validation of the two path functions -------------------------------------------------------------------------------------------
def test_path_functions_refuse_bad_sizes(lib):
    for args in ((0, 8, 32, 8, 0, 1), (-1, 8, 32, 8, 0, 1), (4, 0, 32, 8, 0, 1), (4, 8, 0, 8, 0, 1), (4, 8, -32, 8, 0, 1), (4, 8, 32, 7, 0, 1)):
        assert lib.sbev_linear_f32_path(*args) == -1, args
        assert b'sbev_linear_f32_path' in lib.sbev_last_error()
    used = ctypes.c_int32(77)
    for args in ((0, 8, 64, 1), (4, 0, 64, 1), (4, 8, 0, 1), (4, 8, 64, 0), (4, 8, 64, -2), (-4, 8, 64, 2)):
        assert lib.sbev_linear_splitk_path(*args, ctypes.byref(used)) == -1, args
        assert b'sbev_linear_splitk_path' in lib.sbev_last_error() and used.value == 77
    assert lib.sbev_linear_f32_path(1, 1, 1, 1, 0, 0) == C.LINEAR_PATHS.index('RAGGED64')
