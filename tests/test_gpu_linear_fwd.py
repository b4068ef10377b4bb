"""The exact-fp32 Linear family's forward kernels at every path their dispatch can take, on integers (bit-equal) and against fp64:
sbev_linear_f32 (strip, ragged 64 x 64, 128 x 128, small 256 / 512, 64 x 64), sbev_linear_splitk_f32 with a chosen `splits` (register
tiles with fold 1 / 2, 128 x 128 split-K tiles plain and ragged), sbev_splitk_reduce_f32, sbev_layer_norm_f32, sbev_ln_linear_f32,
sbev_linear_group_f32 and sbev_linear3_ln_relu(_ex)_f32 -- called through the C ABI with explicit leading dimensions and offset
pointers.  Shapes, inputs and references: tests/linear_fwd_cases.py (checked on the host by tests/test_linear_fwd_host.py).

Every operand lives inside a larger buffer filled with a NaN sentinel: the padding columns [K, ld) of the inputs hold it, so a read of
padding that reaches a product shows; every word of an output buffer outside [M, N] -- the row padding [N, ldy), the rows after row
M - 1, the floats before an offset base -- holds it and must hold it afterwards, bit for bit.  Which kernel a case runs is asked of the
library (sbev_linear_f32_path, sbev_linear_splitk_path) and must be the one the case is listed under."""
import ctypes

import pytest
import torch

import linear_fwd_cases as C
from sparsebev_amd import _lib, dense

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD = 64                                 # sentinel words in front; 256 bytes, so an offset of 0 keeps the allocation's alignment
SENT = 0x7fc5a5a5                        # a quiet NaN with a payload: an element nobody wrote compares unequal to everything
GUARD_ROWS = 8                           # sentinel rows behind the last row
VP = ctypes.c_void_p


class Buf:
    """[rows, ld] floats on the device starting `off` floats past a 16-byte boundary, `cols` of them per row in use; everything else --
    PAD + off words in front, the columns cols .. ld - 1 of every row, GUARD_ROWS rows (at least PAD words) behind -- is sentinel"""

    def __init__(self, rows, cols, ld=None, off=0, init=None):
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 0
        self.rows, self.cols, self.ld = rows, cols, ld
        self.start = PAD + off
        self.raw = torch.full((self.start + rows * ld + max(PAD, GUARD_ROWS * ld),), SENT, dtype=torch.int32, device=DEV)
        self.mat = self.raw[self.start:self.start + rows * ld].view(torch.float32).view(rows, ld)
        if init is not None:
            self.mat[:, :cols] = init.to(DEV).reshape(rows, cols)
        self.ptr = VP(self.raw.data_ptr() + 4 * self.start)

    def values(self):
        return self.mat[:, :self.cols].cpu()

    def intact(self):
        """every word outside [rows, cols] still holds the sentinel"""
        r = self.raw.clone()
        r[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = SENT
        return bool((r == SENT).all())


def ptr(b):
    return b.ptr if b is not None else None


def ok(st, key):
    assert st == 0, (key, _lib.load().sbev_last_error())


def check(got, ref, leg, tol, worst, name, key):
    """integer leg: bit-equal; real leg: under the bound, the worst value kept for the report"""
    if leg == 'int':
        assert torch.equal(got, ref.float()), (key, leg, (got.double() - ref).abs().max().item())
    else:
        e = C.rel_err(got, ref)
        worst[name] = max(worst.get(name, 0.0), e)
        assert e < tol, (key, leg, e, tol)


def report(worst):
    for k, v in sorted(worst.items()):
        print('measured worst %-44s %.2e' % (k, v))


# ---- sbev_linear_f32 ------------------------------------------------------------------------------------------------------------------------
def _linear_call(lib, c, X, W, b, res, key):
    """one sbev_linear_f32 call of a LinCase; returns Y's values after checking the status and every sentinel"""
    Xb, Wb = Buf(c.M, c.K, c.ldx, init=X), Buf(c.N, c.K, c.ldw, init=W)
    bb = Buf(1, c.N, init=b) if b is not None else None
    rb = Buf(c.M, c.N, c.ldy, off=1 if c.res == 'offset' else 0, init=res) if res is not None else None
    Yb = Buf(c.M, c.N, c.ldy, off=c.yoff)
    ok(lib.sbev_linear_f32(Xb.ptr, Wb.ptr, ptr(bb), ptr(rb), Yb.ptr, c.M, c.N, c.K, c.ldx, c.ldw, c.ldy, c.relu, None), key)
    torch.cuda.synchronize()
    for buf in (Yb, Xb, Wb, bb, rb):
        assert buf is None or buf.intact(), (key, 'sentinel')
    return Yb.values()


def _run_linear_cases(cases, name):
    lib = _lib.load()
    worst = {}
    for c in cases:
        path = lib.sbev_linear_f32_path(c.M, c.N, c.K, c.ldy, int(c.res is not None), int(c.yoff % 4 == 0))
        assert path == C.LINEAR_PATHS.index(c.path), (c, path)
        for leg in ('int', 'real'):
            X, W, b, res, ref = C.linear_operands(c, leg)
            got = _linear_call(lib, c, X, W, b, res, (c, leg))
            check(got, ref, leg, C.TOL, worst, 'sbev_linear_f32 ' + name, c)
    report(worst)


@pytest.mark.parametrize('path', C.LINEAR_PATHS)
def test_linear_f32_every_path(path):
    """every listed shape of the path with strided X / W / Y, the relu x residual (none, aligned, offset) sub-grid, ldy - N in
    {0, 1, 3, 4} x Y offset by 0 / 1 float: the vector and the scalar epilogue"""
    _run_linear_cases(C.linear_cases(path), path)


def test_linear_f32_strip_shapes_that_leave_the_strip_kernel():
    """the strip kernel's shapes with a residual, ldy = N + 1 or an offset Y, and N one tile short of it: the path function says
    where they go, and they are still exact"""
    _run_linear_cases(C.strip_leavers(), 'strip leavers')


# ---- sbev_linear_splitk_f32 with `splits` given -------------------------------------------------------------------------------------------------
def _splitk_call(lib, c, X, W, b, res, ln, key):
    Xb, Wb = Buf(c.M, c.K, c.ldx, init=X), Buf(c.N, c.K, c.ldw, init=W)
    bb = Buf(1, c.N, init=b) if b is not None else None
    rb = Buf(c.M, c.N, init=res) if res is not None else None
    gb, hb = (Buf(1, c.N, init=ln[0]), Buf(1, c.N, init=ln[1])) if ln is not None else (None, None)
    Yb = Buf(c.M, c.N)
    nbytes = lib.sbev_linear_splitk_workspace(c.M, c.N, c.splits)
    assert nbytes == 4 * c.M * c.N * c.splits
    ws = Buf(1, nbytes // 4)
    ok(lib.sbev_linear_splitk_f32(Xb.ptr, Wb.ptr, ptr(bb), ptr(rb), ptr(gb), ptr(hb), C.EPS, Yb.ptr, c.M, c.N, c.K, c.ldx, c.ldw,
                                  c.relu, c.splits, ws.ptr, None), key)
    torch.cuda.synchronize()
    for buf in (Yb, ws, Xb, Wb, bb, rb, gb, hb):
        assert buf is None or buf.intact(), (key, 'sentinel')
    return Yb.values(), ws


@pytest.mark.parametrize('kernel', ['REGTILE', 'SPLIT128', 'SPLIT128_RAGGED'])
def test_linear_splitk_f32_every_path(kernel):
    """integer leg without the LayerNorm (bit-equal through every split plan, fold and slab sum, and the slabs the path function
    announces are the ones written); real leg without and, where the case has one, with the LayerNorm.  relu + LayerNorm together is the
    documented LN(relu(XW^T + b) + res)."""
    lib = _lib.load()
    worst = {}
    used = ctypes.c_int32(0)
    for c in C.splitk_cases(kernel):
        path = lib.sbev_linear_splitk_path(c.M, c.N, c.K, c.splits, ctypes.byref(used))
        assert path == C.SPLITK_PATHS.index(c.path), (c, path)
        for leg, with_ln in (('int', False), ('real', False)) + ((('real', True),) if c.ln else ()):
            X, W, b, res, ln, ref = C.splitk_operands(c, leg, with_ln)
            got, ws = _splitk_call(lib, c, X, W, b, res, ln, (c, leg, with_ln))
            check(got, ref, leg, C.TOL_LN if ln is not None else C.TOL, worst,
                  'sbev_linear_splitk_f32 %s%s' % (c.path, ' + LayerNorm' if ln is not None else ''), (c, with_ln))
            if leg == 'int':        # exactly `used` slabs were written, and they add up to X W^T
                slabs = ws.mat.view(c.splits, c.M, c.N).cpu()
                written = slabs[:used.value]
                assert not torch.isnan(written).any() and torch.isnan(slabs[used.value:]).all(), (c, used.value)
                assert torch.equal(written.double().sum(0), C.product(c.M, c.N, c.K, 'int')), c
    report(worst)


# ---- sbev_splitk_reduce_f32 ------------------------------------------------------------------------------------------------------------------
def test_splitk_reduce_f32_from_synthetic_slabs():
    lib = _lib.load()
    worst = {}
    for c in C.reduce_cases():
        for leg, with_ln in (('int', False), ('real', False)) + ((('real', True),) if c.ln else ()):
            S, b, res, ln, ref = C.reduce_operands(c, leg, with_ln)
            Sb = Buf(c.splits * c.M, c.N, init=S)
            bb = Buf(1, c.N, init=b) if b is not None else None
            rb = Buf(c.M, c.N, init=res) if res is not None else None
            gb, hb = (Buf(1, c.N, init=ln[0]), Buf(1, c.N, init=ln[1])) if ln is not None else (None, None)
            Yb = Buf(c.M, c.N)
            key = (c, leg, with_ln)
            ok(lib.sbev_splitk_reduce_f32(Sb.ptr, c.splits, ptr(bb), ptr(rb), ptr(gb), ptr(hb), C.EPS, Yb.ptr, c.M, c.N, c.relu, None), key)
            torch.cuda.synchronize()
            for buf in (Yb, Sb, bb, rb, gb, hb):
                assert buf is None or buf.intact(), (key, 'sentinel')
            check(Yb.values(), ref, leg, C.TOL_LN if ln is not None else C.TOL, worst,
                  'sbev_splitk_reduce_f32%s' % (' + LayerNorm' if ln is not None else ''), key)
    report(worst)


# ---- sbev_layer_norm_f32 ----------------------------------------------------------------------------------------------------------------------
def test_layer_norm_f32_every_width_with_a_large_mean():
    """relu x add_after at every (M, N); rows = 3 randn + 100.  Here the ReLU is the LayerNorm's: relu(LN(x)) + add_after."""
    lib = _lib.load()
    worst = {}
    for M, N in C.layer_norm_shapes():
        x, (gam, bet), add = C.ln_rows(M, N), C.ln_params(N), C.matrix(M, N, 'real', 'add')
        gb, hb = Buf(1, N, init=gam), Buf(1, N, init=bet)
        for relu in (0, 1):
            for with_add in (0, 1):
                Xb, Ab, Yb = Buf(M, N, init=x), (Buf(M, N, init=add) if with_add else None), Buf(M, N)
                key = (M, N, relu, with_add)
                ok(lib.sbev_layer_norm_f32(Xb.ptr, gb.ptr, hb.ptr, C.EPS, ptr(Ab), Yb.ptr, M, N, relu, None), key)
                torch.cuda.synchronize()
                for buf in (Yb, Xb, Ab, gb, hb):
                    assert buf is None or buf.intact(), (key, 'sentinel')
                check(Yb.values(), C.layer_norm_ref(x, gam, bet, relu, add if with_add else None), 'real', C.TOL_LN, worst,
                      'sbev_layer_norm_f32', key)
    report(worst)


# ---- sbev_ln_linear_f32 ------------------------------------------------------------------------------------------------------------------------
def test_ln_linear_f32_fused_and_fallback():
    """M up to 2048 in one launch, 2049 and every K != 256 in two (the header's rule, asked of sbev_linear_f32_path).  Xn and Y against
    fp64; Y bit-equal to sbev_linear_f32 on the stored Xn (the prologue changes where the rows come from, not the GEMM); the rows of Xn
    past M stay sentinel."""
    lib = _lib.load()
    worst = {}
    small = C.LINEAR_PATHS.index('SMALL256')
    for c in C.ln_linear_cases():
        fused = c.K == 256 and c.M <= C.LN_FUSE_MAX_ROWS and lib.sbev_linear_f32_path(c.M, c.N, c.K, c.N, 0, 1) == small
        assert fused == (c.M <= 2048 and c.K == 256), c
        X, W, b = C.rows(c.M, c.K, 'real'), C.weights(c.N, c.K, 'real'), C.vector(c.N, 'real')
        gam, bet = C.ln_params(c.K)
        add = C.matrix(c.M, c.K, 'real', 'add') if c.ln_add else None
        res = C.matrix(c.M, c.N, 'real') if c.res else None
        xn_ref, y_ref = C.ln_linear_ref(X, gam, bet, c.ln_relu, add, W, b, res, c.relu)
        Xb, Xn, Ab = Buf(c.M, c.K, init=X), Buf(c.M, c.K), (Buf(c.M, c.K, init=add) if add is not None else None)
        gb, hb, Wb, bb = Buf(1, c.K, init=gam), Buf(1, c.K, init=bet), Buf(c.N, c.K, c.ldw, init=W), Buf(1, c.N, init=b)
        rb = Buf(c.M, c.N, c.ldy, init=res) if res is not None else None
        Yb, Y2 = Buf(c.M, c.N, c.ldy), Buf(c.M, c.N, c.ldy)
        ok(lib.sbev_ln_linear_f32(Xb.ptr, gb.ptr, hb.ptr, C.EPS, c.ln_relu, ptr(Ab), Xn.ptr, Wb.ptr, bb.ptr, ptr(rb), Yb.ptr,
                                  c.M, c.N, c.K, c.ldw, c.ldy, c.relu, None), c)
        ok(lib.sbev_linear_f32(Xn.ptr, Wb.ptr, bb.ptr, ptr(rb), Y2.ptr, c.M, c.N, c.K, c.K, c.ldw, c.ldy, c.relu, None), c)
        torch.cuda.synchronize()
        for buf in (Yb, Y2, Xn, Xb, Ab, gb, hb, Wb, bb, rb):
            assert buf is None or buf.intact(), (c, 'sentinel')
        name = 'sbev_ln_linear_f32 ' + ('one launch' if fused else 'two launches')
        check(Xn.values(), xn_ref, 'real', C.TOL_LN, worst, name + ', Xn', c)
        check(Yb.values(), y_ref, 'real', C.TOL_LN, worst, name + ', Y', c)
        assert torch.equal(Yb.values(), Y2.values()), c
    report(worst)


# ---- sbev_linear_group_f32 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', sorted(C.GROUPS))
def test_linear_group_f32_three_problems_in_one_launch(K):
    """different M, N and leading dimensions side by side: each output bit-equal to its single launch and, on integers, to the reference"""
    lib = _lib.load()
    worst = {}
    group = C.GROUPS[K]
    for leg in ('int', 'real'):
        arr = (dense._LinearProblem * len(group))()
        bufs, singles, refs = [], [], []
        for i, c in enumerate(group):
            X, W, b, res, ref = C.linear_operands(c, leg)
            singles.append(_linear_call(lib, c, X, W, b, res, (c, leg, 'single')))
            refs.append(ref)
            Xb, Wb = Buf(c.M, c.K, c.ldx, init=X), Buf(c.N, c.K, c.ldw, init=W)
            bb = Buf(1, c.N, init=b) if b is not None else None
            rb = Buf(c.M, c.N, c.ldy, off=1 if c.res == 'offset' else 0, init=res) if res is not None else None
            Yb = Buf(c.M, c.N, c.ldy, off=c.yoff)
            bufs.append((Yb, Xb, Wb, bb, rb))
            arr[i] = dense._LinearProblem(Xb.ptr.value, Wb.ptr.value, bb.ptr.value if bb else None, rb.ptr.value if rb else None, Yb.ptr.value,
                                          c.M, c.N, c.K, c.ldx, c.ldw, c.ldy, c.relu)
        ok(lib.sbev_linear_group_f32(ctypes.cast(arr, VP), len(group), None), (K, leg))
        torch.cuda.synchronize()
        for c, bs, single, ref in zip(group, bufs, singles, refs):
            for buf in bs:
                assert buf is None or buf.intact(), (c, leg, 'sentinel')
            got = bs[0].values()
            assert torch.equal(got, single), (c, leg)
            check(got, ref, leg, C.TOL, worst, 'sbev_linear_group_f32 K=%d' % K, c)
    report(worst)


# ---- sbev_linear3_ln_relu_f32 / _ex ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ex', [False, True], ids=['plain', 'ex'])
def test_linear3_ln_relu_f32_every_width(ex):
    """x [M, ldx] with only its first 3 columns read (the others hold NaN); y against fp64; `pre` of _ex = the Linear's rows before the
    LayerNorm, bit-equal on integers (and NULL is allowed); both entry points give the same y"""
    lib = _lib.load()
    worst = {}
    for M in C.LIN3_M:
        for N in C.LIN3_N:
            gam, bet = C.ln_params(N)
            gb, hb = Buf(1, N, init=gam), Buf(1, N, init=bet)
            for ldx in C.LIN3_LDX:
                for leg in ('int', 'real'):
                    x, w, b = C.lin3_case(M, N, leg)
                    y_ref, pre_ref = C.lin3_ref(x, w, b, gam, bet)
                    Xb, Wb, bb, Yb = Buf(M, 3, ldx, init=x), Buf(N, 3, init=w), Buf(1, N, init=b), Buf(M, N)
                    Pb = Buf(M, N) if ex else None
                    key = (M, N, ldx, leg)
                    if ex:
                        ok(lib.sbev_linear3_ln_relu_ex_f32(Xb.ptr, ldx, Wb.ptr, bb.ptr, gb.ptr, hb.ptr, C.EPS, Yb.ptr, Pb.ptr, M, N, None), key)
                    else:
                        ok(lib.sbev_linear3_ln_relu_f32(Xb.ptr, ldx, Wb.ptr, bb.ptr, gb.ptr, hb.ptr, C.EPS, Yb.ptr, M, N, None), key)
                    torch.cuda.synchronize()
                    for buf in (Yb, Pb, Xb, Wb, bb, gb, hb):
                        assert buf is None or buf.intact(), (key, 'sentinel')
                    check(Yb.values(), y_ref, 'real', C.TOL_LN, worst, 'sbev_linear3_ln_relu%s_f32 y (%s inputs)' % ('_ex' if ex else '', leg), key)
                    if ex:
                        check(Pb.values(), pre_ref, leg, C.TOL, worst, 'sbev_linear3_ln_relu_ex_f32 pre', key)
                        Y0 = Buf(M, N)                       # pre = NULL: the plain kernel's result
                        ok(lib.sbev_linear3_ln_relu_ex_f32(Xb.ptr, ldx, Wb.ptr, bb.ptr, gb.ptr, hb.ptr, C.EPS, Y0.ptr, None, M, N, None), key)
                        torch.cuda.synchronize()
                        assert Y0.intact() and torch.equal(Y0.values(), Yb.values()), key
    report(worst)


# ---- the split-image out-projections forward their relu to the reducer ------------------------------------------------------------------------------
def _out_proj_case():
    M, N, K = 33, 256, 256                  # the smallest K sbev_linear_bf16s_out_ok accepts
    X, W, b, res = C.rows(M, K, 'real'), C.weights(N, K, 'real'), C.vector(N, 'real'), C.matrix(M, N, 'real')
    gam, bet = C.ln_params(N)
    return X, W, b, res, gam, bet, C.splitk_ref(X, W, b, res, (gam, bet), True)


def test_linear_splitk_bf16s_relu_before_residual_and_layer_norm():
    """relu + residual + LayerNorm through dense.linear_splitk_bf16s = LN(relu(XW^T + b) + res), to the absolute 2e-5 of its LayerNorm
    case in test_gpu_bf16s.py::test_out_projection_bf16x6_not_narrower_than_f32_mfma"""
    X, W, b, res, gam, bet, ref = _out_proj_case()
    d = lambda t: t.to(DEV)
    y = dense.linear_splitk_bf16s(d(X), dense.pack_bf16s_frags(d(W), 3), d(b), nimg=3, residual=d(res), ln=(d(gam), d(bet)), relu=True)
    e = (y.cpu().double() - ref).abs().max().item()
    print('measured linear_splitk_bf16s relu + residual + LayerNorm: max |err| %.2e' % e)
    assert e < 2e-5, e


def test_linear_splitk_f16s_relu_before_residual_and_layer_norm():
    """the same through dense.linear_splitk_f16s, to the absolute 5e-3 of its LayerNorm case in
    test_gpu_bf16s.py::test_out_projection_f16_not_narrower_than_f32_mfma"""
    X, W, b, res, gam, bet, ref = _out_proj_case()
    d = lambda t: t.to(DEV)
    wf, wsc = dense.pack_f16s_frags(d(W))
    y = dense.linear_splitk_f16s(d(X), wf, wsc, d(b), nprod=3, residual=d(res), ln=(d(gam), d(bet)), relu=True)
    e = (y.cpu().double() - ref).abs().max().item()
    print('measured linear_splitk_f16s relu + residual + LayerNorm: max |err| %.2e' % e)
    assert e < 5e-3, e


def test_dense_linear_relu_and_layer_norm_is_one_function_on_both_routes():
    """dense.linear(relu=True, ln=...) = LN(relu(x w^T + b) + residual) below and above the split-K threshold; ln_relu on the split-K
    route is refused before anything is launched"""
    for K in (512, 2048):
        M, N = 33, 256
        X, W, b, res = C.rows(M, K, 'real'), C.weights(N, K, 'real'), C.vector(N, 'real'), C.matrix(M, N, 'real')
        gam, bet = C.ln_params(N)
        d = lambda t: t.to(DEV)
        y = dense.linear(d(X), d(W), d(b), relu=True, residual=d(res), ln=(d(gam), d(bet)))
        e = C.rel_err(y, C.splitk_ref(X, W, b, res, (gam, bet), True))
        assert e < C.TOL_LN, (K, e)
    with pytest.raises(RuntimeError, match='ln_relu with split-K'):
        dense.linear(d(X), d(W), d(b), ln=(d(gam), d(bet)), ln_relu=True)
