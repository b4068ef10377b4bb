"""The row-wise half of the training step against fp64, at every path its kernels can take: sbev_bias_relu_bwd (one pass up to
ONE_PASS_ROWS rows, two passes above), sbev_layer_norm_bwd (all widths, both column paths), the grouped launches sbev_colsum_group and
sbev_layer_norm_param_group, and sbev_gemm_f32_multi -- called through the C ABI, so that what is measured is the kernel's own error.
Shapes, inputs and references: tests/backward_rows_cases.py (checked on the host by tests/test_backward_rows_host.py).

Integer leg: bit-equal to the exact integer result.  Real leg: max |err| / max |ref| < 2e-5 against fp64.  Every buffer a kernel writes
sits between sentinel words (and has sentinel guard columns where ld > N), every workspace has the size the library's own *_workspace
function states and is followed by sentinels: none of them may change."""
import ctypes

import pytest
import torch

import backward_rows_cases as C
from sparsebev_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD = 64                                 # sentinel words on either side; 256 bytes, so the body keeps the allocation's alignment
SENT = 0x7fc5a5a5                        # a quiet NaN with a payload: an output element nobody wrote compares unequal to everything
VP = ctypes.c_void_p


class Buf:
    """[rows, ld] floats on the device, `cols` of them per row in use; sentinels before, after and in the columns cols .. ld - 1"""

    def __init__(self, rows, cols, ld=None, init=None):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld = rows, cols, ld
        self.raw = torch.full((2 * PAD + rows * ld,), SENT, dtype=torch.int32, device=DEV)
        self.mat = self.raw[PAD:PAD + rows * ld].view(torch.float32).view(rows, ld)
        if init is not None:
            self.mat[:, :cols] = init.to(DEV).reshape(rows, cols)
        self.ptr = VP(self.raw.data_ptr() + 4 * PAD)

    def values(self):
        return self.mat[:, :self.cols].cpu()

    def vector(self):
        return self.values().reshape(-1)

    def bits(self):
        return self.raw.clone()

    def intact(self):
        body = self.raw[PAD:PAD + self.rows * self.ld].view(self.rows, self.ld)
        return bool((self.raw[:PAD] == SENT).all() & (self.raw[PAD + self.rows * self.ld:] == SENT).all() & (body[:, self.cols:] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


def workspace(nbytes):
    assert nbytes >= 0 and nbytes % 4 == 0
    return Buf(1, nbytes // 4)


def ok(st):
    assert st == 0, _lib.load().sbev_last_error()


def check(got, ref, leg, worst, key):
    """integer leg: bit-equal; real leg: under the bound, the worst value kept for the report"""
    if leg == 'int':
        assert torch.equal(got, ref.float()), (key, (got.double() - ref).abs().max().item())
    else:
        e = C.rel_err(got, ref)
        worst[key] = max(worst.get(key, 0.0), e)
        assert e < C.TOL, (key, e)


def report(worst):
    for k, v in sorted(worst.items()):
        print('measured worst %-40s %.2e' % (k, v))


# ---- sbev_bias_relu_bwd ----------------------------------------------------------------------------------------------------------------
def _bias_call(lib, dY, Y, dZ, db, M, N, ld, ws, accumulate, plain):
    p = lambda b: b.ptr if b is not None else None
    if plain:
        return lib.sbev_bias_relu_bwd(p(dY), p(Y), p(dZ), p(db), M, N, ld, p(ws), None)
    return lib.sbev_bias_relu_bwd_acc(p(dY), p(Y), p(dZ), p(db), M, N, ld, p(ws), accumulate, None)


@pytest.mark.parametrize('M,N', C.bias_shapes())
def test_bias_relu_bwd_every_argument_both_legs(M, N):
    """Y NULL / given (with +0, -0 and denormals), ld = N / N + 4, dZ separate / aliasing dY / NULL, db written / added to / NULL (then
    without a workspace), through sbev_bias_relu_bwd and sbev_bias_relu_bwd_acc.  dZ is a masked copy: bit-exact in both legs.
    measured worst db error (real leg, max |err| / max |ref|): one pass 2.4e-7, two passes 4.3e-7."""
    lib = _lib.load()
    worst = {}
    path = 'one pass' if M <= 2048 else 'two passes'
    for leg in ('int', 'real'):
        for with_y in (False, True):
            dY, Y, db0 = C.bias_case(M, N, leg, with_y)
            dZ_ref, db_ref = C.bias_relu_ref(dY, Y)
            _, db_acc_ref = C.bias_relu_ref(dY, Y, db0)
            first = None
            for ld in (N, N + 4):
                Yb = Buf(M, N, ld, Y) if with_y else None
                for dz_mode in ('separate', 'alias', 'null'):
                    for db_mode in ('write', 'add', 'null'):
                        dYb = Buf(M, N, ld, dY)
                        dZb = {'separate': Buf(M, N, ld), 'alias': dYb, 'null': None}[dz_mode]
                        dbb = None if db_mode == 'null' else Buf(1, N, init=db0 if db_mode == 'add' else None)
                        ws = None if db_mode == 'null' else workspace(lib.sbev_colsum_workspace(M, N))
                        # the plain entry point where it can express the call; _acc with accumulate = 0 for the aliasing ones
                        ok(_bias_call(lib, dYb, Yb, dZb, dbb, M, N, ld, ws, int(db_mode == 'add'), plain=db_mode != 'add' and dz_mode != 'alias'))
                        torch.cuda.synchronize()
                        key = (leg, with_y, ld, dz_mode, db_mode)
                        if dZb is not None:
                            assert torch.equal(dZb.values(), dZ_ref.float()), key
                        if dz_mode != 'alias':
                            assert torch.equal(dYb.values(), dY), key
                        if dbb is not None:
                            check(dbb.vector(), db_acc_ref if db_mode == 'add' else db_ref, leg, worst, 'bias_relu_bwd db, ' + path)
                        for b in (dYb, dZb, dbb, ws, Yb):
                            assert b is None or b.intact(), key
                        if dz_mode == 'separate' and db_mode == 'write':       # the same call again (other ld included): the same bits
                            now = (dZb.values(), dbb.vector())
                            first = first or now
                            assert torch.equal(first[0], now[0]) and torch.equal(first[1].view(torch.int32), now[1].view(torch.int32)), key
    report(worst)


@pytest.mark.parametrize('N', [1, 65, 256])
def test_bias_relu_bwd_no_rows(N):
    """M = 0: db = 0, or unchanged under accumulate; nothing else is touched"""
    lib = _lib.load()
    db0 = torch.arange(1, N + 1).float()
    for accumulate in (0, 1):
        dYb, dZb, dbb, ws = Buf(0, N), Buf(0, N), Buf(1, N, init=db0), workspace(lib.sbev_colsum_workspace(0, N))
        ok(lib.sbev_bias_relu_bwd_acc(dYb.ptr, None, dZb.ptr, dbb.ptr, 0, N, N, ws.ptr, accumulate, None))
        torch.cuda.synchronize()
        assert torch.equal(dbb.vector(), db0 if accumulate else torch.zeros(N))
        assert dYb.untouched() and dZb.untouched() and ws.untouched() and dbb.intact()
    dbb = Buf(1, N)
    ok(lib.sbev_bias_relu_bwd(dYb.ptr, None, None, dbb.ptr, 0, N, N, ws.ptr, None))
    torch.cuda.synchronize()
    assert torch.equal(dbb.vector(), torch.zeros(N)) and dbb.intact()


# ---- sbev_layer_norm_bwd -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', C.ln_shapes())
def test_layer_norm_bwd_vs_fp64(M, N):
    """relu on / off, parameter gradients written (sbev_layer_norm_bwd) and added to (sbev_layer_norm_bwd_acc); sbev_layer_norm_bwd_rows
    gives the same dX bit for bit and leaves the (mean, rstd) rows; a repeated call gives the same bits.
    measured worst (max |err| / max |ref|): dX 2.1e-7; dgamma 3.0e-7 (one pass), 5.4e-7 (two passes); dbeta 2.9e-7, 3.1e-7; mean 1.4e-7; rstd 1.3e-7."""
    lib = _lib.load()
    worst = {}
    path = 'one pass' if M <= 2048 else 'two passes'
    for relu in (0, 1):
        c = C.ln_case(M, N, relu)
        dYb, Xb, gb, bb = Buf(M, N, init=c['dY']), Buf(M, N, init=c['X']), Buf(1, N, init=c['gamma']), Buf(1, N, init=c['beta'])
        beta_ptr = bb.ptr if relu else None                      # beta is only read for the mask
        seen = []
        for accumulate in (0, 1, 0):
            ref = C.layer_norm_ref(c['dY'], c['X'], c['gamma'], c['beta'], relu, *((c['dgamma_before'], c['dbeta_before']) if accumulate else ()))
            dXb = Buf(M, N)
            dgb, dbb = (Buf(1, N, init=c[k] if accumulate else None) for k in ('dgamma_before', 'dbeta_before'))
            ws = workspace(lib.sbev_layer_norm_bwd_workspace(M, N))
            if accumulate:
                ok(lib.sbev_layer_norm_bwd_acc(dYb.ptr, Xb.ptr, gb.ptr, beta_ptr, C.EPS, relu, dXb.ptr, dgb.ptr, dbb.ptr, ws.ptr, M, N, 1, None))
            elif seen:
                ok(lib.sbev_layer_norm_bwd_acc(dYb.ptr, Xb.ptr, gb.ptr, bb.ptr, C.EPS, relu, dXb.ptr, dgb.ptr, dbb.ptr, ws.ptr, M, N, 0, None))
            else:
                ok(lib.sbev_layer_norm_bwd(dYb.ptr, Xb.ptr, gb.ptr, beta_ptr, C.EPS, relu, dXb.ptr, dgb.ptr, dbb.ptr, ws.ptr, M, N, None))
            torch.cuda.synchronize()
            key = (relu, accumulate)
            check(dXb.values(), ref['dX'], 'real', worst, 'layer_norm_bwd dX')
            check(dgb.vector(), ref['dgamma'], 'real', worst, 'layer_norm_bwd dgamma, ' + path)
            check(dbb.vector(), ref['dbeta'], 'real', worst, 'layer_norm_bwd dbeta, ' + path)
            for b in (dXb, dgb, dbb, ws, dYb, Xb, gb, bb):
                assert b.intact(), key
            if not accumulate:
                seen.append((dXb.bits(), dgb.bits(), dbb.bits()))
        assert all(torch.equal(a, b) for a, b in zip(*seen)), 'two identical calls differ'
        # the first half alone: the same dX, and the statistics the grouped launch reads
        dXb, st = Buf(M, N), Buf(M, 2)
        ok(lib.sbev_layer_norm_bwd_rows(dYb.ptr, Xb.ptr, gb.ptr, beta_ptr, C.EPS, relu, dXb.ptr, st.ptr, M, N, None))
        torch.cuda.synchronize()
        assert torch.equal(dXb.bits(), seen[0][0]) and dXb.intact() and st.intact()
        check(st.values()[:, 0], ref['mean'], 'real', worst, 'layer_norm_bwd_rows mean')
        check(st.values()[:, 1], ref['rstd'], 'real', worst, 'layer_norm_bwd_rows rstd')
        assert torch.equal(dYb.values(), c['dY']) and torch.equal(Xb.values(), c['X'])
    report(worst)


# ---- sbev_colsum_group ---------------------------------------------------------------------------------------------------------------------
def _colsum_group(lib, M, leg, widths, nsegs, accs, worst):
    groups = C.colsum_group_case(M, leg, tuple(widths), tuple(nsegs))
    ng = len(groups)
    segs, outs = (VP * (ng * 8))(), (VP * ng)()
    Ns, ns_, acc_ = (ctypes.c_int32 * ng)(*widths), (ctypes.c_int32 * ng)(*nsegs), (ctypes.c_int32 * ng)(*accs)
    seg_bufs, out_bufs = [], []
    for i, ((mats, out0), N, acc) in enumerate(zip(groups, widths, accs)):
        bufs = [Buf(M, N, init=m) for m in mats]
        out = Buf(1, N, init=out0 if acc else None)
        for k, b in enumerate(bufs):
            segs[i * 8 + k] = b.ptr.value
        outs[i] = out.ptr.value
        seg_bufs.append(bufs)
        out_bufs.append(out)
    ok(lib.sbev_colsum_group(segs, outs, Ns, ns_, acc_, ng, M, None))
    torch.cuda.synchronize()
    for i, ((mats, out0), N, acc) in enumerate(zip(groups, widths, accs)):
        check(out_bufs[i].vector(), C.colsum_group_ref(mats, out0 if acc else None), leg, worst, 'colsum_group')
        assert out_bufs[i].intact() and all(b.intact() for b in seg_bufs[i]), (i, N)
    return [o.bits() for o in out_bufs]


@pytest.mark.parametrize('M', C.COLSUM_GROUP_M)
def test_colsum_group_sixteen_biases_and_one(M):
    """one launch over 16 biases of widths 1 .. 776 with 1 .. 8 segments each and mixed accumulate flags -- the integer leg is bit-equal
    per group, which is what proves the block offsets and the row tails -- and the single group with a single segment.
    measured worst (real leg, max |err| / max |ref|): 9.3e-7."""
    lib = _lib.load()
    worst = {}
    for leg in ('int', 'real'):
        a = _colsum_group(lib, M, leg, C.COLSUM_WIDTHS, C.COLSUM_NSEGS, C.COLSUM_ACC, worst)
        b = _colsum_group(lib, M, leg, C.COLSUM_WIDTHS, C.COLSUM_NSEGS, C.COLSUM_ACC, worst)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two identical calls differ'
        for N in (1, 65, 776):
            for acc in (0, 1):
                _colsum_group(lib, M, leg, [N], [1], [acc], worst)
    report(worst)


# ---- sbev_layer_norm_param_group -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', C.LN_GROUP_M)
def test_layer_norm_param_group_vs_fp64_and_vs_per_segment_calls(M):
    """8 LayerNorms (widths 4 .. 1024, relu and accumulate mixed, 1 .. 8 segments) in one launch, the statistics from
    sbev_layer_norm_bwd_rows as autograd._group_ln_grads takes them; against fp64, and against the per-segment
    sbev_layer_norm_bwd_acc calls added up (another summation order: to the bound, not bit for bit).
    measured worst (max |err| / max |ref|): dgamma 7.5e-7, dbeta 5.7e-7; against the per-segment calls 7.4e-7."""
    lib = _lib.load()
    worst = {}
    groups = C.ln_group_case(M)
    ng = len(groups)
    dYs, Xs, Ss = (VP * (ng * 8))(), (VP * (ng * 8))(), (VP * (ng * 8))()
    gam, bet, dgs, dbs = (VP * ng)(), (VP * ng)(), (VP * ng)(), (VP * ng)()
    Ns, nsegs, relus, accs = [(ctypes.c_int32 * ng)() for _ in range(4)]
    keep, outs, singles = [], [], []
    for i, grp in enumerate(groups):
        N, relu, acc = grp['gamma'].shape[0], grp['relu'], grp['accumulate']
        gb, bb = Buf(1, N, init=grp['gamma']), Buf(1, N, init=grp['beta'])
        dgb, dbb = (Buf(1, N, init=grp[k] if acc else None) for k in ('dgamma_before', 'dbeta_before'))
        sg, sb = (Buf(1, N, init=grp[k] if acc else torch.zeros(N)) for k in ('dgamma_before', 'dbeta_before'))     # the per-segment calls' sums
        for k, (dY, X) in enumerate(grp['segs']):
            dYb, Xb, dXb, st = Buf(M, N, init=dY), Buf(M, N, init=X), Buf(M, N), Buf(M, 2)
            ok(lib.sbev_layer_norm_bwd_rows(dYb.ptr, Xb.ptr, gb.ptr, bb.ptr, C.EPS, relu, dXb.ptr, st.ptr, M, N, None))
            ws = workspace(lib.sbev_layer_norm_bwd_workspace(M, N))
            ok(lib.sbev_layer_norm_bwd_acc(dYb.ptr, Xb.ptr, gb.ptr, bb.ptr, C.EPS, relu, dXb.ptr, sg.ptr, sb.ptr, ws.ptr, M, N, 1, None))
            dYs[i * 8 + k], Xs[i * 8 + k], Ss[i * 8 + k] = dYb.ptr.value, Xb.ptr.value, st.ptr.value
            keep += [dYb, Xb, dXb, st, ws]
        gam[i], bet[i], dgs[i], dbs[i] = gb.ptr.value, bb.ptr.value, dgb.ptr.value, dbb.ptr.value
        Ns[i], nsegs[i], relus[i], accs[i] = N, len(grp['segs']), relu, acc
        keep += [gb, bb, sg, sb]
        outs.append((dgb, dbb))
        singles.append((sg, sb))
    bits = []
    for _ in range(2):
        if bits:                                         # the second launch starts from the same buffers
            for grp, (dgb, dbb) in zip(groups, outs):
                if grp['accumulate']:
                    dgb.mat[0] = grp['dgamma_before'].to(DEV)
                    dbb.mat[0] = grp['dbeta_before'].to(DEV)
        ok(lib.sbev_layer_norm_param_group(dYs, Xs, Ss, gam, bet, dgs, dbs, Ns, nsegs, relus, accs, ng, M, None))
        torch.cuda.synchronize()
        bits.append([b.bits() for pair in outs for b in pair])
    assert all(torch.equal(a, b) for a, b in zip(*bits)), 'two identical calls differ'
    for grp, (dgb, dbb), (sg, sb) in zip(groups, outs, singles):
        dg_ref, db_ref, _ = C.ln_group_ref(grp)
        check(dgb.vector(), dg_ref, 'real', worst, 'layer_norm_param_group dgamma')
        check(dbb.vector(), db_ref, 'real', worst, 'layer_norm_param_group dbeta')
        check(dgb.vector(), sg.vector().double(), 'real', worst, 'layer_norm_param_group vs per-segment calls')
        check(dbb.vector(), sb.vector().double(), 'real', worst, 'layer_norm_param_group vs per-segment calls')
        assert dgb.intact() and dbb.intact()
    assert all(b.intact() for b in keep)
    report(worst)


# ---- one entry point stated through another ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 260, 1024])
@pytest.mark.parametrize('M', [1, 17, 33, 900, 2048])
def test_layer_norm_bwd_one_pass_is_the_grouped_launch_of_one_segment(M, N):
    """up to ONE_PASS_ROWS rows sbev_layer_norm_bwd_acc's dgamma / dbeta are, bit for bit, what sbev_layer_norm_bwd_rows followed by
    sbev_layer_norm_param_group with one group of one segment gives on the same buffers: relu on / off, written / added to"""
    lib = _lib.load()
    for relu in (0, 1):
        c = C.ln_case(M, N, relu)
        dYb, Xb, gb, bb = Buf(M, N, init=c['dY']), Buf(M, N, init=c['X']), Buf(1, N, init=c['gamma']), Buf(1, N, init=c['beta'])
        for acc in (0, 1):
            got = {}
            for how in ('acc', 'group'):
                dXb = Buf(M, N)
                dgb, dbb = (Buf(1, N, init=c[k] if acc else None) for k in ('dgamma_before', 'dbeta_before'))
                ws = workspace(lib.sbev_layer_norm_bwd_workspace(M, N))
                if how == 'acc':
                    ok(lib.sbev_layer_norm_bwd_acc(dYb.ptr, Xb.ptr, gb.ptr, bb.ptr, C.EPS, relu, dXb.ptr, dgb.ptr, dbb.ptr, ws.ptr, M, N, acc, None))
                else:
                    ok(lib.sbev_layer_norm_bwd_rows(dYb.ptr, Xb.ptr, gb.ptr, bb.ptr, C.EPS, relu, dXb.ptr, ws.ptr, M, N, None))
                    one = lambda b: (VP * 8)(b.ptr.value)
                    i32 = lambda v: (ctypes.c_int32 * 1)(v)
                    ok(lib.sbev_layer_norm_param_group(one(dYb), one(Xb), one(ws), _ptrs([gb]), _ptrs([bb]), _ptrs([dgb]), _ptrs([dbb]),
                                                       i32(N), i32(1), i32(relu), i32(acc), 1, M, None))
                torch.cuda.synchronize()
                assert all(b.intact() for b in (dXb, dgb, dbb, ws)), (relu, acc, how)
                got[how] = (dXb.bits(), dgb.bits(), dbb.bits())
            assert all(torch.equal(a, b) for a, b in zip(got['acc'], got['group'])), (relu, acc)


@pytest.mark.parametrize('N', [1, 65, 776])
@pytest.mark.parametrize('M', [1, 17, 65, 2048])
def test_bias_column_sum_against_colsum_group_of_one_segment(M, N):
    """sbev_bias_relu_bwd without Y and dZ is a plain column sum, as is sbev_colsum_group with one group of one segment: 4 rows per trip
    against 8, so two different trees -- bit-equal on the integer leg, to the bound on the real leg.
    measured worst (real leg, max |difference| / max |colsum_group|): 2.3e-7."""
    lib = _lib.load()
    worst = {}
    for leg in ('int', 'real'):
        dY, _, _ = C.bias_case(M, N, leg, False)
        dYb, dbb, out = Buf(M, N, init=dY), Buf(1, N), Buf(1, N)
        ws = workspace(lib.sbev_colsum_workspace(M, N))
        ok(lib.sbev_bias_relu_bwd(dYb.ptr, None, None, dbb.ptr, M, N, N, ws.ptr, None))
        i32 = lambda v: (ctypes.c_int32 * 1)(v)
        ok(lib.sbev_colsum_group((VP * 8)(dYb.ptr.value), _ptrs([out]), i32(N), i32(1), i32(0), 1, M, None))
        torch.cuda.synchronize()
        check(dbb.vector(), out.vector().double(), leg, worst, 'bias_relu_bwd db vs colsum_group')
        assert all(b.intact() for b in (dYb, dbb, out, ws)) and torch.equal(dYb.values(), dY)
    report(worst)


# ---- sbev_gemm_f32_multi -------------------------------------------------------------------------------------------------------------------
def _ptrs(bufs):
    return (VP * len(bufs))(*[b.ptr.value for b in bufs])


def _operands(case, nseg, ak, bk):
    A, B, _, _ = case
    As = [C.stored(a, ak, True) for a in A[:nseg]]
    Bs = [C.stored(b, bk, False) for b in B[:nseg]]
    return [Buf(*a.shape, init=a) for a in As], [Buf(*b.shape, init=b) for b in Bs]


def _gemm_multi(lib, case, M, N, K, nseg, ak, bk, accumulate, Ab, Bb):
    C0 = case[2]
    Cb = Buf(M, N, N + 3, init=C0 if accumulate else None)
    ws = workspace(lib.sbev_gemm_f32_multi_workspace(M, N, K, nseg))
    ok(lib.sbev_gemm_f32_multi(_ptrs(Ab), ak, Ab[0].ld, _ptrs(Bb), bk, Bb[0].ld, nseg, Cb.ptr, N + 3, M, N, K, accumulate, ws.ptr, None))
    torch.cuda.synchronize()
    assert Cb.intact() and ws.intact() and all(b.intact() for b in Ab + Bb), (ak, bk, accumulate)
    return Cb


@pytest.mark.parametrize('nseg', C.GEMM_NSEGS)
@pytest.mark.parametrize('M,N,K', C.GEMM_MULTI_SHAPES)
def test_gemm_f32_multi_layouts_segments_both_legs(M, N, K, nseg):
    """the four operand layouts, C written and added to at ldc = N + 3; one segment is sbev_gemm_f32's result bit for bit on the integer leg.
    measured worst (real leg, max |err| / max |ref|): 3.9e-7."""
    lib = _lib.load()
    worst = {}
    for leg in ('int', 'real'):
        case = C.gemm_case(M, N, K, leg)
        for ak, bk in C.LAYOUTS:
            Ab, Bb = _operands(case, nseg, ak, bk)
            for accumulate in (0, 1):
                Cb = _gemm_multi(lib, case, M, N, K, nseg, ak, bk, accumulate, Ab, Bb)
                check(Cb.values(), C.gemm_ref(case, nseg, accumulate), leg, worst, 'gemm_f32_multi')
                again = _gemm_multi(lib, case, M, N, K, nseg, ak, bk, accumulate, Ab, Bb)
                assert torch.equal(Cb.bits(), again.bits()), 'two identical calls differ'
                if nseg == 1 and leg == 'int':
                    one = Buf(M, N, N + 3, init=case[2] if accumulate else None)
                    ws = workspace(lib.sbev_gemm_f32_workspace(M, N, K))
                    ok(lib.sbev_gemm_f32(Ab[0].ptr, ak, Ab[0].ld, Bb[0].ptr, bk, Bb[0].ld, one.ptr, N + 3, M, N, K, accumulate, ws.ptr, None))
                    torch.cuda.synchronize()
                    assert torch.equal(one.bits(), Cb.bits()) and ws.intact()
    report(worst)


@pytest.mark.parametrize('ak,bk', C.LAYOUTS)
def test_gemm_f32_multi_one_segment_off_alignment(ak, bk):
    """every size allows the float4 staging, but one segment's pointer sits 4 bytes off a 16-byte boundary: the library has to take the
    element-wise staging for the launch, and stay exact"""
    lib = _lib.load()
    M, N, K, nseg = 256, 256, 64, 3
    case = C.gemm_case(M, N, K, 'int')
    for which in ('A', 'B'):
        Ab, Bb = _operands(case, nseg, ak, bk)
        src = (Ab if which == 'A' else Bb)[1]
        moved = Buf(1, src.rows * src.ld + 1)
        moved.mat[0, 1:] = src.mat.reshape(-1)
        ptrs = [_ptrs(Ab), _ptrs(Bb)]
        ptrs[which == 'B'][1] = moved.ptr.value + 4
        assert (moved.ptr.value + 4) % 16 == 4
        Cb = Buf(M, N, N + 3)
        ws = workspace(lib.sbev_gemm_f32_multi_workspace(M, N, K, nseg))
        ok(lib.sbev_gemm_f32_multi(ptrs[0], ak, Ab[0].ld, ptrs[1], bk, Bb[0].ld, nseg, Cb.ptr, N + 3, M, N, K, 0, ws.ptr, None))
        torch.cuda.synchronize()
        assert torch.equal(Cb.values(), C.gemm_ref(case, nseg, 0).float()), which
        assert Cb.intact() and ws.intact() and moved.intact()


@pytest.mark.parametrize('M,N', [(1, 5), (130, 129), (256, 256)])
def test_gemm_with_no_k_writes_zero_or_leaves_c(M, N):
    """K = 0 is an empty sum: sbev_gemm_f32 and sbev_gemm_f32_multi return OK with C = 0, or C unchanged under accumulate"""
    lib = _lib.load()
    C0 = torch.arange(M * N).float().reshape(M, N) + 1
    some = Buf(1, 4, init=torch.zeros(4))
    for ak, bk in C.LAYOUTS:
        lda, ldb = (M if ak else 4), (N if bk else 4)
        for accumulate in (0, 1):
            want = C0 if accumulate else torch.zeros(M, N)
            Cb = Buf(M, N, N + 3, init=C0)
            ok(lib.sbev_gemm_f32(some.ptr, ak, lda, some.ptr, bk, ldb, Cb.ptr, N + 3, M, N, 0, accumulate, None, None))
            torch.cuda.synchronize()
            assert torch.equal(Cb.values(), want) and Cb.intact()
            for nseg in (1, 3, 8):
                Cb = Buf(M, N, N + 3, init=C0)
                ws = workspace(lib.sbev_gemm_f32_multi_workspace(M, N, 0, nseg))
                segs = (VP * nseg)(*[some.ptr.value] * nseg)
                ok(lib.sbev_gemm_f32_multi(segs, ak, lda, segs, bk, ldb, nseg, Cb.ptr, N + 3, M, N, 0, accumulate, ws.ptr, None))
                torch.cuda.synchronize()
                assert torch.equal(Cb.values(), want) and Cb.intact() and ws.untouched()
