"""The sampler's backward kernels (csrc/msmv_sampling_bwd.hip) through the C ABI, per instantiation against fp64: sbev_msmv_bwd_ex and
sbev_msmv_bwd over {C = 64 kernel, generic kernel} x L = 1..5 x both grad_out layouts x both pyramid layouts, with channel counts, point
counts and camera counts rotating, one-column and 1 x 1 levels, a pixel stride wider than the row, the forced fall-back of C = 64 to
the generic kernel, one (b', q) item, NaN / Inf / 1e30 coordinates in every cell and feature-gradient buffers that already hold values.
Cells, the fp64 reference in its four admissible definitions and the derivation of the bound: tests/sampler_bwd_cases.py (checked on the
host by tests/test_sampler_bwd_host.py).

Every buffer sits between NaN sentinel words and has sentinel columns where the pixel stride is wider than the row: none may change.
Each test prints the worst error / bound it measured per output with the fp32 restatement's next to it; one run is kept in
profiles/sampler_bwd_matrix.json."""
import ctypes
import types

import pytest
import torch

import sampler_bwd_cases as S
from sparsebev_amd import _lib, ops
from test_gpu_backward_rows import DEV, Buf, ok

pytestmark = pytest.mark.gpu

LAYOUT = {'ref': ops.OUT_REF, 'mix': ops.OUT_MIX}


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr.value for b in bufs])


class Call:
    """the buffers of one backward call of a cell: inputs and descriptor once, fresh outputs per run()"""

    def __init__(self, case):
        self.case, self.cell = case, case['cell']
        c = self.cell
        self.points = c['Bp'] * c['Q'] * c['P']
        self.gdiv, sbo, self.stride_g, sv, self.px = S.descriptor(c)
        self.sbo, self.sv = _i64(sbo), _i64(sv)
        self.hw = (ctypes.c_int32 * (2 * c['L']))(*[v for s in c['sizes'] for v in s])
        self.rows = [S.device_rows(c, f) for f in case['feats']]
        self.pre_rows = [S.device_rows(c, f) for f in case['pre']]
        self.feats = [Buf(r.shape[0], r.shape[1], self.px, init=r) for r in self.rows]
        self.loc = Buf(self.points, 3, init=case['loc'])
        self.wts = Buf(self.points, c['L'], init=case['wts'])
        self.gout = Buf(self.points, c['C'], init=S.device_gout(c, case['gout']))
        self.ins = self.feats + [self.loc, self.wts, self.gout]
        self.in_bits = [b.bits() for b in self.ins]
        if not c['pad'] and self.px < (1 << 20):          # the hand-written descriptor is ops._pyramid's wherever that one applies
            shaped = [r.reshape(-1, h, w, r.shape[1]) for r, (h, w) in zip(self.rows, c['sizes'])]
            _, (gdiv, p_sbo, sg, p_sv, px) = ops._pyramid(shaped, c['N'], c['G'] if c['pyr'] == 'grouped' else None)
            assert (gdiv, list(p_sbo), sg, list(p_sv), px) == (self.gdiv, sbo, self.stride_g, sv, self.px)

    def run(self, lib, entry='ex', feature_grad=True):
        """one call into fresh output buffers -> (grad_loc Buf, grad_weights Buf, feature-gradient Bufs or None)"""
        c = self.cell
        gloc, gw = Buf(self.points, 3), Buf(self.points, c['L'])
        gf = [Buf(r.shape[0], r.shape[1], self.px, init=r) for r in self.pre_rows] if feature_grad else None
        head = (_ptrs(self.feats), _ptrs(gf) if gf else None, self.hw, c['L'], c['Bp'], c['N'], c['C'], c['Q'], c['P'],
                self.gdiv, self.sbo, self.stride_g, self.sv, self.px, self.loc.ptr, self.wts.ptr, self.gout.ptr)
        if entry == 'ex':
            T, G = (c['T'], c['G']) if c['layout'] == 'mix' else (1, 1)
            ok(lib.sbev_msmv_bwd_ex(*head, LAYOUT[c['layout']], T, G, gloc.ptr, gw.ptr, None))
        else:
            ok(lib.sbev_msmv_bwd(*head, gloc.ptr, gw.ptr, None))
        torch.cuda.synchronize()
        assert gloc.intact() and gw.intact() and all(b.intact() for b in gf or []), 'a guard word or a padding column was written'
        assert all(torch.equal(b.bits(), bits) for b, bits in zip(self.ins, self.in_bits)), 'an input changed'
        return gloc, gw, gf

    def host(self, gloc, gw, gf):
        c = self.cell
        return (gloc.values().reshape(c['Bp'], c['Q'], c['P'], 3), gw.values().reshape(c['Bp'], c['Q'], c['P'], c['L']),
                [S.host_level(c, b.values(), l) for l, b in enumerate(gf)] if gf else None)


def _report(name, kernel, worst, own):
    print('sampler_bwd cell %-34s kernel %-7s error / bound: %s' % (name, kernel, '  '.join(
        '%s %.4f (fp32 restatement %.4f)' % (k, worst[k], own[k]) for k in ('grad_loc', 'grad_weights', 'grad_feats'))))


@pytest.mark.parametrize('name', list(S.CELLS))
def test_msmv_bwd_cell_vs_fp64(name):
    """Per element, for at least one of the four admissible definitions of the bilinear fractions: |got - ref| <= (n + 8) U A (n terms
    whose absolute values sum to A; U = 2^-24); exact zeros where A = 0 -- every point with a NaN / Inf coordinate --, grad_loc[..., 2]
    exactly 0; the feature gradient ADDED to what the buffer held, elements without a live tap unchanged bit for bit; guards and
    padding intact; grad_feats = NULL gives the same grad_loc / grad_weights bits and writes no feature; a repeated call and (reference
    layout) sbev_msmv_bwd give the same grad_loc / grad_weights bits.
    measured worst error / bound over all cells (the fp32 restatement's next to it): grad_loc 0.20 (0.23), grad_weights 0.25 (0.27),
    grad_feats 0.29 (0.32).  With the complement of a fraction taken as 1 - fraction, as the kernels did before, cell
    L5-C128-P4-N2-ref-bp-alt missed the grad_feats bound 4.6 times."""
    lib = _lib.load()
    case = S.cell_case(name)
    cell, call = case['cell'], Call(case)
    gloc, gw, gf = call.run(lib)
    h_gloc, h_gw, h_gf = call.host(gloc, gw, gf)
    worst = S.check_outputs(case['refs'], h_gloc, h_gw, h_gf, pre=case['pre'])
    _report(name, S.kernel_of(cell), worst, case['fp32'])
    rows = S.nonfinite_rows(case['loc'])
    assert bool((h_gloc.view(-1, 3)[rows] == 0).all()) and bool((h_gw.view(-1, cell['L'])[rows] == 0).all()), \
        'a point with a non-finite coordinate has a gradient: %s' % h_gw.view(-1, cell['L'])[rows]
    assert all(v <= 1 for v in worst.values()), worst
    # frozen features: the same grad_loc / grad_weights, no feature written (there is no buffer; the inputs are checked in run())
    gloc2, gw2, _ = call.run(lib, feature_grad=False)
    assert torch.equal(gloc2.bits(), gloc.bits()) and torch.equal(gw2.bits(), gw.bits()), 'grad_feats = NULL changes grad_loc / grad_weights'
    # no atomics in grad_loc / grad_weights: a repeated call gives the same bits; its feature gradient is inside the bound again
    gloc3, gw3, gf3 = call.run(lib)
    assert torch.equal(gloc3.bits(), gloc.bits()) and torch.equal(gw3.bits(), gw.bits()), 'two identical calls differ'
    again = S.check_outputs(case['refs'], h_gloc, h_gw, call.host(gloc3, gw3, gf3)[2], pre=case['pre'])
    assert again['grad_feats'] <= 1, again
    if cell['layout'] == 'ref':
        gloc4, gw4, gf4 = call.run(lib, entry='plain')
        assert torch.equal(gloc4.bits(), gloc.bits()) and torch.equal(gw4.bits(), gw.bits()), 'sbev_msmv_bwd differs from sbev_msmv_bwd_ex'
        assert S.check_outputs(case['refs'], h_gloc, h_gw, call.host(gloc4, gw4, gf4)[2], pre=case['pre'])['grad_feats'] <= 1


@pytest.mark.parametrize('layout', ['ref', 'mix'])
@pytest.mark.parametrize('C', [64, 24])
def test_nonfinite_coordinates_give_zero_gradient_and_write_nothing(C, layout):
    """Every point of the call has a NaN, +Inf, -Inf or 1e30 in x or y (plain inputs: every address the kernels form is clamped first).
    The reference reads no level for such a point: grad_loc and grad_weights are exactly 0 and the pre-filled feature gradients keep
    every bit, in the C = 64 kernel as in the generic one.
    measured before the fix: the C = 64 kernel returned 187 NaN in grad_loc and 700 in grad_weights (of 792 and 1056), the generic none."""
    lib = _lib.load()
    cell = S.make_cell('nonfinite-C%d-%s' % (C, layout), 4, C, 4, 6, layout, 'grouped' if layout == 'mix' else 'bp')
    assert S.kernel_of(cell) == ('c64' if C == 64 else 'generic')
    feats, loc, wts, gout, pre = S.make_inputs(cell, seed=1)
    flat = loc.view(-1, 3)
    bad = [float('nan'), float('inf'), float('-inf'), 1e30, -1e30]
    for i in range(flat.shape[0]):
        flat[i, i % 2] = bad[i % 5]
        if i % 7 == 0:
            flat[i, 1 - i % 2] = bad[(i + 2) % 5]
    assert not (torch.isfinite(flat[:, :2]) & (flat[:, :2].abs() < 1e30)).all(1).any()
    call = Call(dict(cell=cell, feats=feats, loc=loc, wts=wts, gout=gout, pre=pre))
    gloc, gw, gf = call.run(lib)
    h_gloc, h_gw, h_gf = call.host(gloc, gw, gf)
    print('non-finite C = %d %s: NaN in grad_loc %d, in grad_weights %d; nonzero %d, %d; feature elements changed %d' % (
        C, layout, int(torch.isnan(h_gloc).sum()), int(torch.isnan(h_gw).sum()), int((h_gloc != 0).sum()), int((h_gw != 0).sum()),
        sum(int((a.view(torch.int32) != b.view(torch.int32)).sum()) for a, b in zip(h_gf, pre))))
    assert bool((h_gloc == 0).all()) and bool((h_gw == 0).all())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(h_gf, pre)), 'a feature gradient was written'
    gloc2, gw2, _ = call.run(lib, feature_grad=False)
    assert bool((gloc2.values() == 0).all()) and bool((gw2.values() == 0).all())


def _entry_bits(lib, feats, N, G, Bp, C, loc, wts, gout, layout, T, Gout):
    """sbev_msmv_bwd_ex by hand on plain device tensors, without feature buffers -> (grad_loc, grad_weights)"""
    gloc, gw = torch.full_like(loc, float('nan')), torch.full_like(wts, float('nan'))
    levels, strides = ops._pyramid(feats, N, G)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    Q, P = loc.shape[1:3]
    ok(lib.sbev_msmv_bwd_ex(levels[0], None, levels[1], levels[2], Bp, N, C, Q, P, *strides, p(loc), p(wts), p(gout), layout, T, Gout, p(gloc), p(gw), None))
    torch.cuda.synchronize()
    return gloc, gw


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('name', ['L4-C64-P8-N6-mix-bp-std', 'L2-C24-P4-N6-ref-bp-std'])
def test_python_entry_points_return_the_c_entrys_bits(name):
    """ops.msmv_sampling_nhwc_backward (both grad_out layouts, with and without feature buffers) and ops.MSMVSampling.backward hand
    back the grad_loc / grad_weights bits of sbev_msmv_bwd_ex called by hand; their feature gradients meet the bound"""
    lib = _lib.load()
    case = S.cell_case(name)
    cell = case['cell']
    Bp, N, C, T, G, B = cell['Bp'], cell['N'], cell['C'], cell['T'], cell['G'], cell['B']
    assert N == ops.N_VIEWS
    loc, wts = case['loc'].to(DEV), case['wts'].to(DEV)
    grouped = [S.to_grouped(f, G).to(DEV) for f in case['feats']]
    for lay in ('ref', 'mix'):
        gout = (S.to_mix(case['gout'], B, T, G).contiguous() if lay == 'mix' else case['gout']).to(DEV)
        want = _entry_bits(lib, grouped, N, G, Bp, C, loc, wts, gout, LAYOUT[lay], T, G)
        assert not torch.isnan(want[0]).any() and not torch.isnan(want[1]).any()
        frozen = ops.msmv_sampling_nhwc_backward(grouped, B, T, G, loc, wts, gout, None, grad_layout=LAYOUT[lay], deterministic=False)
        gf = [torch.zeros_like(f) for f in grouped]
        full = ops.msmv_sampling_nhwc_backward(grouped, B, T, G, loc, wts, gout, gf, grad_layout=LAYOUT[lay], deterministic=False)
        torch.cuda.synchronize()
        for got in (frozen, full):
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), lay
        worst = S.check_outputs(case['refs'], full[0].cpu(), full[1].cpu(), [S.from_grouped(f.cpu(), G, N) for f in gf])
        assert all(v <= 1 for v in worst.values()), worst
    plain = [f.to(DEV) for f in case['feats']]
    gout = case['gout'].to(DEV)
    want = _entry_bits(lib, plain, N, None, Bp, C, loc, wts, gout, ops.OUT_REF, 1, 1)
    ctx = types.SimpleNamespace(saved_tensors=(loc, wts, *plain))
    gloc, gw, *gf = ops.MSMVSampling.backward(ctx, gout)
    torch.cuda.synchronize()
    assert _same_bits(gloc, want[0]) and _same_bits(gw, want[1])
    worst = S.check_outputs(case['refs'], gloc.cpu(), gw.cpu(), [f.cpu() for f in gf])
    _report(name + ' (ops)', S.kernel_of(cell), worst, case['fp32'])
    assert all(v <= 1 for v in worst.values()), worst
