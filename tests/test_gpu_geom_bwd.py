"""The sampling geometry's backward kernels through the C ABI, per output column against fp64: sbev_project_select_bwd,
sbev_sampling_front_bwd and sbev_refine_bbox_bwd (csrc/backward_ops.hip), which the training path reaches only through
autograd.Sampling and autograd.RefineBbox.  Inputs, fp64 references and the reasoning behind every bound: tests/geom_bwd_cases.py
(checked on the host by tests/test_geom_bwd_host.py, which also shows that the oracle differentiated in float32 meets these bounds and
that eight wrong variants of the references break them).

Every buffer a kernel writes sits between sentinel words and has sentinel guard columns where its rows are wider than the payload:
none of them may change.  Each test prints the worst figure it measured per column; one run is kept in profiles/geom_bwd_columns.json."""
import ctypes

import pytest
import torch

import geom_bwd_cases as C
from sparsebev_amd import _lib
from sparsebev_amd.utils import VERSION
from test_gpu_backward_rows import DEV, VP, Buf, ok

pytestmark = pytest.mark.gpu


def report(worst):
    """worst: key -> (kernel error, fp32-oracle error, kernel error / bound); the errors in the unit the key names"""
    for k, (e, e32, share) in sorted(worst.items()):
        print('measured worst %-46s kernel %.3e  fp32 oracle %.3e  kernel / oracle %7.3f  kernel / bound %.4f'
              % (k, e, e32, e / e32 if e32 > 0 else float('nan'), share))


def _ptr(buf):
    return buf.ptr if buf is not None else None


def _shifted(buf, words):
    return VP(buf.ptr.value + 4 * words)


# ---- sbev_project_select_bwd ---------------------------------------------------------------------------------------------------------
def _project_call(lib, c, gpts):
    B, Q, T, N, G, P = c['dims']
    ins = [Buf(B * Q * T * G * P, 3, init=c['pts']), Buf(B * T * N, 16, init=c['l2i']), Buf(B * T * G * Q * P, 3, init=c['gloc'])]
    st = lib.sbev_project_select_bwd(ins[0].ptr, ins[1].ptr, ins[2].ptr, B, Q, T, N, G, P, C.IMAGE_H, C.IMAGE_W, C.EPS, _ptr(gpts), None)
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins)
    return st


@pytest.mark.parametrize('name', C.PROJECT_CASES)
def test_project_select_bwd_per_element_vs_fp64(name):
    """|got - ref| <= 16 U A per element, A the sum of the absolute values of the element's three terms (U = 2^-24): camera counts 1, 2,
    3 and 6, a point count that is no multiple of the block, and by construction no hit (hm above and below eps), two hits, a hit in
    the last camera only, hm in (eps, 2 eps) and u, v exactly 0 or 1 in the first camera.
    measured worst |err| / (U A) per component: kernel 2.65, 3.17, 2.61; the float32 oracle's autograd 2.01, 2.75, 2.61."""
    lib = _lib.load()
    c = C.project_case(name)
    B, Q, T, N, G, P = c['dims']
    gpts = Buf(B * Q * T * G * P, 3)
    ok(_project_call(lib, c, gpts))
    assert gpts.intact()
    got = gpts.values().reshape(B, Q, T, G * P, 3)
    g32 = C.project_oracle_autograd(c['pts'], c['l2i'], c['gloc'], C.EPS, C.IMAGE_H, C.IMAGE_W, torch.float32)
    worst = {}
    for k in range(3):
        e, e32 = (C.project_excess(t[..., k], c['ref'][..., k], c['A'][..., k]) for t in (got, g32))
        worst['project_select_bwd gpts[%d] |err| / (U A)' % k] = (e, e32, e / C.PROJECT_FACTOR)
    report(worst)
    assert all(share <= 1 for _, _, share in worst.values()), worst
    again = Buf(B * Q * T * G * P, 3)
    ok(_project_call(lib, c, again))
    assert torch.equal(again.bits(), gpts.bits()), 'two identical calls differ'


# ---- sbev_sampling_front_bwd ---------------------------------------------------------------------------------------------------------
class FrontCall:
    """the buffers of one sbev_sampling_front_bwd call in one of the three layouts of geom_bwd_cases.FRONT_CASES"""

    def __init__(self, dims, layout, inputs, null=None):
        B, Q, T, G, P, L = dims
        self.dims, GP, BQ = dims, G * P, B * Q
        self.n_off = n_off = GP * 3
        self.ld_off, self.ld_logit, self.ld_grad, self.packed = C.front_layout(layout, GP, L)
        offset, logits = inputs['offset'].reshape(BQ, n_off), inputs['logits'].reshape(BQ, GP * L)
        self.bbox = Buf(BQ, 10, init=inputs['bbox'])
        if self.packed:                                      # offsets | logits in one row, and the same for the gradient
            both, gboth = Buf(BQ, n_off + GP * L, self.ld_off, init=torch.cat([offset, logits], 1)), Buf(BQ, n_off + GP * L, self.ld_grad)
            self.off_ptr, self.lg_ptr, self.goff_ptr, self.glog_ptr = both.ptr, _shifted(both, n_off), gboth.ptr, _shifted(gboth, n_off)
            self.ins, self.outs = [both], [gboth]
        else:
            self.ins = [Buf(BQ, n_off, self.ld_off, init=offset), Buf(BQ, GP * L, self.ld_logit, init=logits)]
            self.outs = [Buf(BQ, n_off, self.ld_grad), Buf(BQ, GP * L, self.ld_grad)]
            self.off_ptr, self.lg_ptr, self.goff_ptr, self.glog_ptr = self.ins[0].ptr, self.ins[1].ptr, self.outs[0].ptr, self.outs[1].ptr
        self.gpts = Buf(BQ * T * GP, 3, init=inputs['gpts']) if null != 'gpts' else None
        self.gw = Buf(B * G * T * Q * P, L, init=inputs['gw_bp']) if null != 'gw_bp' else None
        self.gbbox = Buf(BQ, 10) if null != 'gbbox' else None
        self.ins += [b for b in (self.bbox, self.gpts, self.gw) if b is not None]
        self.outs += [self.gbbox] if self.gbbox is not None else []
        self.pc = (ctypes.c_double * 6)(*C.PC_RANGE)

    def run(self, lib, **override):
        a = dict(bbox=self.bbox.ptr, off=self.off_ptr, lg=self.lg_ptr, pc=self.pc, dims=self.dims, gpts=_ptr(self.gpts), gw=_ptr(self.gw),
                 goff=self.goff_ptr, glog=self.glog_ptr, ld_grad=self.ld_grad, gbbox=_ptr(self.gbbox))
        a.update(override)
        st = lib.sbev_sampling_front_bwd(a['bbox'], a['off'], self.ld_off, a['lg'], self.ld_logit, a['pc'], *a['dims'], a['gpts'], a['gw'],
                                         a['goff'], a['glog'], a['ld_grad'], a['gbbox'], None)
        torch.cuda.synchronize()
        return st

    def results(self):
        """(goffset [B,Q,GP,3], glogits [B,Q,GP,L], gbbox [B,Q,10] -- zeros when the call has none) on the host"""
        B, Q, T, G, P, L = self.dims
        v = self.outs[0].values() if self.packed else torch.cat([self.outs[0].values(), self.outs[1].values()], 1)
        gb = self.gbbox.values().reshape(B, Q, 10) if self.gbbox is not None else torch.zeros(B, Q, 10)
        return v[:, :self.n_off].reshape(B, Q, G * P, 3), v[:, self.n_off:].reshape(B, Q, G * P, L), gb

    def intact(self):
        return all(b.intact() for b in self.ins + self.outs)

    def untouched(self):
        return all(b.untouched() for b in self.outs)


class box_convention:
    """rot_sign = -1 is the 'v0.17.1' box convention, which the library reads at launch time"""

    def __init__(self, rot_sign):
        self.name = C.version_of(rot_sign)

    def __enter__(self):
        VERSION.name = self.name

    def __exit__(self, *exc):
        VERSION.name = 'v1.0.0'


@pytest.mark.parametrize('null', C.FRONT_NULLS, ids=lambda n: 'null-%s' % n)
@pytest.mark.parametrize('name', list(C.FRONT_CASES))
def test_sampling_front_bwd_per_column_vs_fp64(name, null):
    """Per column -- the 8 box columns, the three offset components, the logits per level index --: e = max |got - ref| is at most
    max(4 e32, 16 U s), e32 the error of the float32 oracle's autograd on that column and s = max |ref|.  B * Q in {1, 3, 4, 5, 18, 257}
    (a block holds 4 queries), G * P in {1, 16, 32, 63, 64} (one wave), T in {1, 2, 15}, L in {1, 4, 5}, both rotation signs, the packed
    layout of autograd.Sampling with and without guard columns and three unrelated wider buffers; grad_points, grad_weights_bp and
    grad_bbox null in turn.  Exact zeros: box columns 8 and 9 always, the offsets and box columns 0 .. 7 without grad_points, the
    logits without grad_weights_bp.
    measured worst e / bound over all cases: 0.45 (bbox[5], 3.0 x the float32 oracle's error there); the yaw columns 0.19 and 0.25, the
    offsets at most 0.19, the logits at most 0.22.  Every column: profiles/geom_bwd_columns.json.
    This test found the yaw columns of case bq3-gp16 at 1.10 and 1.12 of their bounds (1.9e-6 and 2.7e-6, 4.8 and 7.7 x the float32
    oracle's error) while the kernel took cos and sin through the rounded fp32 angle; it now takes them as c / r and s / r."""
    lib = _lib.load()
    B, Q, T, G, P, L, layout, rot_sign = C.FRONT_CASES[name]
    c = C.front_case(name, null if null != 'gbbox' else None)
    call = FrontCall((B, Q, T, G, P, L), layout, C.front_inputs(name), null)
    with box_convention(rot_sign):
        ok(call.run(lib))
        first = [o.bits() for o in call.outs]
        ok(call.run(lib))
    assert all(torch.equal(a, o.bits()) for a, o in zip(first, call.outs)), 'two identical calls differ'
    assert call.intact()
    goff, glog, gbbox = call.results()
    assert bool((gbbox[..., 8:] == 0).all())
    if null == 'gpts':
        assert bool((goff == 0).all()) and bool((gbbox == 0).all())
    if null == 'gw_bp':
        assert bool((glog == 0).all())
    worst = {}
    for k, (e, e32, s, bound) in C.front_column_errors((goff, glog, gbbox), c['ref'], c['oracle32']).items():
        if null == 'gbbox' and k.startswith('bbox'):
            continue
        worst['sampling_front_bwd %s max |err|' % k] = (e, e32, e / bound if bound > 0 else float(e > 0))
    report(worst)
    assert all(share <= 1 for _, _, share in worst.values()), worst


# ---- sbev_refine_bbox_bwd ------------------------------------------------------------------------------------------------------------
def _rel_units(got, ref):
    """max |got - ref| / (U |ref|) over the elements with ref != 0; got must be 0 exactly where ref is"""
    got, nz = got.double(), ref != 0
    assert torch.equal(got != 0, nz)
    return ((got - ref).abs()[nz] / (C.U * ref.abs()[nz])).max().item() if bool(nz.any()) else 0.0


@pytest.mark.parametrize('with_grad_bbox', [True, False], ids=['grad_bbox', 'no-grad_bbox'])
@pytest.mark.parametrize('with_vel_div', [True, False], ids=['vel_div', 'no-vel_div'])
@pytest.mark.parametrize('name', list(C.REFINE_CASES))
def test_refine_bbox_bwd_per_element_vs_fp64(name, with_vel_div, with_grad_bbox):
    """B * Q in {1, 255, 256, 257} around the 256-thread block.  Columns 0 .. 2 of grad_reg (the sigmoid) and of grad_bbox (the clamped
    inverse sigmoid): |got - ref| <= 8 U |ref| per element, and at the proposal coordinates on the clamp's comparisons -- 0, 1,
    float32(1e-5), 1 - 1e-5, their float32 neighbours, a negative value, a value above 1 -- exactly the reference's elements are zero.
    Columns 3 .. 7 are grad_out bit for bit, columns 8 and 9 the float32 quotient by vel_div[b] bit for bit (grad_out without vel_div);
    grad_bbox columns 3 .. 9 are zero.
    measured worst |err| / (U |ref|): grad_reg 2.19 (float32 oracle 2.11), grad_bbox 3.46 (float32 oracle 3.26)."""
    lib = _lib.load()
    B, Q = C.REFINE_CASES[name]
    c = C.refine_case(name)
    vd = c['vel_div'] if with_vel_div else None
    ref_reg, ref_bbox = C.refine_bwd_ref(c['gout'], c['out32'], c['bbox'], vd)
    _, greg32, gbbox32 = C.refine_oracle(c['bbox'], c['reg'], vd, c['gout'], torch.float32)
    ins = [Buf(B * Q, 10, init=c['gout']), Buf(B * Q, 10, init=c['out32']), Buf(B * Q, 10, init=c['bbox'])]
    vdb = Buf(1, B, init=vd) if with_vel_div else None
    greg, gbbox = Buf(B * Q, 10), (Buf(B * Q, 10) if with_grad_bbox else None)
    ok(lib.sbev_refine_bbox_bwd(ins[0].ptr, ins[1].ptr, ins[2].ptr, _ptr(vdb), greg.ptr, _ptr(gbbox), B, Q, None))
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins + [greg]) and (vdb is None or vdb.intact()) and (gbbox is None or gbbox.intact())
    got = greg.values().reshape(B, Q, 10)
    assert torch.equal(got[..., 3:8], c['gout'][..., 3:8])
    assert torch.equal(got[..., 8:], c['gout'][..., 8:] / vd[:, None, None] if with_vel_div else c['gout'][..., 8:])
    e, e32 = _rel_units(got[..., :3], ref_reg[..., :3]), _rel_units(greg32[..., :3], ref_reg[..., :3])
    worst = {'refine_bbox_bwd grad_reg[0:3] |err| / (U |ref|)': (e, e32, e / C.REFINE_FACTOR)}
    if with_grad_bbox:
        gb = gbbox.values().reshape(B, Q, 10)
        assert bool((gb[..., 3:] == 0).all())
        assert torch.equal(gb[..., :3][c['edge']] == 0, ref_bbox[..., :3][c['edge']] == 0)
        e, e32 = _rel_units(gb[..., :3], ref_bbox[..., :3]), _rel_units(gbbox32[..., :3], ref_bbox[..., :3])
        worst['refine_bbox_bwd grad_bbox[0:3] |err| / (U |ref|)'] = (e, e32, e / C.REFINE_FACTOR)
    report(worst)
    assert all(share <= 1 for _, _, share in worst.values()), worst


# ---- what the entry points refuse, and the empty call ---------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone_and_empty_calls_return_ok():
    """G * P = 65 (more than a wave), L = 6, ld_grad below either payload and a null required pointer return nonzero and write nothing;
    B = 0 or Q = 0 is an empty call that needs no pointer at all"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)

    def front_call(B, Q, T, G, P, L, layout):
        """buffers that really have the stated sizes, whether the library accepts them or not"""
        rand = lambda *s: torch.rand(*s, generator=g) + 0.25
        return FrontCall((B, Q, T, G, P, L), layout, dict(bbox=rand(B, Q, 10), offset=rand(B, Q, G * P, 3), logits=rand(B, Q, G * P, L),
                                                          gpts=rand(B, Q, T, G * P, 3), gw_bp=rand(B * G * T, Q, P, L)))

    def refused(call, **override):
        assert call.run(lib, **override) != 0 and lib.sbev_last_error()
        assert call.untouched() and call.intact()

    refused(front_call(2, 3, 2, 5, 13, 4, 'wide'))           # G * P = 65: more than a wave
    refused(front_call(2, 3, 2, 4, 4, 6, 'packed'))          # L = 6
    B, Q, T, G, P, L = 2, 3, 2, 4, 4, 4
    call = front_call(B, Q, T, G, P, L, 'wide')
    refused(call, ld_grad=G * P * 3 - 1)
    refused(call, ld_grad=G * P * L - 1)
    refused(front_call(B, Q, T, G, P, 2, 'wide'), ld_grad=G * P * 3 - 1)          # wide enough for the logits alone
    for required in ('bbox', 'off', 'lg', 'pc', 'goff', 'glog'):
        refused(call, **{required: None})
    refused(call, dims=(B, Q, 0, G, P, L))
    for dims in ((0, Q, T, G, P, L), (B, 0, T, G, P, L)):
        ok(lib.sbev_sampling_front_bwd(None, None, 0, None, 0, None, *dims, None, None, None, None, 0, None, None))
    torch.cuda.synchronize()
    assert call.untouched()
    ok(call.run(lib))                                        # the same buffers are a valid call
    assert not call.untouched() and call.intact()

    c = C.project_case('one-camera')
    pB, pQ, pT, pN, pG, pP = c['dims']
    n = pB * pQ * pT * pG * pP
    bufs = [Buf(n, 3, init=c['pts']), Buf(pB * pT * pN, 16, init=c['l2i']), Buf(n, 3, init=c['gloc']), Buf(n, 3)]
    for k in range(4):
        ptrs = [b.ptr for b in bufs]
        ptrs[k] = None
        assert lib.sbev_project_select_bwd(*ptrs[:3], pB, pQ, pT, pN, pG, pP, C.IMAGE_H, C.IMAGE_W, C.EPS, ptrs[3], None) != 0
    ptrs = [b.ptr for b in bufs]
    assert lib.sbev_project_select_bwd(*ptrs[:3], pB, pQ, pT, 0, pG, pP, C.IMAGE_H, C.IMAGE_W, C.EPS, ptrs[3], None) != 0      # no camera
    for dims in ((0, pQ), (pB, 0)):
        ok(lib.sbev_project_select_bwd(None, None, None, *dims, pT, pN, pG, pP, C.IMAGE_H, C.IMAGE_W, C.EPS, None, None))
    torch.cuda.synchronize()
    assert bufs[3].untouched() and all(b.intact() for b in bufs)

    ins, greg, gbbox = [Buf(4, 10, init=torch.rand(4, 10, generator=g)) for _ in range(3)], Buf(4, 10), Buf(4, 10)
    for k in range(4):
        ptrs = [b.ptr for b in ins] + [greg.ptr]
        ptrs[k] = None
        assert lib.sbev_refine_bbox_bwd(*ptrs[:3], None, ptrs[3], gbbox.ptr, 2, 2, None) != 0
    for dims in ((0, 2), (2, 0)):
        ok(lib.sbev_refine_bbox_bwd(None, None, None, None, None, None, *dims, None))
    torch.cuda.synchronize()
    assert greg.untouched() and gbbox.untouched()


# ---- the autograd nodes pass exactly these calls ------------------------------------------------------------------------------------------
@torch.enable_grad()
def test_autograd_nodes_are_the_c_entries_called_by_hand():
    """autograd.Sampling.backward returns, bit for bit, what sbev_project_select_bwd and sbev_sampling_front_bwd give when called here on
    the same recomputed points, grad_loc and grad_weights with the node's packed row width and its 4 * n_off pointer offset; the same for
    autograd.RefineBbox and sbev_refine_bbox_bwd"""
    from sparsebev_amd import autograd as AG, dense, ops, synthetic as S
    from sparsebev_amd.transformer import DecoderContext, FeaturePyramid
    lib = _lib.load()
    B, Q, T, G, P, L = 2, 9, 2, 4, 4, 4
    ih, iw, sizes = S.PYRAMIDS['tiny']
    g = torch.Generator().manual_seed(11)
    bbox, _ = S.make_queries(B, Q, seed=7)
    both = torch.randn(B, Q, G * P * (3 + L), generator=g) * 0.5
    gy = torch.randn(B, Q, G, T * P, 64, generator=g).to(DEV)
    pyr = FeaturePyramid([f.to(DEV) for f in S.make_features(B, T, sizes, seed=8)])
    dctx = DecoderContext(S.make_img_metas(B, T, ih, iw), B, torch.device(DEV))
    bd, sd = bbox.to(DEV).requires_grad_(True), both.to(DEV).requires_grad_(True)
    AG.Sampling.apply(bd, sd, pyr, dctx, (T, G, P, L, tuple(S.PC_RANGE)), None).backward(gy)
    n_off, ld = G * P * 3, G * P * (3 + L)
    with torch.no_grad():
        bb, packed = bd.detach().contiguous(), sd.detach().contiguous()
        pts, w_bp = ops.sampling_front(bb, packed[..., :n_off], packed[..., n_off:], dctx.time_diff, S.PC_RANGE, T, G, P, L)
        loc = ops.project_select(pts, dctx.lidar2img, dctx.image_h, dctx.image_w, G, P)
        gloc, gw = pyr.sample_backward(loc, w_bp, gy.contiguous(), T, G, None)
        p = lambda t: VP(t.data_ptr())
        gpts, gboth, gbbox = Buf(B * Q * T * G * P, 3), Buf(B * Q, ld), Buf(B * Q, 10)
        ok(lib.sbev_project_select_bwd(p(pts), p(dctx.lidar2img.contiguous()), p(gloc), B, Q, T, ops.N_VIEWS, G, P,
                                       float(dctx.image_h), float(dctx.image_w), 1e-5, gpts.ptr, None))
        pc = (ctypes.c_double * 6)(*S.PC_RANGE)
        ok(lib.sbev_sampling_front_bwd(p(bb), p(packed), ld, VP(packed.data_ptr() + 4 * n_off), ld, pc, B, Q, T, G, P, L,
                                       gpts.ptr, p(gw), gboth.ptr, _shifted(gboth, n_off), ld, gbbox.ptr, None))
        torch.cuda.synchronize()
        assert gpts.intact() and gboth.intact() and gbbox.intact()
        assert torch.equal(bd.grad.cpu().reshape(B * Q, 10), gbbox.values()) and torch.equal(sd.grad.cpu().reshape(B * Q, ld), gboth.values())
        assert bd.grad.abs().max() > 0 and sd.grad[..., :n_off].abs().max() > 0 and sd.grad[..., n_off:].abs().max() > 0

    reg, gout = torch.randn(B, Q, 10, generator=g).to(DEV), torch.randn(B, Q, 10, generator=g).to(DEV)
    vd = torch.tensor([0.5, 2.0], device=DEV)
    prop = torch.rand(B, Q, 10, generator=g)
    prop[0, 0, 0], prop[0, 1, 1], prop[1, 2, 2] = 0.0, 1.0, 1e-5
    bd, rd = prop.to(DEV).requires_grad_(True), reg.clone().requires_grad_(True)
    AG.RefineBbox.apply(bd, rd, vd).backward(gout)
    with torch.no_grad():
        out = dense.refine_bbox(bd.detach(), reg, vd)
        greg, gb = Buf(B * Q, 10), Buf(B * Q, 10)
        ok(lib.sbev_refine_bbox_bwd(p(gout), p(out), p(bd.detach()), p(vd), greg.ptr, gb.ptr, B, Q, None))
        torch.cuda.synchronize()
        assert greg.intact() and gb.intact()
        assert torch.equal(rd.grad.cpu().reshape(B * Q, 10), greg.values()) and torch.equal(bd.grad.cpu().reshape(B * Q, 10), gb.values())
