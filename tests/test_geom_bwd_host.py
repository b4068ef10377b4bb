"""What tests/geom_bwd_cases.py promises, checked without a device: each closed-form fp64 reference is torch's fp64 autograd of the
oracle's ops with the fp32 decisions fixed; every edge case hits its edge; the oracle differentiated in float32 stays inside the bounds
tests/test_gpu_geom_bwd.py sets, so a correct fp32 kernel can meet them; and eight deliberately wrong variants of the references break
those per-column bounds, while the aggregate measure of the function test (max |err| / max |ref| over a whole gradient tensor) admits
errors of 2 % to 24 % of the largest yaw and size gradients and does not see a wrong level-weight row at all."""
import numpy as np
import pytest
import torch

import geom_bwd_cases as C
from oracle import sparsebev_oracle as O
from sparsebev_amd import synthetic as S


def assert_close(a, b, scale=None):
    """|a - b| <= 1e-12 |b| per element (or 1e-12 `scale`)"""
    a, b = a.double(), b.double()
    bad = (a - b).abs() > 1e-12 * (b.abs() if scale is None else scale)
    assert not bool(bad.any()), ((a - b).abs().max().item(), int(bad.sum()))


# ---- the references are autograd's gradients --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.PROJECT_CASES)
def test_project_reference_is_fp64_autograd_with_the_view_fixed(name):
    """to 1e-12 of A per element, A the absolute sum of the element's three signed terms: that is what two fp64 evaluations of a
    cancelling sum can agree to.  (Relative to the result itself the worst element, whose terms cancel, is at 2.0e-12.)"""
    c = C.project_case(name)
    auto = C.project_oracle_autograd(c['pts'], c['l2i'], c['gloc'], C.EPS, C.IMAGE_H, C.IMAGE_W, torch.float64)
    assert_close(c['ref'], auto, scale=c['A'])               # three signed terms: relative to their absolute sum
    assert bool((c['A'] >= c['ref'].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('name', list(C.FRONT_CASES))
@pytest.mark.parametrize('null', C.FRONT_NULLS[:3])
def test_front_reference_is_fp64_autograd(name, null):
    """to 1e-12 of the column's maximum per element: an entry is a sum of up to T * G * P signed terms of the column's size.  (Relative
    to the entry itself the worst one, a sum that cancels, is at 1.6e-12.)"""
    B, Q, T, G, P, L, _, rot_sign = C.FRONT_CASES[name]
    c = C.front_case(name, null)
    auto = C.front_oracle_autograd(c['bbox'], c['offset'], c['logits'], c['gpts'], c['gw_bp'], C.PC_RANGE, T, G, P, L, rot_sign, torch.float64)
    for (k, r), a in zip(C.front_columns(*c['ref']).items(), C.front_columns(*auto).values()):
        assert (r - a).abs().max() <= 1e-12 * r.abs().max(), (k, (r - a).abs().max().item())
    assert bool((c['ref'][2][..., 8:] == 0).all())
    if null == 'gpts':
        assert bool((c['ref'][0] == 0).all()) and bool((c['ref'][2] == 0).all())
    if null == 'gw_bp':
        assert bool((c['ref'][1] == 0).all())


@pytest.mark.parametrize('name', list(C.REFINE_CASES))
@pytest.mark.parametrize('with_vel_div', [False, True])
def test_refine_reference_is_fp64_autograd(name, with_vel_div):
    c = C.refine_case(name)
    vd = c['vel_div'] if with_vel_div else None
    out, greg, gbbox = C.refine_oracle(c['bbox'], c['reg'], vd, c['gout'], torch.float64)
    ref_reg, ref_bbox = C.refine_bwd_ref(c['gout'], out, c['bbox'], vd)
    assert_close(ref_reg, greg)
    assert_close(ref_bbox, gbbox)
    # float32 torch takes the same three decisions at every edge value: the same elements are zero
    _, _, gbbox32 = C.refine_oracle(c['bbox'], c['reg'], vd, c['gout'], torch.float32)
    assert torch.equal(gbbox32 == 0, ref_bbox == 0)


# ---- the cases are what they claim --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.PROJECT_MAIN))
def test_project_main_cases_fp32_view_is_the_fp64_view_and_hm_is_at_least_one(name):
    c = C.project_case(name)
    B, Q, T, N, G, P = c['dims']
    v32 = C.project_views(c['pts'], c['l2i'], C.EPS, C.IMAGE_H, C.IMAGE_W, torch.float32)
    v64 = C.project_views(c['pts'], c['l2i'], C.EPS, C.IMAGE_H, C.IMAGE_W, torch.float64)
    assert all(torch.equal(a, b) for a, b in zip(v32, v64))
    with C.oracle_setting(n_views=N):
        uvh, _ = O.project_points(c['pts'], c['l2i'], C.IMAGE_H, C.IMAGE_W, C.EPS)
    assert uvh[..., 2].min() >= 1.0
    valid, view, _ = v32
    if view.numel() >= 40:                                   # some points are seen, some by no camera, and not all by camera 0
        assert bool(valid.any()) and not bool(valid.any(2).all()) and (N == 1 or int((view > 0).sum()) > 0)
    # lidar2img is distinct per (b, t, n)
    assert len({tuple(m.reshape(-1).tolist()) for m in c['l2i'].reshape(-1, 4, 4)}) == B * T * N


def test_project_main_cases_select_every_camera_somewhere():
    views = set()
    for name, dims in C.PROJECT_MAIN.items():
        if dims[3] == 6:
            c = C.project_case(name)
            views |= set(C.project_views(c['pts'], c['l2i'], C.EPS, C.IMAGE_H, C.IMAGE_W)[1].unique().tolist())
    assert views == set(range(6))


def test_project_edge_case_hits_every_edge():
    c = C.project_case('edges')
    B, Q, T, N, G, P = c['dims']
    valid, view, over = C.project_views(c['pts'], c['l2i'], C.EPS, C.IMAGE_H, C.IMAGE_W)
    with C.oracle_setting(n_views=N):
        uvh, _ = O.project_points(c['pts'], c['l2i'], C.IMAGE_H, C.IMAGE_W, C.EPS)
        uvh64, _ = O.project_points(c['pts'].double(), c['l2i'].double(), C.IMAGE_H, C.IMAGE_W, C.EPS)
    scen = lambda t, s: t.reshape(B * T, *t.shape[2:])[s]
    hits = valid.sum(2)
    homo64 = (c['l2i'].double().reshape(B, T, N, 1, 1, 4, 4)[..., 2, :3] * c['pts'].double().permute(0, 2, 1, 3, 4)[:, :, None]).sum(-1) \
        + c['l2i'].double().reshape(B, T, N, 1, 1, 4, 4)[..., 2, 3]
    assert not bool((homo64 == C.EPS).any()) and not bool((homo64 == 1e-5).any())           # no tie for torch.maximum to split
    sel_over = torch.gather(over, 2, view[:, :, None]).squeeze(2)
    sel_hm = torch.gather(homo64, 2, view[:, :, None]).squeeze(2)
    for s in (0, 1, 2):                                      # every camera misses: view 0
        assert int(scen(hits, s).sum()) == 0 and int(scen(view, s).abs().sum()) == 0
    assert bool(scen(sel_over, 0).all())                     # hm > eps: g_hm flows
    assert not bool(scen(sel_over, 1).any()) and bool((scen(sel_hm, 1) < 0).all())
    assert not bool(scen(sel_over, 2).any()) and bool(((scen(sel_hm, 2) > 0) & (scen(sel_hm, 2) < C.EPS)).all())
    assert bool((scen(hits, 3) == 2).all()) and bool((scen(view, 3) == 1).all())           # two cameras hit: the first of them wins
    assert bool((scen(hits, 4) == 2).all()) and bool((scen(view, 4) == 0).all())
    assert bool((scen(hits, 5) == 1).all()) and bool((scen(view, 5) == N - 1).all())       # the last camera only
    assert bool((scen(view, 6) == 0).all()) and bool(((scen(sel_hm, 6) > C.EPS) & (scen(sel_hm, 6) < 2 * C.EPS)).all())
    u0, v0 = scen(uvh[..., 0], 7)[0], scen(uvh[..., 1], 7)[0]                               # camera 0 of the last scenario
    on_edge = (u0 == 0) | (u0 == 1) | (v0 == 0) | (v0 == 1)
    for val, coord in ((0.0, u0), (1.0, u0), (0.0, v0), (1.0, v0)):
        assert int((coord == val).sum()) > 0
    assert bool((scen(view, 7)[on_edge] == 1).all()) and bool((scen(view, 7)[~on_edge] == 0).all()) and int((~on_edge).sum()) > 0
    assert int((hits == 0).sum()) > 0 and int((hits == 2).sum()) > 0
    assert torch.equal(uvh[..., :2].double() == 0, uvh64[..., :2] == 0)                     # the exact zeros are exact in fp64 too


def test_front_cases_cover_the_shapes_and_no_yaw_is_degenerate():
    rows = list(C.FRONT_CASES.values())
    assert {b * q for b, q, *_ in rows} >= {1, 3, 4, 5, 257} and all(b >= 2 for b, q, *_ in rows if b * q > 1)
    assert {(g, p) for _, _, _, g, p, *_ in rows} >= {(1, 1), (4, 4), (4, 8), (7, 9), (4, 16)}
    assert {t for _, _, t, *_ in rows} >= {1, 2, 15} and {l for *_, l, _, _ in rows} >= {1, 4, 5}
    assert {r for *_, r in rows} == {1.0, -1.0} and {lay for *_, lay, _ in rows} == {'packed', 'packed+3', 'wide'}
    quadrants = set()
    for name in C.FRONT_CASES:
        s, c = C.front_inputs(name)['bbox'][..., 6].double(), C.front_inputs(name)['bbox'][..., 7].double()
        r = (s * s + c * c).sqrt()
        assert bool((r >= 0.49).all()) and bool(((r - 1).abs() > 1e-6).all())              # never zero, never a unit vector
        assert bool((s.abs() > 0.05).all()) and bool((c.abs() > 0.05).all())
        quadrants |= set(zip((s > 0).reshape(-1).tolist(), (c > 0).reshape(-1).tolist()))
    assert len(quadrants) == 4


def test_refine_cases_hold_every_edge_value():
    edges = C.refine_edges()
    assert len(set(edges.tolist())) == len(edges) == 14
    e = torch.tensor(1e-5, dtype=torch.float32)
    assert int((edges < 0).sum()) == 2 and int((edges > 1).sum()) == 2 and int((edges == e).sum()) == 1
    assert {b * q for b, q in C.REFINE_CASES.values()} == {1, 255, 256, 257}
    for name in C.REFINE_CASES:
        c = C.refine_case(name)
        got = set(c['bbox'][..., :3][c['edge']].tolist())
        assert got == (set(edges.tolist()) if name != '1' else {0.0, e.item(), 1.0})
        inner = c['bbox'][..., :3][~c['edge']]
        assert inner.numel() == 0 or (inner.min() >= 0.05 and inner.max() <= 0.95)


# ---- a correct fp32 implementation meets the device test's bounds -------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.PROJECT_CASES)
def test_project_fp32_oracle_is_inside_the_device_bound(name):
    c = C.project_case(name)
    g32 = C.project_oracle_autograd(c['pts'], c['l2i'], c['gloc'], C.EPS, C.IMAGE_H, C.IMAGE_W, torch.float32)
    excess = C.project_excess(g32, c['ref'], c['A'])
    print('project %-32s fp32 oracle: max |err| / (U A) = %.2f (bound %d)' % (name, excess, C.PROJECT_FACTOR))
    assert excess <= C.PROJECT_FACTOR


@pytest.mark.parametrize('name', list(C.REFINE_CASES))
def test_refine_fp32_oracle_is_inside_the_device_bound(name):
    c = C.refine_case(name)
    out32, greg32, gbbox32 = C.refine_oracle(c['bbox'], c['reg'], c['vel_div'], c['gout'], torch.float32)
    assert torch.equal(out32, c['out32'])
    ref_reg, ref_bbox = C.refine_bwd_ref(c['gout'], out32, c['bbox'], c['vel_div'])
    for got, ref in ((greg32[..., :3], ref_reg[..., :3]), (gbbox32[..., :3], ref_bbox[..., :3])):
        assert bool(((got.double() - ref).abs() <= C.REFINE_FACTOR * C.U * ref.abs()).all())
    assert torch.equal(greg32[..., 3:8], c['gout'][..., 3:8]) and torch.equal(greg32[..., 8:], c['gout'][..., 8:] / c['vel_div'][:, None, None])


# ---- the per-column bounds catch what the aggregate measure lets through ---------------------------------------------------------------------
def _front_breaks(wrong=None, flip=False):
    """the (case, column) pairs in which a wrong variant of the reference, taken as a kernel's output, exceeds the column's bound"""
    broken = []
    for name, (B, Q, T, G, P, L, _, rot_sign) in C.FRONT_CASES.items():
        c = C.front_case(name)
        bad = C.front_bwd_ref(c['bbox'], c['offset'], c['logits'], c['gpts'], c['gw_bp'], C.PC_RANGE, T, G, P, L, -rot_sign if flip else rot_sign, wrong)
        broken += [(name, k) for k, (e, e32, s, bound) in C.front_column_errors(bad, c['ref'], c['oracle32']).items() if e > bound]
    return broken


def _project_breaks(wrong):
    broken = []
    for name in C.PROJECT_CASES:
        c = C.project_case(name)
        bad, _ = C.project_select_bwd_ref(c['pts'], c['l2i'], c['gloc'], C.EPS, C.IMAGE_H, C.IMAGE_W, wrong)
        excess = ((bad - c['ref']).abs() / (C.U * c['A']).clamp_min(1e-300)).amax((0, 1, 2, 3))
        broken += [(name, 'gpts[%d]' % k) for k in range(3) if excess[k] > C.PROJECT_FACTOR]
    return broken


def _refine_breaks(wrong):
    broken = []
    for name in C.REFINE_CASES:
        c = C.refine_case(name)
        ref_reg, ref_bbox = C.refine_bwd_ref(c['gout'], c['out32'], c['bbox'], c['vel_div'])
        bad_reg, bad_bbox = C.refine_bwd_ref(c['gout'], c['out32'], c['bbox'], c['vel_div'], wrong)
        if bool(((bad_bbox - ref_bbox).abs() > C.REFINE_FACTOR * C.U * ref_bbox.abs()).any()):
            broken.append((name, 'gbbox[0:3]'))
        if not torch.equal(bad_reg[..., 8:].float(), ref_reg[..., 8:].float()):
            broken.append((name, 'greg[8:10]'))
    return broken


def test_each_wrong_variant_breaks_a_per_column_bound():
    found = {
        'rot_sign flipped': _front_breaks(flip=True),
        'yaw gradient from t = 0 only': _front_breaks('yaw_t0'),
        'gbbox[6] and gbbox[7] swapped': _front_breaks('swap67'),
        'level gradient from row (b T + t) G + g': _front_breaks('level_row'),
        'g_hm passed when hm <= eps': _project_breaks('g_hm_always'),
        'no hit: the last view': _project_breaks('last_view'),
        'refine clamp passes outside [0, 1]': _refine_breaks('clamp'),
        'velocity not divided by vel_div': _refine_breaks('vel'),
    }
    for what, broken in found.items():
        print('%-42s breaks %d (case, column) pairs, e.g. %s' % (what, len(broken), broken[:2]))
        assert broken, what
    assert not _front_breaks() and not _project_breaks(None) and not _refine_breaks(None)        # the right reference breaks none
    # where each shows: the yaw mistakes in the yaw columns (and, for the sign, the offsets and sizes), the level row in the logits
    assert {k for _, k in found['gbbox[6] and gbbox[7] swapped']} == {'bbox[6]', 'bbox[7]'}
    assert {k for _, k in found['yaw gradient from t = 0 only']} == {'bbox[6]', 'bbox[7]'}
    assert all(k.startswith('logit') for _, k in found['level gradient from row (b T + t) G + g'])
    # T = 1 cannot tell frame 0 from the sum, G = 1 or T = 1 cannot tell the two row orders apart
    assert all(C.FRONT_CASES[n][2] > 1 for n, _ in found['yaw gradient from t = 0 only'] + found['level gradient from row (b T + t) G + g'])


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def test_what_the_aggregate_measure_of_the_function_test_lets_through():
    """test_gpu_backward.py::test_sampling_function_vs_oracle_autograd asserts max |err| / max |ref| < 2e-4 over the whole box gradient and
    over the whole packed offsets | logits gradient.  Here the two closed-form references are chained at that test's kind of input
    (B = 2, Q = 36, T = 3, G = P = 4, the tiny pyramid's cameras, standard normal grad_loc and grad_weights) and the first five wrong
    variants are measured the same way.  Points behind a camera go through hn = eps, so a few centre gradients of 1e7 .. 5e7 set
    max |ref|; the column maxima are 1.8e7 5.1e7 1.0e7 (centre), 2.3e5 2.2e5 5.4e5 (log-dims), 4.3e4 2.7e5 (sin, cos).
    Measured aggregate error: wrong level row 1.6e-6 (packed gradient) -- far under 2e-4, invisible.  Flipped rot_sign 8.5e-3, yaw from
    t = 0 only 9.2e-3, swapped sin / cos columns 6.2e-3 (box gradient): these do NOT stay under 2e-4 at these inputs -- a mistake that
    replaces a whole yaw column is 30 to 50 times the bound --, but only because it is a 100 % error: the bound admits an absolute
    error of 1.0e4, which is 24 % of the largest sin gradient and 2 .. 5 % of the largest cos and log-dim gradients, where the
    per-column bound of the device test admits about 1e-6 of each column's own maximum.  g_hm passed at hm <= eps multiplies the
    outliers themselves (1.5e6) and is seen by any measure.  The inputs are not bent to make any of this otherwise."""
    B, Q, T, G, P, L = 2, 36, 3, 4, 4, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    g = torch.Generator().manual_seed(T * 10 + L)
    bbox, _ = S.make_queries(B, Q, seed=7)
    both = torch.randn(B, Q, G * P * (3 + L), generator=g) * 0.5
    metas = S.make_img_metas(B, T, ih, iw)
    td = O.time_diff_from_metas(metas, B)
    l2i = torch.from_numpy(np.asarray([m['lidar2img'] for m in metas]).astype(np.float32))
    n_off = G * P * 3
    offset, logits = both[..., :n_off].reshape(B, Q, G * P, 3), both[..., n_off:].reshape(B, Q, G * P, L)
    pts = O.make_sample_points(bbox, offset, S.PC_RANGE)[:, :, None].expand(B, Q, T, G * P, 3)
    shift = (bbox[..., 8:][:, :, None, :] * td[:, None, :, None])[:, :, :, None, :]
    pts = torch.cat([pts[..., 0:2] - shift, pts[..., 2:3]], -1).contiguous()
    gloc = torch.randn(B * T * G, Q, P, 3, generator=g)
    gw = torch.randn(B * G * T, Q, P, L, generator=g)

    def chain(project_wrong=None, front_wrong=None, rot_sign=1.0):
        gpts, _ = C.project_select_bwd_ref(pts, l2i, gloc, C.EPS, float(ih), float(iw), project_wrong)
        goff, glog, gbbox = C.front_bwd_ref(bbox, offset, logits, gpts, gw, S.PC_RANGE, T, G, P, L, rot_sign, front_wrong)
        return gbbox, torch.cat([goff.reshape(B, Q, -1), glog.reshape(B, Q, -1)], -1)

    ref_bbox, ref_both = chain()
    print('column maxima of grad_bbox: %s' % ' '.join('%.1e' % v for v in ref_bbox.abs().amax((0, 1))[:8]))
    measured = {}
    for what, kw in (('rot_sign', dict(rot_sign=-1.0)), ('yaw_t0', dict(front_wrong='yaw_t0')), ('swap67', dict(front_wrong='swap67')),
                     ('level_row', dict(front_wrong='level_row')), ('g_hm_always', dict(project_wrong='g_hm_always'))):
        bad_bbox, bad_both = chain(**kw)
        measured[what] = (_rel(bad_bbox, ref_bbox), _rel(bad_both, ref_both))
        print('aggregate rel of %-12s grad_bbox %.1e  grad_offsets|logits %.1e' % ((what,) + measured[what]))
    assert measured['level_row'][0] == 0 and 0 < measured['level_row'][1] < 2e-4 / 100
    for what in ('rot_sign', 'yaw_t0', 'swap67'):
        assert 2e-4 < measured[what][0] < 1e-2, what
    assert measured['g_hm_always'][0] > 1
    # the absolute error the aggregate bound admits, against each column's own maximum
    admitted = 2e-4 * ref_bbox.abs().max() / ref_bbox.abs().amax((0, 1))[:8]
    print('2e-4 max |grad_bbox| as a share of each column\'s maximum: %s' % ' '.join('%.1e' % v for v in admitted))
    assert bool((admitted[3:8] > 1e4 * C.FRONT_FACTOR_U * C.U).all())
