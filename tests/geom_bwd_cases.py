"""Inputs and fp64 references of the sampling geometry's backward kernels (csrc/backward_ops.hip): sbev_project_select_bwd,
sbev_sampling_front_bwd and sbev_refine_bbox_bwd -- tests/test_gpu_geom_bwd.py on the device, tests/test_geom_bwd_host.py for what can be
checked without one.

Every reference is a closed-form fp64 restatement of the kernel's CONTRACT, written from the oracle's forward ops (make_sample_points,
decode_bbox, project_points, select_view, inverse_sigmoid, quirk q1 of sampling_4d) and differentiated by hand; the host test holds each
one against torch's fp64 autograd of those ops.  DECISIONS are taken in fp32, as the kernels take them -- which camera a point is
sampled from, whether the homogeneous coordinate exceeds eps, the three comparisons of the inverse-sigmoid clamp -- and the derivative
is then taken in fp64 with the decision fixed.

The gradients are compared PER COLUMN: a box gradient's centre columns carry the point-cloud span (about 100) and, behind a real
projection, 1 / eps outliers, so one norm over all ten columns cannot see the yaw or size columns at all.

`wrong=` on a reference builds a deliberately wrong variant of it; the host test uses them to show that the per-column bounds of the
device test would catch each of those mistakes.  Everything here is torch on the CPU."""
import contextlib
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import sparsebev_oracle as O

U = 2.0 ** -24                                              # half an ulp of 1.0f: the relative error of one fp32 rounding
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the eps the entry points receive as a float: float32(1e-5), not 1e-5
PC_RANGE = [-40.0, -61.2, -4.0, 62.4, 31.2, 4.0]            # three different spans
IMAGE_H, IMAGE_W = 32.0, 64.0                               # powers of two: u = 0 and u = 1 can be hit exactly
PROJECT_FACTOR = 16                                         # |got - ref| <= 16 U A, see project_select_bwd_ref
FRONT_FACTOR_E32, FRONT_FACTOR_U = 4, 16                    # e <= max(4 e32, 16 U s) per column
REFINE_FACTOR = 8                                           # |got - ref| <= 8 U |ref| on the sigmoid / clamp columns


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))     # the same stream in every process


@contextlib.contextmanager
def oracle_setting(n_views=None, version=None):
    """the oracle's two module globals: the camera count its projection reshapes by, and the box convention (rotation sign)"""
    old = O.N_VIEWS, O.VERSION_NAME
    try:
        if n_views is not None:
            O.N_VIEWS = n_views
        if version is not None:
            O.VERSION_NAME = version
        yield
    finally:
        O.N_VIEWS, O.VERSION_NAME = old


def version_of(rot_sign):
    return 'v0.17.1' if rot_sign < 0 else 'v1.0.0'


# ======================================================================================================================================
# sbev_project_select_bwd
# ======================================================================================================================================
def project_views(pts, l2i, eps, H, W, dtype=torch.float32):
    """the oracle's decisions in `dtype`: valid [B,T,N,Q,GP] (bool), the selected view [B,T,Q,GP] (first hit, 0 when none hits) and
    over [B,T,N,Q,GP] = (homo > eps) per camera.  In float32 this is the documented bit-exact contract with the kernels."""
    T = pts.shape[2]
    N = l2i.shape[1] // T
    with torch.no_grad(), oracle_setting(n_views=N):
        uvh, valid = O.project_points(pts.to(dtype), l2i.to(dtype), H, W, eps)
        view, _ = O.select_view(uvh, valid)
    return valid > 0, view, uvh[..., 2] > eps                # max(homo, eps) > eps  <=>  homo > eps


def _gloc_per_point(gloc, B, T, G, Q, P):
    """[B*T*G, Q, P, 3] -> [B, T, Q, G*P, 3]: the (b, t, g) flattening of sampling_4d undone"""
    return gloc.reshape(B, T, G, Q, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, T, Q, G * P, 3)


def project_select_bwd_ref(pts, l2i, gloc, eps, H, W, wrong=None):
    """pts [B,Q,T,GP,3], l2i [B,T*N,4,4], gloc [B*T*G,Q,P,3] (x, y used) -> (gpts, A), both [B,Q,T,GP,3] in fp64.

    With M the selected camera's matrix, (uh, vh, hm) = M[0:3] . (x, y, z, 1) and hn = max(hm, eps):
        u = uh / hn / W,  v = vh / hn / H
        g_uh = gu / (hn W),  g_vh = gv / (hn H),  g_hm = -(g_uh uh + g_vh vh) / hn  if hm > eps  else 0  (torch.maximum's gradient)
        gpts[k] = g_uh M[0,k] + g_vh M[1,k] + g_hm M[2,k]
    A[k] = |g_uh M[0,k]| + |g_vh M[1,k]| + (|g_uh uh| + |g_vh vh|) / hn |M[2,k]|: the sum of the absolute values of the three terms,
    |g_hm| bounded by its two parts.  An fp32 evaluation rounds each factor about six times (a four-term dot product, a max, two
    divides, a multiply) when the dot products do not cancel, so its error stays below PROJECT_FACTOR U A = about twice that count.
    wrong: 'last_view' (a point no camera hits goes through the LAST camera), 'g_hm_always' (g_hm also where hm <= eps)."""
    B, Q, T, GP, _ = pts.shape
    N = l2i.shape[1] // T
    P = gloc.shape[2]
    G = GP // P
    valid, view, over = project_views(pts, l2i, eps, H, W)
    if wrong == 'last_view':
        view = torch.where(valid.any(2), view, torch.full_like(view, N - 1))
    active = torch.gather(over, 2, view[:, :, None]).squeeze(2)                      # hm > eps of the selected camera, in fp32
    M = l2i.double().reshape(B, T, N, 4, 4)
    bi, ti = torch.arange(B)[:, None, None, None], torch.arange(T)[None, :, None, None]
    Ms = M[bi, ti, view]                                                             # [B,T,Q,GP,4,4]
    x = pts.double().permute(0, 2, 1, 3, 4)                                          # [B,T,Q,GP,3]
    xh = torch.cat([x, torch.ones_like(x[..., :1])], -1)
    uh, vh, hm = ((Ms[..., r, :] * xh).sum(-1) for r in range(3))
    hn = torch.where(active, hm, torch.full_like(hm, eps))
    g = _gloc_per_point(gloc.double(), B, T, G, Q, P)
    g_uh, g_vh = g[..., 0] / (hn * W), g[..., 1] / (hn * H)
    passes = torch.ones_like(active) if wrong == 'g_hm_always' else active
    zero = torch.zeros_like(hm)
    g_hm = torch.where(passes, -(g_uh * uh + g_vh * vh) / hn, zero)
    a_hm = torch.where(passes, ((g_uh * uh).abs() + (g_vh * vh).abs()) / hn, zero)
    gpts = g_uh[..., None] * Ms[..., 0, :3] + g_vh[..., None] * Ms[..., 1, :3] + g_hm[..., None] * Ms[..., 2, :3]
    A = (g_uh[..., None] * Ms[..., 0, :3]).abs() + (g_vh[..., None] * Ms[..., 1, :3]).abs() + a_hm[..., None] * Ms[..., 2, :3].abs()
    return gpts.permute(0, 2, 1, 3, 4).contiguous(), A.permute(0, 2, 1, 3, 4).contiguous()


def project_oracle_autograd(pts, l2i, gloc, eps, H, W, dtype):
    """torch autograd of the oracle's project_points -> select_view -> the (b, t, g) flattening of sampling_4d in `dtype`, the view FIXED
    to the float32 decision (select_view is given that view's one-hot mask in place of the hit mask)"""
    B, Q, T, GP, _ = pts.shape
    N = l2i.shape[1] // T
    P = gloc.shape[2]
    G = GP // P
    _, view, _ = project_views(pts, l2i, eps, H, W)
    onehot = F.one_hot(view, N).permute(0, 1, 4, 2, 3).to(dtype)                     # [B,T,N,Q,GP]
    p = pts.detach().clone().to(dtype).requires_grad_(True)
    with torch.enable_grad(), oracle_setting(n_views=N):
        uvh, _ = O.project_points(p, l2i.to(dtype), H, W, eps)
        _, loc = O.select_view(uvh, onehot)
        loc_bp = loc.reshape(B, T, Q, G, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(B * T * G, Q, P, 3)
        (loc_bp[..., :2] * gloc[..., :2].to(dtype)).sum().backward()
    return p.grad


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
PROJECT_MAIN = {                     # name: (B, Q, T, N, G, P)
    'one-point': (1, 1, 1, 6, 1, 1),
    'odd-210-points': (2, 5, 3, 6, 1, 7),        # no multiple of the 256-thread block, every index divisor distinct
    'one-camera': (2, 3, 2, 1, 2, 2),
    'two-cameras-T15': (1, 9, 15, 2, 4, 8),
    'across-a-block': (2, 33, 2, 6, 4, 16),      # 8448 points, 64 per (b, t, q)
}


def _project_main(name):
    """positive points and matrices: no dot product cancels, hm >= 1 everywhere, so no gradient column has outliers.  The cameras'
    scales differ so that a point is seen by some of them only: every view index wins somewhere, and some points are seen by none."""
    B, Q, T, N, G, P = PROJECT_MAIN[name]
    g = _gen('project', name)
    rand = lambda *s: torch.rand(*s, generator=g)
    pts = 0.5 + 1.5 * rand(B, Q, T, G * P, 3)
    l2i = torch.zeros(B, T * N, 4, 4)
    l2i[:, :, 0] = (0.1 + 0.9 * rand(B, T * N, 4)) * (IMAGE_W * (0.6 + 1.2 * rand(B, T * N, 1)))
    l2i[:, :, 1] = (0.1 + 0.9 * rand(B, T * N, 4)) * (IMAGE_H * (0.6 + 1.2 * rand(B, T * N, 1)))
    l2i[:, :, 2, :3] = 0.1 + 0.4 * rand(B, T * N, 3)
    l2i[:, :, 2, 3] = 1.0 + rand(B, T * N)
    l2i[:, :, 3, 3] = 1.0
    gloc = torch.randn(B * T * G, Q, P, 3, generator=g)
    return dict(pts=pts, l2i=l2i, gloc=gloc, dims=(B, Q, T, N, G, P))


def _cam(row0, row1, row2):
    return torch.tensor([list(row0), list(row1), list(row2), [0.0, 0.0, 0.0, 1.0]])


# Edge scenarios: one per (b, t) of the 'edges' case, three cameras each.  The 18 points are (x, y, z) with x, y in {1, 1.5, 2} and z in
# {1.5, 2.5}; the matrices hold small integers or powers of two, so every uh, vh, hm is exact in fp32 and no decision is left to rounding.
_HIT_A = _cam((16, 0, 4, 0), (0, 8, 2, 0), (0, 0, 0, 1))            # hm = 1: u in (0.34, 0.66), v in (0.34, 0.66)
_HIT_B = _cam((16, 0, 8, 0), (0, 8, 4, 0), (0, 0, 1, 0))            # hm = z: u, v in (0, 0.5)
_HIT_C = _cam((32, 0, -4, 0), (0, -8, 2, 24), (0, 0, 0, 1))         # hm = 1, negative entries: u in (0.34, 0.91), v in (0.34, 0.66)
_MISS_A = _cam((64, 0, 0, 64), (0, 8, 2, 0), (0, 0, 0, 1))          # u >= 2
_MISS_B = _cam((-16, 0, 0, 0), (0, 8, 2, 0), (0, 0, 0, 1))          # u < 0
_MISS_C = _cam((16, 0, 4, 0), (0, 64, 0, 0), (0, 0, 0, 1))          # v >= 2
EDGE_SCENARIOS = [
    ('every camera misses, hm > eps', [_MISS_A, _MISS_B, _MISS_C]),
    ('every camera misses, hm < 0 in view 0', [_cam((16, 0, 4, 0), (0, 8, 2, 0), (0, 0, -1, 0)), _MISS_B, _MISS_C]),
    ('every camera misses, 0 < hm < eps in view 0', [_cam((16, 0, 4, 0), (0, 8, 2, 0), (0, 0, 2.0 ** -20, 0)), _MISS_A, _MISS_C]),
    ('cameras 1 and 2 hit', [_MISS_A, _HIT_A, _HIT_B]),
    ('cameras 0 and 1 hit', [_HIT_C, _HIT_A, _MISS_A]),
    ('the last camera only', [_MISS_A, _MISS_B, _HIT_B]),
    ('hm in (eps, 2 eps)', [_cam((2.0 ** -13, 0, 0, 0), (0, 2.0 ** -14, 0, 0), (0, 0, 2.0 ** -17, 0)), _HIT_A, _MISS_A]),
    ('u or v exactly 0 or 1 in camera 0', [_cam((64, 0, 0, -64), (0, 32, 0, -32), (0, 0, 0, 1)), _HIT_A, _HIT_B]),
]
EDGE_DIMS = (2, 3, 4, 3, 2, 3)       # B, Q, T, N, G, P: B * T = 8 scenarios, Q * G * P = 18 points each


def _project_edges():
    B, Q, T, N, G, P = EDGE_DIMS
    g = _gen('project', 'edges')
    i = torch.arange(Q * G * P)
    grid = torch.stack([torch.tensor([1.0, 1.5, 2.0])[i % 3], torch.tensor([1.0, 1.5, 2.0])[(i // 3) % 3], torch.tensor([1.5, 2.5])[i // 9]], -1)
    pts = grid.reshape(1, Q, 1, G * P, 3).expand(B, Q, T, G * P, 3).contiguous()
    l2i = torch.stack([torch.stack(cams) for _, cams in EDGE_SCENARIOS]).reshape(B, T * N, 4, 4)       # scenario s = b * T + t
    gloc = torch.randn(B * T * G, Q, P, 3, generator=g)
    return dict(pts=pts, l2i=l2i, gloc=gloc, dims=EDGE_DIMS)


PROJECT_CASES = list(PROJECT_MAIN) + ['edges']


@functools.lru_cache(maxsize=None)
def project_case(name):
    """dict(pts, l2i, gloc, dims, ref, A) -- read-only"""
    c = _project_edges() if name == 'edges' else _project_main(name)
    c['ref'], c['A'] = project_select_bwd_ref(c['pts'], c['l2i'], c['gloc'], EPS, IMAGE_H, IMAGE_W)
    return c


def project_excess(got, ref, A):
    """max over the elements of |got - ref| / (U A): the bound is PROJECT_FACTOR.  An element with A = 0 must be exact."""
    err = (got.double() - ref).abs()
    assert bool((err[A == 0] == 0).all())
    return (err / (U * A).clamp_min(1e-300)).max().item()


# ======================================================================================================================================
# sbev_sampling_front_bwd
# ======================================================================================================================================
def front_bwd_ref(bbox, offset, logits, gpts, gw_bp, pc_range, T, G, P, L, rot_sign, wrong=None):
    """bbox [B,Q,10], offset [B,Q,GP,3], logits [B,Q,GP,L], gpts [B,Q,T,GP,3] or None, gw_bp [B*G*T,Q,P,L] or None
    -> goffset [B,Q,GP,3], glogits [B,Q,GP,L], gbbox [B,Q,10] in fp64.

    make_sample_points: with (cx, cy, cz) = bbox[0:3] span + lo, e = exp(bbox[3:6]), yaw = atan2(bbox[6], bbox[7]), c = cos yaw,
    s = rot_sign sin yaw and d = e offset:  px = cx + d0 c - d1 s,  py = cy + d0 s + d1 c,  pz = cz + d2, the same point in every
    frame (the velocity warp is detached).  With g = sum_t gpts:
        g_d = (gx c + gy s, -gx s + gy c, gz);   goffset = g_d e;   gbbox[3:6] = sum_gp g_d d;   gbbox[0:3] = span sum_gp g
        g_yaw = sum_gp (gx d0 + gy d1)(-sin yaw) + (-gx d1 + gy d0) rot_sign cos yaw
        gbbox[6] = g_yaw bbox[7] / r2,  gbbox[7] = -g_yaw bbox[6] / r2,  r2 = bbox[6]^2 + bbox[7]^2;   gbbox[8:10] = 0
    Level softmax w = softmax(logits): sampling_4d reads weight row (b G + g) T + t (quirk q1), every t holding the same softmax:
        gs = sum_t gw_bp[(b G + g) T + t, q, p];   glogits = w (gs - sum_l w gs)
    wrong: 'yaw_t0' (g_yaw from frame 0 alone), 'swap67' (gbbox[6] and [7] exchanged), 'level_row' (weight row (b T + t) G + g)."""
    B, Q = bbox.shape[:2]
    GP = G * P
    bb, off, lg = bbox.double(), offset.double().reshape(B, Q, GP, 3), logits.double().reshape(B, Q, GP, L)
    goffset, gbbox = torch.zeros(B, Q, GP, 3, dtype=torch.float64), torch.zeros(B, Q, 10, dtype=torch.float64)
    if gpts is not None:
        span = torch.tensor([pc_range[3] - pc_range[0], pc_range[4] - pc_range[1], pc_range[5] - pc_range[2]], dtype=torch.float64)
        e = bb[..., None, 3:6].exp()
        r2 = bb[..., 6] ** 2 + bb[..., 7] ** 2
        cos_yaw, sin_yaw = (bb[..., 7] / r2.sqrt())[..., None], (bb[..., 6] / r2.sqrt())[..., None]
        c, s = cos_yaw, rot_sign * sin_yaw
        d = e * off

        def yaw_grad(g):
            g_c, g_s = g[..., 0] * d[..., 0] + g[..., 1] * d[..., 1], -g[..., 0] * d[..., 1] + g[..., 1] * d[..., 0]
            return (g_c * -sin_yaw + g_s * rot_sign * cos_yaw).sum(-1)

        g = gpts.double().sum(2)                                                      # [B,Q,GP,3]
        g_d = torch.stack([g[..., 0] * c + g[..., 1] * s, -g[..., 0] * s + g[..., 1] * c, g[..., 2]], -1)
        goffset = g_d * e
        gbbox[..., 0:3] = g.sum(2) * span
        gbbox[..., 3:6] = (g_d * d).sum(2)
        g_yaw = yaw_grad(gpts.double()[:, :, 0] if wrong == 'yaw_t0' else g)
        gbbox[..., 6], gbbox[..., 7] = g_yaw * bb[..., 7] / r2, -g_yaw * bb[..., 6] / r2
        if wrong == 'swap67':
            gbbox[..., 6], gbbox[..., 7] = gbbox[..., 7].clone(), gbbox[..., 6].clone()
    glogits = torch.zeros(B, Q, GP, L, dtype=torch.float64)
    if gw_bp is not None:
        gw = gw_bp.double()
        gs = gw.reshape(B, T, G, Q, P, L).sum(1) if wrong == 'level_row' else gw.reshape(B, G, T, Q, P, L).sum(2)      # [B,G,Q,P,L]
        gs = gs.permute(0, 2, 1, 3, 4).reshape(B, Q, GP, L)
        w = torch.softmax(lg, -1)
        glogits = w * (gs - (w * gs).sum(-1, keepdim=True))
    return goffset, glogits, gbbox


def front_oracle_autograd(bbox, offset, logits, gpts, gw_bp, pc_range, T, G, P, L, rot_sign, dtype):
    """torch autograd in `dtype` of make_sample_points expanded over the T frames and of the level softmax in the (b, g, t) row order
    in which sampling_4d reads the weights -> (goffset, glogits, gbbox) shaped like front_bwd_ref's"""
    B, Q = bbox.shape[:2]
    GP = G * P
    b = bbox.detach().clone().to(dtype).requires_grad_(True)
    o = offset.detach().clone().to(dtype).reshape(B, Q, GP, 3).requires_grad_(True)
    l = logits.detach().clone().to(dtype).reshape(B, Q, GP, L).requires_grad_(True)
    with torch.enable_grad(), oracle_setting(version=version_of(rot_sign)):
        loss = b.sum() * 0 + o.sum() * 0 + l.sum() * 0
        if gpts is not None:
            pts = O.make_sample_points(b, o, pc_range)[:, :, None].expand(B, Q, T, GP, 3)
            loss = loss + (pts * gpts.to(dtype)).sum()
        if gw_bp is not None:
            sw = torch.softmax(l.reshape(B, Q, G, 1, P, L), -1).expand(B, Q, G, T, P, L)
            w_bp = sw.permute(0, 2, 3, 1, 4, 5).reshape(B * G * T, Q, P, L)
            loss = loss + (w_bp * gw_bp.to(dtype)).sum()
        loss.backward()
    return o.grad, l.grad, b.grad


def front_columns(goffset, glogits, gbbox):
    """the columns the device test bounds one by one: the 8 box columns, the three offset components, the logits per level index"""
    cols = {'bbox[%d]' % d: gbbox[..., d].reshape(-1) for d in range(8)}
    cols.update({'offset[%d]' % d: goffset[..., d].reshape(-1) for d in range(3)})
    cols.update({'logit[%d]' % l: glogits[..., l].reshape(-1) for l in range(glogits.shape[-1])})
    return cols


def front_column_errors(got, ref, oracle32):
    """per column (e, e32, s, bound): e = max |got - ref|, e32 = max |fp32 oracle - ref|, s = max |ref|,
    bound = max(FRONT_FACTOR_E32 e32, FRONT_FACTOR_U U s).  The factor 4 on the fp32 oracle's own error covers the other summation order
    (a wave tree and a loop over T against torch's sums) and the maximum being taken over a few thousand elements."""
    out = {}
    rc, oc = front_columns(*ref), front_columns(*oracle32)
    for k, g in front_columns(*got).items():
        e = (g.double() - rc[k]).abs().max().item()
        e32 = (oc[k].double() - rc[k]).abs().max().item()
        s = rc[k].abs().max().item()
        out[k] = (e, e32, s, max(FRONT_FACTOR_E32 * e32, FRONT_FACTOR_U * U * s))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
# name: (B, Q, T, G, P, L, layout, rot_sign).  layout: 'packed' = one [B*Q, G*P*(3+L)] row of offsets | logits, and the same for the
# gradient, as autograd.Sampling passes them; 'packed+3' = the same with three guard columns behind every row; 'wide' = three unrelated
# buffers whose rows are wider than their payload.
FRONT_CASES = {
    'bq1-gp1-L1': (1, 1, 1, 1, 1, 1, 'packed', 1.0),              # one query, one point, one level: a wave with one live lane
    'bq3-gp16': (3, 1, 2, 4, 4, 4, 'packed', 1.0),                # B * Q below the 4 waves of a block
    'bq4-gp32-T15-L5': (2, 2, 15, 4, 8, 5, 'packed', -1.0),       # one full block
    'bq5-gp63': (5, 1, 2, 7, 9, 4, 'wide', 1.0),                  # one lane of the wave idle, a second block with one query
    'bq257-gp64-L1': (257, 1, 1, 4, 16, 1, 'packed+3', 1.0),      # a full wave, 65 blocks
    'bq18-B2': (2, 9, 2, 4, 4, 4, 'wide', -1.0),                  # Q > 1 under B > 1: the (b, q) split of the weight rows
    'bq5-gp64-T15': (5, 1, 15, 4, 16, 5, 'packed+3', -1.0),
}
FRONT_NULLS = (None, 'gpts', 'gw_bp', 'gbbox')


def front_layout(layout, GP, L):
    """(ld_off, ld_logit, ld_grad, packed)"""
    if layout == 'wide':
        return GP * 3 + 5, GP * L + 2, max(GP * 3, GP * L) + 7, False
    ld = GP * (3 + L) + (3 if layout == 'packed+3' else 0)
    return ld, ld, ld, True


@functools.lru_cache(maxsize=None)
def front_inputs(name):
    """dict(bbox, offset, logits, gpts, gw_bp, dims) -- read-only.  The yaw runs through all four quadrants at angles away from the axes,
    with |(sin, cos)| in [0.5, 2): never a unit vector, never zero.  gpts and gw_bp are standard normal."""
    B, Q, T, G, P, L, _, _ = FRONT_CASES[name]
    g = _gen('front', name)
    GP = G * P
    bbox = torch.randn(B, Q, 10, generator=g)
    bbox[..., 0:3] = torch.rand(B, Q, 3, generator=g)
    bbox[..., 3:6] *= 0.5
    i = torch.arange(B * Q).reshape(B, Q)
    theta = (i % 4).double() * (torch.pi / 2) + 0.2 + 1.1 * torch.rand(B, Q, generator=g).double()
    r = 0.5 + 1.5 * torch.rand(B, Q, generator=g).double()
    bbox[..., 6], bbox[..., 7] = (r * theta.sin()).float(), (r * theta.cos()).float()
    return dict(bbox=bbox, offset=torch.randn(B, Q, GP, 3, generator=g) * 0.5, logits=torch.randn(B, Q, GP, L, generator=g),
                gpts=torch.randn(B, Q, T, GP, 3, generator=g), gw_bp=torch.randn(B * G * T, Q, P, L, generator=g))


@functools.lru_cache(maxsize=None)
def front_case(name, null=None):
    """the inputs with `null` (one of FRONT_NULLS) left out, the fp64 reference and the float32 oracle's autograd -- read-only"""
    B, Q, T, G, P, L, _, rot_sign = FRONT_CASES[name]
    c = dict(front_inputs(name))
    if null in ('gpts', 'gw_bp'):
        c[null] = None
    args = (c['bbox'], c['offset'], c['logits'], c['gpts'], c['gw_bp'], PC_RANGE, T, G, P, L, rot_sign)
    c['ref'] = front_bwd_ref(*args)
    c['oracle32'] = front_oracle_autograd(*args, torch.float32)
    return c


# ======================================================================================================================================
# sbev_refine_bbox_bwd
# ======================================================================================================================================
def refine_bwd_ref(gout, out, bbox, vel_div, wrong=None):
    """gout, out (the forward's output: out[0:3] = the sigmoid), bbox (the proposal) [B,Q,10], vel_div [B] or None -> (greg, gbbox), fp64.

    out[0:3] = sigmoid(reg[0:3] + inverse_sigmoid(p)),  inverse_sigmoid(p) = log(max(x, eps) / max(1 - x, eps)),  x = clamp(p, 0, 1):
        greg[0:3] = gout s (1 - s);   greg[3:8] = gout;   greg[8:10] = gout / vel_div[b]
        gbbox[0:3] = greg[0:3] ([p >= eps] / p + [1 - p >= eps] / (1 - p)) [0 <= p <= 1];   gbbox[3:10] = 0
    (torch's clamp passes the gradient where the input lies inside the closed range).  The three comparisons are made on the float32
    values -- eps = float32(1e-5), 1 - p the float32 difference --, the quotients in fp64.
    wrong: 'clamp' (the gradient also passes outside [0, 1]), 'vel' (no division by vel_div)."""
    go, s = gout.double(), out.double()[..., :3]
    greg = go.clone()
    greg[..., :3] = go[..., :3] * s * (1 - s)
    if vel_div is not None and wrong != 'vel':
        greg[..., 8:] = go[..., 8:] / vel_div.double()[:, None, None]
    p32 = bbox.float()[..., :3]
    eps32 = torch.tensor(1e-5, dtype=torch.float32)
    inside, lo, hi = (p32 >= 0) & (p32 <= 1), p32 >= eps32, (1 - p32) >= eps32
    if wrong == 'clamp':
        inside = torch.ones_like(inside)
    p = p32.double()
    zero = torch.zeros_like(p)
    slope = torch.where(inside & lo, 1 / p, zero) + torch.where(inside & hi, 1 / (1 - p), zero)
    gbbox = torch.zeros_like(go)
    gbbox[..., :3] = greg[..., :3] * slope
    return greg, gbbox


def refine_oracle(bbox, reg, vel_div, gout, dtype):
    """the oracle's refine step (decoder_layer: sigmoid(reg + inverse_sigmoid(proposal)), velocity / vel_div) in `dtype` and its torch
    autograd -> (out, greg, gbbox).  eps is float32(1e-5) in every dtype: the value a float32 comparison sees."""
    b = bbox.detach().clone().to(dtype).requires_grad_(True)
    r = reg.detach().clone().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        xyz = torch.sigmoid(r[..., :3] + O.inverse_sigmoid(b[..., :3], eps=EPS))
        vel = r[..., 8:] / vel_div.to(dtype)[:, None, None] if vel_div is not None else r[..., 8:]
        out = torch.cat([xyz, r[..., 3:8], vel], -1)
        (out * gout.to(dtype)).sum().backward()
    return out.detach(), r.grad, b.grad


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def refine_edges():
    """proposal coordinates at every comparison of the clamp: 0 and 1, their float32 neighbours on both sides (the ones next to 0 are
    denormals), float32(1e-5) and its neighbours, the three values around 1 - 1e-5, a negative value and one above 1"""
    e, one, zero = _f32(1e-5), _f32(1.0), _f32(0.0)
    m = one - e
    na = torch.nextafter
    return torch.stack([zero, one, na(zero, -one), na(zero, one), na(one, zero), na(one, _f32(2.0)), e, na(e, zero), na(e, one),
                        m, na(m, zero), na(m, one), _f32(-0.25), _f32(1.5)])


REFINE_CASES = {'1': (1, 1), '255': (3, 85), '256': (2, 128), '257': (257, 1)}         # name: (B, Q)


@functools.lru_cache(maxsize=None)
def refine_case(name):
    """dict(bbox, reg, gout, vel_div, out32 (the float32 oracle's forward), edge (mask of the edge coordinates)) -- read-only.
    The edge values stand at every fifth coordinate from the start; the one-query case takes 0, float32(1e-5) and 1."""
    B, Q = REFINE_CASES[name]
    g = _gen('refine', name)
    bbox = torch.rand(B, Q, 10, generator=g)
    bbox[..., :3] = 0.05 + 0.9 * bbox[..., :3]
    edges = refine_edges()
    xyz = bbox[..., :3].reshape(-1).clone()
    edge = torch.zeros_like(xyz, dtype=torch.bool)
    if xyz.numel() < 5 * len(edges):
        xyz[:3], edge[:3] = edges[[0, 6, 1]], True
    else:
        xyz[0:5 * len(edges):5], edge[0:5 * len(edges):5] = edges, True
    bbox[..., :3] = xyz.reshape(B, Q, 3)
    reg, gout = torch.randn(B, Q, 10, generator=g), torch.randn(B, Q, 10, generator=g)
    vel_div = 0.25 + torch.rand(B, generator=g)
    out32, _, _ = refine_oracle(bbox, reg, vel_div, gout, torch.float32)
    return dict(bbox=bbox, reg=reg, gout=gout, vel_div=vel_div, out32=out32, edge=edge.reshape(B, Q, 3))
