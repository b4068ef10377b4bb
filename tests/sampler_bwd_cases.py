"""Cases, fp64 reference and bound of the sampler's backward matrix (sbev_msmv_bwd / sbev_msmv_bwd_ex, csrc/msmv_sampling_bwd.hip):
tests/test_gpu_sampler_bwd.py on the device, tests/test_sampler_bwd_host.py for what can be checked without one.

Reference: ``restate`` -- the backward written out once, dtype-generic, evaluated in fp64.  Every DECISION (is the level read, the two
floors, which corner lies inside the map, the view) is taken from the fp32 products y (H-1), x (W-1), z (N-1), as sampling_cases.py does
for the forward, so the fp64 evaluation picks the kernel's taps.  A level that is not read (-1 < h_im < H and -1 < w_im < W is false:
outside, or a NaN / Inf coordinate) contributes exact zeros, which is the reference operator's rule.

Four admissible definitions: a bilinear fraction is either "fp32-rounded product minus its floor" (what the sampler's other kernels
compute) or "exact product minus the floor of the rounded product" (one fma; what msmv_sampling_bwd.hip computes, see corner_frac
there), independently for h and w.  ``references`` evaluates all four (loc.double() * (H-1) is exact in fp64); floors and decisions
are those of the fp32 product in all.

Bound (derived, not measured): with every element the restatement returns A = the sum of the absolute values of the terms that make it
up and n = their number (4 C for grad_weights, 4 C L for a grad_loc component, the live taps of the pixel for a feature gradient).  An
element passes if for at least one definition v  |got - ref_v| <= (n + 8) U A_v, U = 2^-24: (n - 1) U A is the worst case of an fp32 sum
of n terms in ANY order (float atomics, wave trees), 9 U A covers the few roundings that form a term.  Where every A_v is 0 the element
is exactly 0.  The feature gradient is ACCUMULATED into a buffer that already holds values: the value found there is one more term of
the sum, so there n grows by one and A by its absolute value; an element no live tap reaches keeps its bits."""
import functools

import torch

from sampling_cases import SIZES, edge_locs, to_mix

U = 2.0 ** -24
SLACK = 8
DEFINITIONS = [(False, False), (False, True), (True, False), (True, True)]        # (h fraction from the exact product, w fraction ...)
ALT_TAIL = [(3, 1), (1, 1)]            # the second pyramid ends in a one-column and a 1 x 1 map (W - 1 = 0, H - 1 = 0)
C_GENERIC = [1, 4, 24, 65, 68, 128]    # one lane; one quad; cok[] tail of a first trip; second trip with one live lane / one live quad; two full trips
P_LIST = [1, 3, 4, 5, 8, 32]
N_LIST = [1, 2, 6, 7]
B, T, G, Q = 1, 2, 3, 11               # B' = B T G = 6; B' Q = 66 is no multiple of the 4 waves of a block
PREFILL = 0.25                         # scale of what the feature-gradient buffers hold before the call


# ---- the cells -------------------------------------------------------------------------------------------------------------------------
def pyramid_sizes(L, alt):
    if not alt:
        return SIZES[:L]
    tail = ALT_TAIL[-min(L, 2):]
    return SIZES[:L - len(tail)] + tail


def make_cell(name, L, C, P, N, layout, pyr, alt=False, sizes=None, B=B, T=T, G=G, Q=Q, pad=0, stride_px=None):
    sizes = list(sizes) if sizes is not None else pyramid_sizes(L, alt)
    row = (G * C if pyr == 'grouped' else C) + pad
    return dict(name=name, L=L, C=C, P=P, N=N, layout=layout, pyr=pyr, sizes=sizes, B=B, T=T, G=G, Bp=B * T * G, Q=Q, pad=pad,
                stride_px=row if stride_px is None else stride_px)


def matrix_cells():
    """{C = 64 kernel, generic} x L x grad_out layout x pyramid layout in full; the generic kernel gets two more cells per L so that its
    six channel counts all meet every L; (C, P, N) rotate through their lists so that every L meets every value; the two pyramids alternate."""
    cells = []
    for L in range(1, 6):
        combos = [(lay, pyr) for lay in ('ref', 'mix') for pyr in ('bp', 'grouped')]
        per_l = [(64, c) for c in combos] + [(None, c) for c in combos + [combos[(L + 1) % 4], combos[(L + 2) % 4]]]
        for k, (C, (lay, pyr)) in enumerate(per_l):
            if C is None:
                C = C_GENERIC[(k - 4 + L) % 6]
            P, N = P_LIST[(k + 2 * L) % 6], N_LIST[(k + L) % 4]
            cells.append(make_cell('L%d-C%d-P%d-N%d-%s-%s-%s' % (L, C, P, N, lay, pyr, 'alt' if (k + L) % 2 else 'std'), L, C, P, N, lay, pyr,
                               alt=bool((k + L) % 2)))
    return cells


def extra_cells():
    one = dict(B=1, T=1, G=1)
    return [
        make_cell('one-item-C64', 4, 64, 32, 6, 'ref', 'bp', Q=1, **one),                    # B' Q = 1: three idle waves in the only block
        make_cell('one-item-C24', 4, 24, 32, 6, 'ref', 'bp', Q=1, **one),
        # launch_bwd: C = 64 but stride_px >= 2^20 -> the generic kernel; its twin holds the same data at stride_px = 64 (C = 64 kernel)
        make_cell('fallback-px2^20', 1, 64, 4, 1, 'ref', 'bp', sizes=[(1, 2)], stride_px=1 << 20, **one),
        make_cell('fallback-twin-px64', 1, 64, 4, 1, 'ref', 'bp', sizes=[(1, 2)], **one),
        # a pixel stride wider than the row: the padding (NaN in the gradient buffers) must not be written
        make_cell('padded-C64', 4, 64, 4, 6, 'mix', 'grouped', pad=4),
        make_cell('padded-C24', 3, 24, 5, 2, 'ref', 'grouped', pad=4),
        make_cell('padded-C24-bp', 2, 24, 3, 7, 'mix', 'bp', pad=4),
    ]


def all_cells():
    return matrix_cells() + extra_cells()


CELLS = {c['name']: c for c in all_cells()}


def descriptor(cell):
    """(gdiv, stride_bo[L], stride_g, stride_v[L], stride_px) in elements, as ops._pyramid writes them for a dense pyramid; here also
    for a pixel stride wider than the row"""
    px = cell['stride_px']
    pixels = [h * w for h, w in cell['sizes']]
    gdiv, stride_g = (cell['G'], cell['C']) if cell['pyr'] == 'grouped' else (1, 0)
    return gdiv, [cell['N'] * n * px for n in pixels], stride_g, [n * px for n in pixels], px


def kernel_of(cell):
    """Which kernel launch_bwd (csrc/msmv_sampling_bwd.hip) picks: the C = 64 kernel iff C == 64, stride_px < 2^20 and, per level,
    stride_v N + H W stride_px < 2^31 - 1 (everything below the (b', group) base fits a 32-bit offset); else the generic one."""
    _, _, _, sv, px = descriptor(cell)
    fast = cell['C'] == 64 and px < (1 << 20)
    for (h, w), v in zip(cell['sizes'], sv):
        fast = fast and v * cell['N'] + h * w * px < 0x7fffffff
    return 'c64' if fast else 'generic'


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
NONFINITE = [(5, 0, float('nan')), (12, 1, float('nan')), (19, 0, float('inf')), (26, 1, float('-inf')), (33, 0, 1e30), (40, 1, -1e30),
             (47, 0, float('nan')), (47, 1, float('inf'))]                    # (flat point index before wrapping, coordinate, value)


def special_rows(n_points):
    return sorted({i % n_points for i, _, _ in NONFINITE})


def nonfinite_rows(loc):
    """flat indices of the points with a NaN or Inf in x or y: no level is read for them"""
    return (~torch.isfinite(loc.view(-1, 3)[:, :2]).all(1)).nonzero().flatten().tolist()


def make_inputs(cell, seed=0):
    """(features [B', N, H, W, C] per level, loc fp32, weights, grad_out [B', Q, C, P], pre-filled feature gradients like the features)"""
    L, C, P, N, Bp, Q_ = cell['L'], cell['C'], cell['P'], cell['N'], cell['Bp'], cell['Q']
    g = torch.Generator().manual_seed(seed + 1000 * L + 10 * C + P + 100000 * N)
    feats = [torch.randn(Bp, N, h, w, C, generator=g) for h, w in cell['sizes']]
    loc = edge_locs(Bp, Q_, P, N, [SIZES[0]], g)
    for b, q in ((min(2, Bp - 1), min(3, Q_ - 1)), (Bp - 1, Q_ - 1)):              # all P points of a query on one pixel
        loc[b, q, :, :2] = loc[b, q, 0, :2].clamp(0.1, 0.9) + 1e-3 * torch.rand(P, 2, generator=g)
    flat = loc.view(-1, 3)
    for i, k, v in NONFINITE:
        flat[i % flat.shape[0], k] = v
    wts = torch.softmax(torch.randn(Bp, Q_, P, L, generator=g), -1)
    gout = torch.randn(Bp, Q_, C, P, generator=g)
    pre = [PREFILL * torch.randn(f.shape, generator=g) for f in feats]
    return feats, loc, wts, gout, pre


def to_grouped(f, G):
    """[B', N, H, W, C] (b' = bt G + g) -> the grouped channels-last [B T N, H, W, G C]"""
    Bp, N, H, W, C = f.shape
    return f.reshape(Bp // G, G, N, H, W, C).permute(0, 2, 3, 4, 1, 5).reshape(Bp // G * N, H, W, G * C).contiguous()


def from_grouped(f, G, N):
    BTN, H, W, GC = f.shape
    return f.reshape(BTN // N, N, H, W, G, GC // G).permute(0, 4, 1, 2, 3, 5).reshape(BTN // N * G, N, H, W, GC // G).contiguous()


def device_rows(cell, f):
    """one level as the [pixels, row] matrix the call addresses (row = the payload of a pixel; the buffer's ld is stride_px)"""
    f = to_grouped(f, cell['G']) if cell['pyr'] == 'grouped' else f
    return f.reshape(-1, f.shape[-1])


def host_level(cell, rows, l):
    """the inverse of device_rows for level l"""
    h, w = cell['sizes'][l]
    if cell['pyr'] == 'grouped':
        return from_grouped(rows.reshape(-1, h, w, cell['G'] * cell['C']), cell['G'], cell['N'])
    return rows.reshape(cell['Bp'], cell['N'], h, w, cell['C'])


def device_gout(cell, gout):
    return to_mix(gout, cell['B'], cell['T'], cell['G']).contiguous() if cell['layout'] == 'mix' else gout


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def restate(feats, loc, wts, gout, dt=torch.float64, exact=(False, False), contracted=False):
    """The backward of the sampler, every value in ``dt``; feats [B', N, H, W, C] per level, loc fp32 [B', Q, P, 3], wts [B', Q, P, L],
    gout [B', Q, C, P].  ``exact``: per axis (h, w), the bilinear fraction from the exact product instead of the fp32-rounded one;
    ``contracted`` (with dt = float32): round that fraction once to fp32, which is what an fma gives.
    Returns dict(gf, gloc, gw: the gradients; gf_A, gloc_A, gw_A: the sums of the absolute values of their terms; gf_n: live taps per
    pixel [B', N, H, W]; gloc_n, gw_n: ints)."""
    assert loc.dtype == torch.float32
    Bp, N, _, _, C = feats[0].shape
    Q_, P = loc.shape[1:3]
    L = len(feats)
    g = gout.to(dt).permute(0, 1, 3, 2)                                  # [B', Q, P, C]
    x, y = loc[..., 0], loc[..., 1]
    z = loc[..., 2] * (N - 1)                                            # fp32
    view = torch.where(z >= 0, torch.floor(z + 0.5), torch.ceil(z - 0.5)).long().clamp(0, N - 1)      # C round(): half away from zero
    b_ix = torch.arange(Bp)[:, None, None].expand(Bp, Q_, P)
    out = dict(gf=[], gf_A=[], gf_n=[], gloc=torch.zeros(Bp, Q_, P, 3, dtype=dt), gloc_A=torch.zeros(Bp, Q_, P, 3, dtype=dt),
               gw=torch.zeros(Bp, Q_, P, L, dtype=dt), gw_A=torch.zeros(Bp, Q_, P, L, dtype=dt), gloc_n=4 * C * L, gw_n=4 * C)

    def fraction(coord, m, prod, fl, ex):
        """(fraction, 1 - fraction): both exact in fp64; ``contracted``: each rounded ONCE to fp32, as the two fmas of the kernels'
        corner_frac do -- not the complement taken from the rounded fraction, which next to a pixel boundary (fraction -> 1) leaves
        the small coefficient with a relative error far above U"""
        lo = (coord.double() * m if ex else prod.double()) - fl.double()
        hi = 1 - lo
        if ex and contracted:
            lo, hi = lo.float(), hi.float()
        return lo.to(dt), hi.to(dt)

    for l, f in enumerate(feats):
        f = f.to(dt)
        H, W = f.shape[2:4]
        h_im, w_im = y * (H - 1), x * (W - 1)                            # fp32: the kernel's products
        ok = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)         # false for NaN
        h_im, w_im = torch.where(ok, h_im, torch.zeros_like(h_im)), torch.where(ok, w_im, torch.zeros_like(w_im))
        yy, xx = torch.where(ok, y, torch.zeros_like(y)), torch.where(ok, x, torch.zeros_like(x))
        hf, wf = torch.floor(h_im), torch.floor(w_im)
        (lh, hh), (lw, hw) = fraction(yy, H - 1, h_im, hf, exact[0]), fraction(xx, W - 1, w_im, wf, exact[1])
        h0, w0 = hf.long(), wf.long()
        wl = wts[..., l].to(dt)
        gf, gfA, gfn = torch.zeros_like(f), torch.zeros_like(f), torch.zeros(f.shape[:4], dtype=torch.int64)
        # corner k = 2 kh + kw: bilinear coefficient, d coefficient / d w_im, d coefficient / d h_im
        for dh, dw, cw, dcx, dcy in ((0, 0, hh * hw, -hh, -hw), (0, 1, hh * lw, hh, -lw), (1, 0, lh * hw, -lh, hw), (1, 1, lh * lw, lh, lw)):
            hc, wc = h0 + dh, w0 + dw
            inb = ok & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
            hcc, wcc = hc.clamp(0, H - 1), wc.clamp(0, W - 1)
            live = inb[..., None].to(dt)
            gv = g * f[b_ix, view, hcc, wcc] * live                       # [B', Q, P, C]: g_c v_c of a live corner, else 0
            out['gw'][..., l] += (cw[..., None] * gv).sum(-1)
            out['gw_A'][..., l] += (cw[..., None] * gv).abs().sum(-1)
            tx, ty = (dcx * wl * (W - 1))[..., None] * gv, (dcy * wl * (H - 1))[..., None] * gv
            out['gloc'][..., 0] += tx.sum(-1)
            out['gloc'][..., 1] += ty.sum(-1)
            out['gloc_A'][..., 0] += tx.abs().sum(-1)
            out['gloc_A'][..., 1] += ty.abs().sum(-1)
            term = (cw * wl)[..., None] * g * live
            gf.index_put_((b_ix, view, hcc, wcc), term, accumulate=True)
            gfA.index_put_((b_ix, view, hcc, wcc), term.abs(), accumulate=True)
            gfn.index_put_((b_ix, view, hcc, wcc), inb.long(), accumulate=True)
        out['gf'].append(gf)
        out['gf_A'].append(gfA)
        out['gf_n'].append(gfn)
    return out


def references(feats, loc, wts, gout):
    """the fp64 restatement under the four admissible definitions of the bilinear fractions"""
    return [restate(feats, loc, wts, gout, torch.float64, exact=d) for d in DEFINITIONS]


def excess(got, refs, key, n, pre=None):
    """max over elements of min over definitions of |got - ref_v| / ((n + SLACK) U A_v); an element whose A_v is 0 under every definition
    must be exactly 0 (Inf otherwise).  ``pre``: what the buffer held before the call -- one more term."""
    got = got.double()
    n = torch.as_tensor(n, dtype=torch.float64)
    if n.dim() and n.dim() < got.dim():
        n = n[..., None]
    best = torch.full(got.shape, float('inf'), dtype=torch.float64)
    for r in refs:
        ref, A = r[key], r[key + '_A']
        if isinstance(ref, list):
            raise TypeError('one level at a time')
        ref, A, terms = (ref, A, n) if pre is None else (ref + pre.double(), A + pre.double().abs(), n + 1)
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ((terms + SLACK) * U * A))           # x / 0 = inf for x > 0
        best = torch.minimum(best, torch.nan_to_num(ratio, nan=float('inf')))
    return best.max().item() if best.numel() else 0.0


def level_refs(refs, l):
    return [dict(gf=r['gf'][l], gf_A=r['gf_A'][l]) for r in refs]


def check_outputs(refs, gloc, gw, gfeats, pre=None):
    """{'grad_loc' | 'grad_weights' | 'grad_feats': worst error / bound}; also asserts what is exact: the view component of grad_loc is
    0, and a feature-gradient element that no live tap reaches (or whose terms are all zero) holds what it held"""
    r0 = refs[0]
    assert bool((gloc[..., 2] == 0).all()), 'grad_loc[..., 2] is not exactly 0'
    worst = {'grad_loc': excess(gloc[..., :2], [dict(gloc=r['gloc'][..., :2], gloc_A=r['gloc_A'][..., :2]) for r in refs], 'gloc', r0['gloc_n']),
             'grad_weights': excess(gw, refs, 'gw', r0['gw_n']), 'grad_feats': 0.0}
    for l, got in enumerate(gfeats):
        before = pre[l] if pre is not None else torch.zeros_like(got)
        dead = torch.stack([r['gf_A'][l] for r in refs]).amax(0) == 0
        assert torch.equal(got[dead].view(torch.int32), before[dead].view(torch.int32)), 'level %d: an element without a live term changed' % l
        live_got = torch.where(dead, torch.zeros_like(got), got)
        live_pre = torch.where(dead, torch.zeros_like(got), before)            # a dead element now reads 0 against 0
        worst['grad_feats'] = max(worst['grad_feats'], excess(live_got, level_refs(refs, l), 'gf', r0['gf_n'][l], pre=live_pre if pre is not None else None))
    return worst


@functools.lru_cache(maxsize=None)
def cell_case(name):
    """One cell's inputs, its four fp64 references and the fp32 restatement's own ratios, computed once and shared (read-only)."""
    cell = CELLS[name]
    feats, loc, wts, gout, pre = make_inputs(cell)
    refs = references(feats, loc, wts, gout)
    r32 = restate(feats, loc, wts, gout, torch.float32)
    own = check_outputs(refs, r32['gloc'], r32['gw'], r32['gf'])
    return dict(cell=cell, feats=feats, loc=loc, wts=wts, gout=gout, pre=pre, refs=refs, fp32=own)


# ---- what the cell list must reach (asserted by the host test) -------------------------------------------------------------------------
def coverage(cells):
    """item of the issue's list -> the cells that reach it"""
    def has(pred):
        return [c['name'] for c in cells if pred(c)]
    gen = lambda c: kernel_of(c) == 'generic'
    return {
        'L = 1, C = 64 kernel': has(lambda c: c['L'] == 1 and not gen(c)),
        'L = 1, generic kernel': has(lambda c: c['L'] == 1 and gen(c)),
        'generic kernel, mixing grad_out layout': has(lambda c: gen(c) and c['layout'] == 'mix'),
        'generic kernel, C > 64 with a full second trip': has(lambda c: gen(c) and c['C'] == 128),
        'generic kernel, C > 64 with a partly dead second trip': has(lambda c: gen(c) and 64 < c['C'] < 128),
        'generic kernel, C no multiple of 16': has(lambda c: gen(c) and c['C'] % 16 and c['C'] % 4 == 0),
        'generic kernel, C no multiple of 4': has(lambda c: gen(c) and c['C'] % 4),
        'generic kernel, grouped pyramid': has(lambda c: gen(c) and c['pyr'] == 'grouped' and c['G'] > 1),
        'C = 64 falls back to the generic kernel at stride_px >= 2^20': has(lambda c: gen(c) and c['C'] == 64),
        'one camera (nm1 = 0)': has(lambda c: c['N'] == 1),
        'camera counts 2 and 7': has(lambda c: c['N'] == 2) and has(lambda c: c['N'] == 7),
        'a one-column level': has(lambda c: any(w == 1 and h > 1 for h, w in c['sizes'])),
        'a 1 x 1 level': has(lambda c: (1, 1) in c['sizes']),
        'pixel stride wider than the row, C = 64 kernel': has(lambda c: c['pad'] and not gen(c)),
        'pixel stride wider than the row, generic kernel': has(lambda c: c['pad'] and gen(c)),
        'P = 32, C = 64 kernel': has(lambda c: c['P'] == 32 and not gen(c)),
        'P = 32, generic kernel': has(lambda c: c['P'] == 32 and gen(c)),
        "B' Q no multiple of 4": has(lambda c: c['Bp'] * c['Q'] % 4),
        "B' Q = 1": has(lambda c: c['Bp'] * c['Q'] == 1),
    }
