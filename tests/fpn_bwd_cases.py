"""The FPN neck's backward: the fp64 restatement of its definition (include/sbev_hip.h: sbev_fpn_backward) over fpn_cases' cases and
helpers, shared by test_fpn_bwd_host.py, test_gpu_fpn_bwd.py and tools/bench_fpn_train.py.  Like the forward's restatement it uses no
convolution and no interpolation of torch's: a data gradient is the forward's nine shifted einsums over flipped, transposed weights, a
weight gradient nine einsums over pixels, the top-down adjoint sums each parent's children over the ranges of
``sparsebev_amd.fpn.children``.  test_fpn_bwd_host.py holds it against torch.autograd with the roundings off."""
import math

import torch

import fpn_cases as FC
from fpn_cases import BY_NAME, CASES, out_planes, r16  # noqa: F401  (the cases are the forward's)
from sparsebev_amd import fpn

WINDOW = fpn.GRAD_WINDOW_LOG2


# ---------------------------------------------------------------- data
def real_grads(case, seed, scale=1.0):
    """fp32 output gradients (NCHW values), unit scale times ``scale``"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(case.n, 256, h, w, generator=g) * scale for h, w in out_planes(case)]


def integer_grads(case, seed, keep=2):
    """Output gradients in {-2 .. 2} with at most ``keep`` non-zero channels per pixel: with fpn_cases.integer_data every scaled
    intermediate stays an integer that fp16 holds exactly and every weight-gradient sum one that fp32 holds exactly (the tests assert
    both on the restatement before they ask the device)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in out_planes(case):
        x = torch.randint(-2, 3, (case.n, 256, h, w), generator=g).float()
        rank = torch.rand(case.n, 256, h, w, generator=g).argsort(dim=1).argsort(dim=1)
        x = x * (rank < keep)
        x[0, 0, 0, 0] = 2.0                  # amax is 2 whatever the draw
        out.append(x)
    return out


# ---------------------------------------------------------------- the restatement, fp64
def scale_exponent(gP):
    """e with 2^e amax in [2^WINDOW, 2^(WINDOW + 1)), capped at 126; 0 for a zero or non-finite amax"""
    amax = max(float(g.abs().max()) if g.numel() else 0.0 for g in gP)
    if amax == 0.0 or not math.isfinite(amax):
        return 0
    return min(WINDOW - (math.frexp(amax)[1] - 1), 126)


def staged_grads(gP, L, e, rounded=True):
    """g_l: G_l = gP_l (+ the extra levels' gradients at their source pixels, added in order in fp32), times 2^e, rounded to fp16"""
    G = [g.clone() for g in gP[:L]]
    if rounded:
        G = [g.float() for g in G]
    else:
        G = [g.double() for g in G]
    for k, g in enumerate(gP[L:], start=1):
        G[L - 1][:, :, ::2 ** k, ::2 ** k] += g.to(G[L - 1].dtype)
    return [r16(g.double() * 2.0 ** e, rounded) for g in G]


def data_grad3(g, w3, rounded=True):
    """(D, A): conv3x3(g, W3') with W3'[ci, co, ky, kx] = fp16(W3[co, ci, 2 - ky, 2 - kx]), and the sum of absolute products"""
    wt = r16(w3.cpu(), rounded).flip(2, 3).transpose(0, 1).contiguous()
    return FC.conv3x3(g, wt), FC.conv3x3(g.abs(), wt.abs())


def children_sum(child, pH, pW):
    """(S, A, most): per parent pixel the sum of ``child`` over its children, of their absolute values, and the largest child count"""
    n, c, H, W = child.shape
    y0, y1 = fpn.children(pH, H)
    x0, x1 = fpn.children(pW, W)
    S = torch.zeros(n, c, pH, pW, dtype=torch.float64)
    A = torch.zeros_like(S)
    most = 0
    for py in range(pH):
        for px in range(pW):
            blk = child[:, :, int(y0[py]):int(y1[py]), int(x0[px]):int(x1[px])].double()
            S[:, :, py, px] = blk.sum((2, 3))
            A[:, :, py, px] = blk.abs().sum((2, 3))
            most = max(most, blk.shape[2] * blk.shape[3])
    return S, A, most


def shifted(m, ky, kx):
    n, c, H, W = m.shape
    p = torch.zeros(n, c, H + 2, W + 2, dtype=m.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = m
    return p[:, :, ky:ky + H, kx:kx + W]


def weight_grad3(g, m):
    """(gW3 [256, 256, 3, 3], A) in the scaled domain: sum over pixels of g[p, co] m[p + (ky - 1, kx - 1), ci]"""
    m = m.double()
    gw = torch.zeros(g.shape[1], m.shape[1], 3, 3, dtype=torch.float64)
    A = torch.zeros_like(gw)
    for ky in range(3):
        for kx in range(3):
            s = shifted(m, ky, kx)
            gw[:, :, ky, kx] = torch.einsum('nohw,nchw->oc', g, s)
            A[:, :, ky, kx] = torch.einsum('nohw,nchw->oc', g.abs(), s.abs())
    return gw, A


def backward_reference(xs, params, M, gP, rounded=True):
    """The whole backward in fp64 from the forward's merged laterals M (fpn_cases.reference) and the output gradients gP (NCHW).
    Returns a dict: e, and per level lists g (scaled staged gradients), D, gM (scaled), gC, gW3, gWlat, gc, gblat (unscaled, fp64 --
    the caller rounds gC to the inputs' dtype).  ``rounded`` False switches every fp16 rounding and the scale off."""
    L = len(xs)
    e = scale_exponent(gP) if rounded else 0
    down = 2.0 ** -e
    g = staged_grads(gP, L, e, rounded)
    out = dict(e=e, g=g, D=[], gM=[], gC=[], gW3=[], gWlat=[], gc=[], gblat=[])
    for l in range(L):
        D, _ = data_grad3(g[l], params['fpn_convs.%d.conv.weight' % l], rounded)
        out['D'].append(D)
        if l > 0:
            D = D + children_sum(out['gM'][l - 1], D.shape[2], D.shape[3])[0]
        out['gM'].append(r16(D, rounded))
    for l in range(L):
        gm = out['gM'][l]
        wl = r16(params['lateral_convs.%d.conv.weight' % l].cpu(), rounded)[:, :, 0, 0]
        out['gC'].append(down * torch.einsum('nohw,oc->nchw', gm, wl))
        out['gW3'].append(down * weight_grad3(g[l], M[l])[0])
        out['gWlat'].append(down * torch.einsum('nohw,nchw->oc', gm, r16(xs[l].cpu(), rounded))[:, :, None, None])
        out['gc'].append(down * g[l].sum((0, 2, 3)))
        out['gblat'].append(down * gm.sum((0, 2, 3)))
    return out


def param_grads(ref):
    """the restatement's parameter gradients under the parameters' names"""
    named = {}
    for l in range(len(ref['gW3'])):
        named['lateral_convs.%d.conv.weight' % l] = ref['gWlat'][l]
        named['lateral_convs.%d.conv.bias' % l] = ref['gblat'][l]
        named['fpn_convs.%d.conv.weight' % l] = ref['gW3'][l]
        named['fpn_convs.%d.conv.bias' % l] = ref['gc'][l]
    return named


# ---------------------------------------------------------------- device helpers (GPU tests and the bench tool)
def make_trainable_neck(case, params, device):
    from sparsebev_amd import FPNNeck
    neck = FPNNeck(case.cin, 256, case.num_outs, trainable=True)
    neck.load_state_dict(params, strict=True)
    return neck.to(device)


def chw_of(case):
    return [(c, h, w) for c, (h, w) in zip(case.cin, case.planes)]


class DeviceBackward:
    """One direct call of the C entry after a no-grad forward: NaN-filled destinations, the workspace kept for the stage tests.
    ``grads``: the parameter gradients under the parameters' names (fp32, on the device); ``gC``: the input gradients or None."""

    def __init__(self, neck, case, xs, gP, in_dtype, g_dtype, device, input_grads=True):
        self.case, self.device = case, device
        self.chw = chw_of(case)
        L = len(xs)
        self.inputs = [FC.channels_last(x.to(device=device, dtype=in_dtype)) for x in xs]
        self.gouts = [FC.channels_last(g.to(device=device, dtype=g_dtype)) for g in gP]
        with torch.no_grad():
            neck(self.inputs, out_dtype=torch.float32)
        self.merged_ws = neck.merged[0]          # level 0 starts the forward's workspace: the merged laterals, level after level
        self.merged = [m.clone() for m in neck.merged]
        self.plan = fpn.backward_plan(self.chw, case.n, case.num_outs, input_grads)
        self.ws = torch.full((max(self.plan['workspace_bytes'], 256),), 0xff, dtype=torch.uint8, device=device)
        nan = lambda *s, dtype=torch.float32: torch.full(s, float('nan'), dtype=dtype, device=device)
        self.gwl = [nan(256, c, 1, 1) for c in case.cin]
        self.gbl = [nan(256) for _ in range(L)]
        self.gw3 = [nan(256, 256, 3, 3) for _ in range(L)]
        self.gb3 = [nan(256) for _ in range(L)]
        self.gC = [nan(case.n, h, w, c, dtype=in_dtype).permute(0, 3, 1, 2) for c, (h, w) in zip(case.cin, case.planes)] if input_grads else None
        self.pack = neck.pack_bwd()
        self.run()

    def run(self, stream=None):
        fpn.backward_raw(self.chw, self.case.n, self.case.num_outs, self.inputs, self.merged_ws, self.gouts, self.pack, self.ws, self.gC,
                         self.gwl, self.gbl, self.gw3, self.gb3, stream)

    @property
    def grads(self):
        named = {}
        for l in range(len(self.gw3)):
            named['lateral_convs.%d.conv.weight' % l] = self.gwl[l]
            named['lateral_convs.%d.conv.bias' % l] = self.gbl[l]
            named['fpn_convs.%d.conv.weight' % l] = self.gw3[l]
            named['fpn_convs.%d.conv.bias' % l] = self.gb3[l]
        return named

    def scale(self):
        """(2^e, 2^-e) as the device wrote them"""
        pair = self.ws[:8].view(torch.float32).cpu()
        return float(pair[0]), float(pair[1])

    def stage(self, what, l):
        """gM_l (fp16, scaled) or D_l (fp32, scaled, l >= 1) as the device left them in the workspace, NCHW values on the CPU"""
        n = self.case.n
        pix = [n * h * w for h, w in self.case.planes]
        h, w = self.case.planes[l]
        if what == 'gM':
            at = self.plan['gm_offset'] + 512 * sum(pix[:l])
            t = self.ws[at:at + 512 * pix[l]].view(torch.float16)
        else:
            at = self.plan['d_offset'] + 1024 * sum(pix[1:l])
            t = self.ws[at:at + 1024 * pix[l]].view(torch.float32)
        return t.view(n, h, w, 256).permute(0, 3, 1, 2).cpu()
