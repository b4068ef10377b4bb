"""Yardsticks of the atomics-free feature gradient (tests/test_gpu_det_feature_grad.py on the device, tests/test_det_feature_grad_host.py
for what can be checked without one).

The definition under test (include/sbev_hip.h, sbev_msmv_bwd_taps): taps are numbered i = (((b' Q + q) P + p) L + l) 4 + k; a live tap
has key (l << 56) | off and coefficient (ch * cwid) * wl; per destination, acc = +0, then acc = acc + coef_i * g_i[c] over its live taps
in ascending i (product rounded, then the sum), then ONE addition into the gradient buffer.

  * host_feature_grad: that sum in numpy float32 from DEVICE-produced keys / coefs -- the bit-for-bit reference of the sum kernel;
  * ref_taps: an independent restatement of the tap geometry (fp64 arithmetic behind fp32 coordinate products, as in sampling_cases.py:
    the products decide which taps exist, so they stay in the kernel's precision) -- keys exactly, coefs to 1e-6."""
import numpy as np
import torch

SIZES = [(9, 14), (5, 7), (3, 4), (2, 2), (1, 3)]
CASES = [(6, 4, 64), (1, 5, 64), (9, 2, 64), (5, 3, 24)]          # (P, L, C): the sampler backward's tail cases
BP, Q, N = 3, 10, 6
KEY_DEAD = np.int64(2 ** 63 - 1)
LEVEL_SHIFT = 56


def case_id(case):
    return 'P%d-L%d-C%d' % case


def make_case(P, L, C, Bp=BP, Q=Q, seed=None):
    """(loc, weights, grad_out [B', Q, C, P]) of one case: locations rand * 1.3 - 0.15, the exact points (0, 1) and (0.5, 0.5), one point
    with a NaN coordinate."""
    g = torch.Generator().manual_seed(P * 10 + L if seed is None else seed)
    loc = torch.rand(Bp, Q, P, 3, generator=g) * 1.3 - 0.15
    loc[..., 2] = torch.randint(0, N, (Bp, Q, P), generator=g).float() / (N - 1)
    loc[0, 0, 0, :2] = torch.tensor([0.0, 1.0])
    loc[0, 1, 0, :2] = torch.tensor([0.5, 0.5])
    loc[1, 2, 0, 0] = float('nan')
    wts = torch.softmax(torch.randn(Bp, Q, P, L, generator=g), -1)
    gout = torch.randn(Bp, Q, C, P, generator=g)
    return loc, wts, gout


def to_rows(gout):
    """grad_out [B', Q, C, P] -> the tap rows [B' * Q * P, C] (row of tap i: i // (4 L)) as float32 numpy."""
    Bp, Q_, C, P = gout.shape
    return np.ascontiguousarray(gout.permute(0, 1, 3, 2).reshape(Bp * Q_ * P, C).cpu().numpy(), dtype=np.float32)


def to_mix(gout, B, T, G):
    """[B', Q, C, P] -> the mixing layout [B, Q, G, T * P, C] (b' = (b * T + t) * G + g)."""
    Bp, Q_, C, P = gout.shape
    return gout.reshape(B, T, G, Q_, C, P).permute(0, 3, 2, 1, 5, 4).reshape(B, Q_, G, T * P, C).contiguous()


def host_feature_grad(keys, coefs, rows, bufs, L, descending=False):
    """The sum of the definition.  keys [n] int64, coefs [n] float32 (device-produced), rows [n / (4 L), C] float32, bufs: one flat float32
    array per level (the pre-filled gradient buffers; copied).  Stable ascending sort, then per run of equal keys sequential float32
    sums in run order (``descending``: the same terms back to front -- another order, for tests that must tell orders apart)."""
    keys = np.asarray(keys, dtype=np.int64)
    coefs = np.asarray(coefs, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.float32)
    out = [np.array(b, dtype=np.float32, copy=True).reshape(-1) for b in bufs]
    C = rows.shape[1]
    order = np.argsort(keys, kind='stable')
    sk = keys[order]
    n = len(keys)
    j = 0
    while j < n and sk[j] != KEY_DEAD:
        e = j
        while e < n and sk[e] == sk[j]:
            e += 1
        run = order[j:e]
        if descending:
            run = run[::-1]
        acc = np.zeros(C, dtype=np.float32)
        for i in run:
            prod = coefs[i] * rows[i // (4 * L)]              # float32 * float32 array: rounded once
            acc = acc + prod                                  # rounded once
        lvl, off = int(sk[j] >> LEVEL_SHIFT), int(sk[j] & ((1 << LEVEL_SHIFT) - 1))
        out[lvl][off:off + C] = out[lvl][off:off + C] + acc
        j = e
    return out


def ref_taps(loc, wts, sizes, n_views, gdiv, stride_bo, stride_g, stride_v, stride_px):
    """Independent restatement of the tap list: (keys [n] int64, coefs [n] float64) for loc [B', Q, P, 3], wts [B', Q, P, L] (torch, fp32)
    over levels ``sizes`` addressed by the C ABI's strides (elements).  Vectorised over [B', Q, P, L, 4]."""
    loc = loc.cpu().numpy().astype(np.float32)
    wts = wts.cpu().numpy().astype(np.float32)
    Bp, Q_, P, _ = loc.shape
    L = len(sizes)
    f32 = np.float32
    x, y, z = loc[..., 0], loc[..., 1], loc[..., 2]
    with np.errstate(invalid='ignore'):
        zz = (z * f32(n_views - 1)).astype(np.float32).astype(np.float64)
        view = np.clip(np.where(np.isnan(zz), 0, np.sign(zz) * np.floor(np.abs(zz) + 0.5)), 0, n_views - 1).astype(np.int64)      # roundf
    bp = np.arange(Bp, dtype=np.int64)[:, None, None]
    bo, gi = bp // gdiv, bp % gdiv
    keys = np.empty((Bp, Q_, P, L, 4), dtype=np.int64)
    coefs = np.zeros((Bp, Q_, P, L, 4), dtype=np.float64)
    for l, (H, W) in enumerate(sizes):
        with np.errstate(invalid='ignore'):
            h_im = (y * f32(H - 1)).astype(np.float32)          # fp32 products: they pick the taps
            w_im = (x * f32(W - 1)).astype(np.float32)
            ok = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)          # False for NaN
        h64 = np.where(ok, h_im, 0).astype(np.float64)
        w64 = np.where(ok, w_im, 0).astype(np.float64)
        hf, wf = np.floor(h64), np.floor(w64)
        lh, lw = h64 - hf, w64 - wf
        for k in range(4):
            kh, kw = k >> 1, k & 1
            hc, wc = hf.astype(np.int64) + kh, wf.astype(np.int64) + kw
            live = ok & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
            off = bo * stride_bo[l] + gi * stride_g + view * stride_v[l] + (np.clip(hc, 0, H - 1) * W + np.clip(wc, 0, W - 1)) * stride_px
            keys[:, :, :, l, k] = np.where(live, (np.int64(l) << LEVEL_SHIFT) | off, KEY_DEAD)
            c = ((lh if kh else 1 - lh) * (lw if kw else 1 - lw)) * wts[..., l].astype(np.float64)
            coefs[:, :, :, l, k] = np.where(live, c, 0.0)
    return keys.reshape(-1), coefs.reshape(-1)
