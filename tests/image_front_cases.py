"""Shapes, input generators and a plain numpy restatement (fp64) of the image front end, for tests/test_image_front_host.py,
tests/test_gpu_image_front.py and tests/golden/make_golden_image_front.py.  The restatement is written from the description of the
pipeline (float(src) as RGB, brightness, contrast, RGB -> HSV, saturation, hue, one wrap, HSV -> RGB, contrast, channel permutation,
RGB -> BGR, to_rgb flip, mean / std, zero pad, GridMask), not from anybody's code; it covers the cases fixture G16 does not hold."""
import numpy as np

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]         # the configs' img_norm_cfg (to_rgb=True)
NORM_CFG = dict(mean=MEAN, std=STD, to_rgb=True)
DATA_AUG = dict(img_color_aug=True, img_norm_cfg=NORM_CFG, img_pad_cfg=dict(size_divisor=32))

# fixture G16's calls: name -> (shape, training, seed index into the fixture's 'seeds')
G16_CALLS = ('train_a', 'train_b', 'eval', 'aligned')
G16_SHAPES = {'train_a': (12, 3, 37, 45), 'train_b': (12, 3, 37, 45), 'eval': (2, 3, 37, 45), 'aligned': (2, 3, 64, 96)}
G16_TRAINING = {'train_a': True, 'train_b': True, 'eval': False, 'aligned': True}
G16_VIEWS = {'train_a': 6, 'train_b': 6, 'eval': 2, 'aligned': 2}      # N of [B, N, ...]: B = n / N samples

BRIGHT, CONTRAST, SAT, HUE, SWAP = 1, 2, 4, 8, 16


def make_images(shape, seed, special=True):
    """uint8 [n, 3, H, W]; with ``special`` image 0 is all 0, image 1 all 255 and image 2 grey (its three channels equal)."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=shape).astype(np.uint8)
    if special and shape[0] >= 3:
        img[0] = 0
        img[1] = 255
        img[2] = img[2, :1]
    return img


def padded(H, W, div):
    return -(-H // div) * div, -(-W // div) * div


def grid_mask_keep(Hp, Wp, d, l, st_h, st_w):
    """bool [Hp, Wp]: the pixels GridMask KEEPS.  A grid of stripes of thickness l and period d is laid over a canvas of 1.5 x the
    (padded) size, at most (canvas // d) stripes per direction starting at st; the image is the canvas' centre crop; a pixel survives
    iff a row stripe or a column stripe covers it."""
    hh, ww = int(1.5 * Hp), int(1.5 * Wp)

    def on(size, count, st):
        line = np.zeros(size, dtype=bool)
        for i in range(count):
            lo = d * i + st
            line[lo:min(lo + l, size)] = True
        return line

    rows = on(hh, hh // d, st_h)[(hh - Hp) // 2:(hh - Hp) // 2 + Hp]
    cols = on(ww, ww // d, st_w)[(ww - Wp) // 2:(ww - Wp) // 2 + Wp]
    return rows[:, None] | cols[None, :]


def _pymod(a, b):
    """remainder with the sign of the (positive) divisor"""
    return a - b * np.floor(a / b)


def distort_f64(rgb, flags, mode, delta, alpha, sat, hue, perm):
    """One image [3, H, W] (float64, RGB order) through the photometric distortion; returns RGB order after the permutation."""
    x = rgb.astype(np.float64).copy()
    if flags & BRIGHT:
        x = x + delta
    if (flags & CONTRAST) and mode == 0:
        x = x * alpha
    u = x / 255.0
    mx, mn = u.max(0), u.min(0)
    arg = u.argmax(0)                              # first maximum
    dc = mx - mn
    v = mx
    s = dc / (mx + 1e-8)
    dc = np.where(dc == 0, 1.0, dc)
    rc, gc, bc = mx - u[0], mx - u[1], mx - u[2]
    cand = np.stack([bc - gc, (rc - bc) + 2.0 * dc, (gc - rc) + 4.0 * dc]) / dc
    h = np.take_along_axis(cand, arg[None], 0)[0]
    h = _pymod(h / 6.0, 1.0) * 360.0
    v = v * 255.0
    if flags & SAT:
        s = s * sat
    if flags & HUE:
        h = h + hue
    h = np.where(h > 360, h - 360, h)
    h = np.where(h < 0, h + 360, h)
    hn, vn = h / 360.0, v / 255.0
    h6 = hn * 6
    hi = _pymod(np.floor(h6), 6)
    f = _pymod(h6, 6) - hi
    p, q, t = vn * (1 - s), vn * (1 - f * s), vn * (1 - (1 - f) * s)
    k = hi.astype(np.int64)
    sextants = [(vn, t, p), (q, vn, p), (p, vn, t), (p, q, vn), (t, p, vn), (vn, p, q)]
    out = np.stack([np.choose(k, [sx[c] for sx in sextants]) for c in range(3)]) * 255.0
    if (flags & CONTRAST) and mode == 1:
        out = out * alpha
    if flags & SWAP:
        out = out[list(perm)]
    return out


def pipeline_f64(img, mean, std, to_rgb, div, rows=None, colour=False):
    """The whole stage in float64 for img [n, 3, H, W] (BGR planes as the loader delivers them).  ``rows``: the structured parameter
    rows (fields flags, mode, delta, alpha, sat, hue, perm, mask) or None; ``colour``: the distortion runs (then for EVERY image, also
    one whose flags are all clear: the HSV round trip is part of it).  Returns [n, 3, Hp, Wp] float64."""
    n, _, H, W = img.shape
    Hp, Wp = padded(H, W, div)
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64)         # the device holds them in fp32
    std = np.asarray(std, dtype=np.float32).astype(np.float64)
    out = np.zeros((n, 3, Hp, Wp))
    for i in range(n):
        x = img[i].astype(np.float64)
        if colour:
            r = rows[i]
            rgb = distort_f64(x[::-1], int(r['flags']), int(r['mode']), float(r['delta']), float(r['alpha']), float(r['sat']),
                              float(r['hue']), [int(v) for v in r['perm']])
            x = rgb[::-1]
        if to_rgb:
            x = x[::-1]
        x = (x - mean[:, None, None]) / std[:, None, None]
        out[i, :, :H, :W] = x
        if rows is not None and rows[i]['mask'][0]:
            _, d, l, st_h, st_w = [int(v) for v in rows[i]['mask']]
            out[i] *= grid_mask_keep(Hp, Wp, d, l, st_h, st_w)[None]
    return out
