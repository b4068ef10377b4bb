"""Cases, input generators and a numpy restatement of the loader's image geometry (resize with Pillow's 8-bit bicubic resampler, crop
with black fill, mirror, HWC -> CHW), for tests/test_image_geom_host.py, tests/test_gpu_image_geom.py and
tests/golden/make_golden_image_geom.py.  The restatement is written from the description of the resampler, with no dependency on Pillow:

  * per output index xx of an axis of ``in_size`` resized to ``out_size``: scale = in_size / out_size, filterscale = max(scale, 1),
    support = 2 * filterscale, ksize = 2 * ceil(support) + 1, center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
    xmax = min(int(center + support + 0.5), in_size); weights bicubic((x + xmin - center + 0.5) * (1 / filterscale)) with a = -0.5,
    summed in order, each divided by the sum, then int(+-0.5 + w * 2^22) by sign -- all in double;
  * each pass: int accumulator from 1 << 21, plus pixel * coefficient, >> 22, clamp to 0 .. 255; the horizontal pass first, stored as
    uint8, then the vertical pass over those values;
  * crop: a coordinate outside the resized image gives 0; mirror: output column x reads cropped column fW - 1 - x.
"""
import math

import numpy as np

KMAX = 16                    # SBEV_GEOM_KMAX
PRECISION_BITS = 22


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_of(in_size, out_size):
    return 2 * int(math.ceil(2.0 * max(in_size / out_size, 1.0))) + 1


def coeffs(in_size, out_size):
    """(bounds int32 [out_size, 2] = (first, count), coefficients int32 [out_size, ksize]) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img, bounds, kk):
    """one pass along axis 1 of uint8 [rows, in_size, C] -> uint8 [rows, out_size, C]"""
    out = np.empty((img.shape[0], len(bounds), img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (first, count) in enumerate(bounds):
        acc = np.full((img.shape[0], img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(count):
            acc += src[:, first + t] * int(kk[xx, t])
        assert np.abs(acc).max() < 2 ** 31
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, new_w, new_h):
    """uint8 [H, W, C] -> uint8 [new_h, new_w, C]: the horizontal pass, then the vertical one."""
    H, W, _ = img.shape
    tmp = _pass(img, *coeffs(W, new_w))
    return _pass(tmp.transpose(1, 0, 2), *coeffs(H, new_h)).transpose(1, 0, 2)


def transform(img, resize_dims, crop, flip):
    """One image of the loader's geometry: uint8 [H, W, 3] -> uint8 [3, fH, fW] (resize, crop with zero fill, mirror, CHW)."""
    new_w, new_h = resize_dims
    x0, y0, x1, y1 = crop
    r = resize(img, new_w, new_h)
    out = np.zeros((y1 - y0, x1 - x0, img.shape[2]), dtype=np.uint8)
    ya, yb, xa, xb = max(y0, 0), min(y1, new_h), max(x0, 0), min(x1, new_w)
    if yb > ya and xb > xa:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = r[ya:yb, xa:xb]
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def tables(H, W, resize_dims, crop):
    """What sbev_image_geom_plan writes: (column bounds [fW, 2], row bounds [fH, 2], column coefficients [fW, KMAX], row coefficients
    [fH, KMAX]) for the fW columns and fH rows the crop keeps; an index outside the resized image has count 0."""
    new_w, new_h = resize_dims
    x0, y0, x1, y1 = crop

    def axis(in_size, out_size, lo, hi):
        b, k = coeffs(in_size, out_size)
        assert k.shape[1] <= KMAX
        bounds, kk = np.zeros((hi - lo, 2), dtype=np.int32), np.zeros((hi - lo, KMAX), dtype=np.int32)
        for j in range(lo, hi):
            if 0 <= j < out_size:
                bounds[j - lo] = b[j]
                kk[j - lo, :k.shape[1]] = k[j]
        return bounds, kk

    xb, xk = axis(W, new_w, x0, x1)
    yb, yk = axis(H, new_h, y0, y1)
    return xb, yb, xk, yk


# ---------------------------------------------------------------- inputs
def random_bytes(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def extremes(shape, seed):
    """a 0 / 255 random pattern: bicubic overshoot drives both clamps"""
    return (np.random.RandomState(seed).randint(0, 2, size=shape) * 255).astype(np.uint8)


# ---------------------------------------------------------------- the case list
def case(name, H, W, resize_dims, crop, flip=False):
    return dict(name=name, H=H, W=W, resize_dims=tuple(resize_dims), crop=tuple(crop), flip=bool(flip),
                fH=crop[3] - crop[1], fW=crop[2] - crop[0])


def _scaled(H, W, f):
    return int(W * f), int(H * f)


TILE_W, TILE_H = 64, 16      # the kernel's output tile (sbev_image_geom_plan reports it; the host test checks these two)

CASES = [
    case('down_041', 37, 53, _scaled(37, 53, 0.41), (0, 0, 21, 15)),                    # ksize 13 horizontally, 11 vertically
    case('pure_crop', 33, 47, (47, 33), (5, 7, 36, 29)),                                # factor 1.0
    case('one_axis', 40, 50, (50, 17), (0, 0, 50, 17)),                                 # width unchanged
    case('enlarge_13', 23, 31, _scaled(23, 31, 1.3), (3, 2, 38, 27)),                   # ksize 5
    case('overhang_right', 30, 60, (34, 17), (0, 1, 45, 14)),                           # newW 34 < fW 45: 11 zero columns
    case('negative_crop_y', 30, 60, (34, 17), (4, -5, 30, 15)),                         # zero rows on top
    case('overhang_mirror', 30, 60, (34, 17), (0, 1, 45, 14), flip=True),               # the zeros land on the left
    case('mid_image', 90, 120, _scaled(90, 120, 0.55), (9, 11, 9 + 40, 11 + 33)),       # halo partly outside the source: below
    case('whole_small', 50, 70, _scaled(50, 70, 0.5), (0, 0, 35, 25), flip=True),       # first / last row and column of the source
] + [
    case('tile_%dx%d' % (fh, fw), 61, 167, _scaled(61, 167, 0.47), (6, 5, 6 + fw, 5 + fh), flip=(fw + fh) % 2 == 1)
    for fh in (TILE_H - 1, TILE_H, TILE_H + 1) for fw in (TILE_W - 1, TILE_W, TILE_W + 1)
]
CASE_NAMES = [c['name'] for c in CASES]

# the r50 config's geometry on full camera frames
R50_CONF = dict(H=900, W=1600, final_dim=(256, 704), resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True)
FULL_EVAL = case('full_eval', 900, 1600, (704, 396), (0, 140, 704, 396))
FULL_038 = case('full_038_mirror', 900, 1600, (608, 342), (0, 86, 704, 342), flip=True)

# fixture G17: small configs in the configs' vocabulary, each run in training mode under G17_SEEDS and once in eval mode
G17_CONFS = {
    'r50_small': dict(H=36, W=64, final_dim=(10, 30), resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True),
    'no_flip': dict(H=45, W=80, final_dim=(16, 30), resize_lim=(0.4, 0.7), bot_pct_lim=(0.0, 0.2), rot_lim=(0.0, 0.0), rand_flip=False),
    'tall_crop': dict(H=48, W=72, final_dim=(30, 24), resize_lim=(0.9, 1.4), bot_pct_lim=(0.0, 0.1), rot_lim=(0.0, 0.0), rand_flip=True),
}
G17_SEEDS = (0, 1, 2, 3)
G17_VIEWS = 2                # images per call; one transform for all of them
G17_CALLS = ['train%d' % s for s in G17_SEEDS] + ['eval']
G17_KEYS = [(conf, call) for conf in G17_CONFS for call in G17_CALLS]


def g17_params(g, conf, call):
    """the recorded sample_augmentation() tuple of one call: (resize, resize_dims, crop, flip, rotate)"""
    t = np.asarray(g['%s_%s_tuple' % (conf, call)], dtype=np.float64)
    return float(t[0]), (int(t[1]), int(t[2])), tuple(int(v) for v in t[3:7]), bool(t[7]), float(t[8])
