"""Dev tool: time sparsebev_amd.ImageFrontEnd (csrc/image_front.hip, one launch) beside a plain-torch restatement of the reference's
flow on the same device with the same draws -- .float(), the photometric distortion (per-image scalar ops, RGB -> HSV and back over the
whole tensor with stack / gather), mean / std, F.pad, the GridMask multiply; and the inference call (no distortion, no mask) beside its four
torch ops -- and write one JSON line to profiles/image_front.json.

Shapes: B * N in {48, 384} images of 3 x 256 x 704 uint8 (one sample and the recipe's 8 samples of 48 images), to fp32 and to fp16.  The
legs are interleaved in one process, warmed up, timed with HIP events; the figure is the median of three rounds' medians.  The fused
launch is also reported as bytes moved / time (3 H W (1 + 4) or (1 + 2) bytes per image; 256 x 704 needs no padding) and as a fraction
of the float4 copy rate recorded in profiles/optim_step.json.  The comparison is against the torch restatement, never against an earlier
run of the kernel.  The record carries the compiler's register / scratch / LDS figures of every instantiation.  Nothing here is a gate.

    python tools/bench_image_front.py [--iters 20] [--out profiles/image_front.json]
    python tools/bench_image_front.py --resources-only          (no GPU needed: times are written as "NOT measured")
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
import torch.nn.functional as F               # noqa: E402

COPY_RATE = 6.23e12          # bytes / s: profiles/optim_step.json, the update launch
DATA_AUG = dict(img_color_aug=True, img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                img_pad_cfg=dict(size_divisor=32))
BRIGHT, CONTRAST, SAT, HUE, SWAP = 1, 2, 4, 8, 16


def kernel_resources():
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS['image_front.hip'] + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                                                                  os.path.join(build.HERE, 'image_front.hip'), '-o', os.path.join(tmp, 'unit.o')]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'TotalSGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], stdout=subprocess.PIPE).stdout.decode().strip() or m.group(1)
            inst = re.search(r'image_front_kernel<([^>]*)>', name)
            cur = out.setdefault('image_front_kernel<%s>' % inst.group(1) if inst else name, {})
            continue
        for k, v in keys.items():
            m = re.search(r'remark:\s+' + re.escape(k) + r': (\d+)', line)
            if m and cur is not None:
                cur[v] = int(m.group(1))
    return out


def grid_keep(Hp, Wp, d, l, st_h, st_w):
    """GridMask's factor, built on the host as the reference builds it: 1 on the row and column stripes of the centre crop, else 0"""
    hh, ww = int(1.5 * Hp), int(1.5 * Wp)
    rows, cols = np.zeros(hh, np.uint8), np.zeros(ww, np.uint8)
    for i in range(hh // d):
        rows[d * i + st_h:min(d * i + st_h + l, hh)] = 1
    for i in range(ww // d):
        cols[d * i + st_w:min(d * i + st_w + l, ww)] = 1
    rows, cols = rows[(hh - Hp) // 2:(hh - Hp) // 2 + Hp], cols[(ww - Wp) // 2:(ww - Wp) // 2 + Wp]
    return np.maximum(rows[:, None], cols[None, :])


def torch_chain(img, rows, mean, std, out_dtype):
    """The reference's flow restated with torch ops, one pass per step as there: img uint8 [n, 3, H, W] on the device, rows the drawn
    parameters.  The same arithmetic as the fused launch (compared once before the timing)."""
    x = img.float()
    x = x[:, [2, 1, 0]]
    n = x.shape[0]
    for i in range(n):
        if rows['flags'][i] & BRIGHT:
            x[i] += float(rows['delta'][i])
        if rows['flags'][i] & CONTRAST and rows['mode'][i] == 0:
            x[i] *= float(rows['alpha'][i])
    u = x / 255.0
    mx, arg = u.max(1)
    mn = u.min(1).values
    dc = mx - mn
    s = dc / (mx + 1e-8)
    dc = torch.where(dc == 0, torch.ones_like(dc), dc)
    rc, gc, bc = (mx.unsqueeze(1) - u).unbind(1)
    h = torch.stack([bc - gc, (rc - bc) + 2.0 * dc, (gc - rc) + 4.0 * dc], 1) / dc.unsqueeze(1)
    h = h.gather(1, arg.unsqueeze(1)).squeeze(1)
    h = ((h / 6.0) % 1.0) * 360.0
    hsv = torch.stack([h, s, mx * 255.0], 1)
    for i in range(n):
        if rows['flags'][i] & SAT:
            hsv[i, 1] *= float(rows['sat'][i])
        if rows['flags'][i] & HUE:
            hsv[i, 0] += float(rows['hue'][i])
    hsv[:, 0][hsv[:, 0] > 360] -= 360
    hsv[:, 0][hsv[:, 0] < 0] += 360
    hue, s, val = hsv[:, 0] / 360.0, hsv[:, 1], hsv[:, 2] / 255.0
    sext = torch.floor(hue * 6) % 6
    frac = ((hue * 6) % 6) - sext
    lo, fall, rise = val * (1 - s), val * (1 - frac * s), val * (1 - (1 - frac) * s)
    table = {'R': (val, fall, lo, lo, rise, val), 'G': (rise, val, val, fall, lo, lo), 'B': (lo, lo, rise, val, val, fall)}   # per sextant
    planes = torch.stack(table['R'] + table['G'] + table['B'], 1)          # 18 planes, as the reference materialises them
    sext = sext.long()
    x = planes.gather(1, torch.stack([sext, sext + 6, sext + 12], 1)) * 255.0
    for i in range(n):
        if rows['flags'][i] & CONTRAST and rows['mode'][i] == 1:
            x[i] *= float(rows['alpha'][i])
        if rows['flags'][i] & SWAP:
            x[i] = x[i, [int(k) for k in rows['perm'][i]]]
    x = x[:, [2, 1, 0]]
    x = x[:, [2, 1, 0]]                         # to_rgb
    x = (x - mean) / std
    H, W = x.shape[-2:]
    pad_h, pad_w = -H % 32, -W % 32
    if pad_h or pad_w:
        x = F.pad(x, [0, pad_w, 0, pad_h], value=0)
    x = x.to(out_dtype)
    if rows['mask'][0][0]:
        _, d, l, st_h, st_w = [int(k) for k in rows['mask'][0]]
        x = x * torch.tensor(grid_keep(x.shape[-2], x.shape[-1], d, l, st_h, st_w), dtype=x.dtype, device=x.device)
    return x


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_shape(a, n, out_dtype):
    from sparsebev_amd import ImageFrontEnd
    dev = 'cuda:0'
    H, W = 256, 704
    g = torch.Generator(device=dev).manual_seed(n)
    img = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=dev, generator=g)
    front = ImageFrontEnd.from_data_aug(DATA_AUG, out_dtype=out_dtype).train()
    rng = np.random.RandomState(1)
    params = front.draw(n, H, rng=rng)
    while not params.mask[0, 0]:                   # a step WITH the mask (70 % of them)
        params = front.draw(n, H, rng=rng)
    rows = params.rows
    mean = torch.tensor(DATA_AUG['img_norm_cfg']['mean'], device=dev).view(1, 3, 1, 1)
    std = torch.tensor(DATA_AUG['img_norm_cfg']['std'], device=dev).view(1, 3, 1, 1)
    out = torch.empty((n, 3, H, W), dtype=out_dtype, device=dev)
    metas = [dict()]
    front.upload(params)
    table = front._tables[(0, n)]

    def fused_launch():                             # the launch alone: the table is in place (a replayed step)
        import ctypes
        from sparsebev_amd import _lib
        _lib.check(_lib.load().sbev_image_front(ctypes.c_void_p(img.data_ptr()), 3, ctypes.c_void_p(out.data_ptr()), 0 if out_dtype == torch.float32 else 2,
                                                n, H, W, 32, front._mean_c, front._std_c, 1, 1, ctypes.c_void_p(table.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_image_front')

    plain = ImageFrontEnd.from_data_aug(DATA_AUG, out_dtype=out_dtype).eval()          # the inference call: no table

    def torch_plain():
        return ((img.float()[:, [2, 1, 0]] - mean) / std).to(out_dtype)

    assert torch.equal(plain(img[:8], metas), torch_plain()[:8])
    legs = {'fused_launch': (fused_launch, a.iters), 'fused_plain_forward': (lambda: plain(img, metas, out=out), a.iters),
            'torch_plain_chain': (torch_plain, max(1, a.iters // 4)), 'fused_forward_with_upload': (lambda: front(img, metas, params=params, out=out), a.iters),
            'torch_chain': (lambda: torch_chain(img, rows, mean, std, out_dtype), max(1, a.iters // 10))}
    ref = torch_chain(img[:8], rows[:8], mean, std, out_dtype).float()
    small = front(img[:8], metas, params=_first(params, 8)).float()
    agree = (ref - small).abs().max().item()
    for fn, _ in legs.values():                     # warm-up
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(3):
        for k, (fn, inner) in legs.items():
            rounds[k].append(statistics.median(timed(fn, inner) for _ in range(3)))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    nbytes = n * 3 * H * W * (1 + out.element_size())
    rate = nbytes / (med['fused_launch'] * 1e-3)
    plain_rate = nbytes / (med['fused_plain_forward'] * 1e-3)
    return {'images': n, 'H': H, 'W': W, 'src': 'uint8', 'dst': str(out_dtype).replace('torch.', ''),
            'median_ms': {k: round(v, 4) for k, v in med.items()}, 'rounds_ms': {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            'torch_over_fused_launch': round(med['torch_chain'] / med['fused_launch'], 1),
            'fused_bytes': nbytes, 'fused_TBps': round(rate / 1e12, 3), 'fused_fraction_of_copy_rate': round(rate / COPY_RATE, 3),
            'plain_TBps': round(plain_rate / 1e12, 3), 'plain_fraction_of_copy_rate': round(plain_rate / COPY_RATE, 3),
            'torch_plain_over_fused_plain': round(med['torch_plain_chain'] / med['fused_plain_forward'], 1),
            'max_abs_difference_torch_chain_vs_fused_first_8_images': agree}


def _first(params, k):
    from sparsebev_amd.image_front import FrontParams
    p = FrontParams(k)
    p.rows[:] = params.rows[:k]
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_front.json'))
    ap.add_argument('--resources-only', action='store_true')
    a = ap.parse_args()
    res = kernel_resources()
    scratch = {k: v.get('scratch_bytes_per_lane') for k, v in res.items()}
    rec = {'tool': 'bench_image_front', 'kernel_resources': res, 'scratch_free': all(v == 0 for v in scratch.values()),
           'copy_rate_TBps': COPY_RATE / 1e12, 'copy_rate_source': 'profiles/optim_step.json (update launch)'}
    if a.resources_only or not torch.cuda.is_available():
        rec.update(device=None, shapes='NOT measured (no GPU run)')
    else:
        prop = torch.cuda.get_device_properties(0)
        rec.update(device=torch.cuda.get_device_name(0), compute_units=prop.multi_processor_count,
                   clock_rate_khz=getattr(prop, 'clock_rate', None), hip=torch.version.hip, torch=torch.__version__, iters=a.iters, rounds=3,
                   timing='HIP events, legs interleaved in one process, median of the rounds\' medians',
                   shapes=[bench_shape(a, n, dt) for n in (48, 384) for dt in (torch.float32, torch.float16)])
    line = json.dumps(rec)
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
