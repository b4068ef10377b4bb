"""Dev tool: time sparsebev_amd.ImageGeometry's launch (csrc/image_geom.hip: Pillow-exact resize + crop + mirror + HWC -> CHW for all
images at once) and write one JSON line to profiles/image_geom.json.

The launch: 6 and 48 frames of 900 x 1600 x 3 uint8 to 3 x 256 x 704, at three transforms of the r50 recipe: the eval transform
(factor 0.44), factor 0.38 mirrored (the recipe's smallest: 13 taps, 96 black columns) and factor 0.55 (its largest).  The table is in
place (a replayed step), so the figure is the kernel.  Two figures per shape: ``rotating`` walks over enough distinct input buffers
(> 512 MB in all) that no launch finds its frames in the 256 MiB last-level cache -- the streaming case, frames arrive fresh -- and
``same_buffer`` re-reads one input.  Bytes are counted from the tables: read = the source rows x columns any tap of the crop touches
(out[4] of sbev_image_geom_plan), written = 3 fH fW; the rate is given as a fraction of the float4 copy rate recorded in
profiles/optim_step.json.

Context, not a gate: torch.nn.functional.interpolate(mode='bicubic', antialias=True) plus crop on the same device (fp32, not bit-equal
to Pillow); Pillow on this host for one frame, if it imports; the pinned host-to-device copy of six raw frames (26 MB) beside the copy
of six pre-resized ones (3.2 MB).  Legs are interleaved in one process, warmed up, timed with HIP events; a figure is the median of
three rounds' medians.  The record carries the compiler's register / scratch / LDS figures.

    python tools/bench_image_geom.py [--iters 50] [--out profiles/image_geom.json]
    python tools/bench_image_geom.py --resources-only          (no GPU needed: times are written as "NOT measured")
    python tools/bench_image_geom.py --launch-only             (five launches of 48 frames at the eval transform and nothing else: the
                                                                program to put beneath ``rocprofv3 --pmc ... --``, counters in a run of their own)
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
import torch.nn.functional as F               # noqa: E402

COPY_RATE = 6.23e12          # bytes / s: profiles/optim_step.json, the update launch
CONF = dict(H=900, W=1600, final_dim=(256, 704), resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True)
# name -> (resize, resize_dims, crop, flip)
TRANSFORMS = {'eval_0.44': (0.44, (704, 396), (0, 140, 704, 396), False),
              'factor_0.38_mirrored': (0.38, (608, 342), (0, 86, 704, 342), True),
              'factor_0.55': (0.55, (880, 495), (88, 239, 792, 495), False)}


def kernel_resources():
    from sparsebev_amd.csrc import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.COMMON + build.UNITS['image_geom.hip'] + ['-Rpass-analysis=kernel-resource-usage', '-c',
                                                                                 os.path.join(build.HERE, 'image_geom.hip'), '-o', os.path.join(tmp, 'unit.o')]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, cur = {}, None
    keys = {'VGPRs': 'vgprs', 'TotalSGPRs': 'sgprs', 'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'LDS Size [bytes/block]': 'lds_bytes_per_block',
            'Occupancy [waves/SIMD]': 'occupancy_waves_per_simd'}
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], stdout=subprocess.PIPE).stdout.decode().strip() or m.group(1)
            cur = out.setdefault('image_geom_kernel' if 'image_geom_kernel' in name else name, {})
            continue
        for k, v in keys.items():
            m = re.search(r'remark:\s+' + re.escape(k) + r': (\d+)', line)
            if m and cur is not None:
                cur[v] = int(m.group(1))
    return out


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(legs):
    """legs: name -> (fn, inner).  Warm-up, then three rounds of interleaved medians of three."""
    for fn, _ in legs.values():
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(3):
        for k, (fn, inner) in legs.items():
            rounds[k].append(statistics.median(timed(fn, inner) for _ in range(3)))
    return {k: statistics.median(v) for k, v in rounds.items()}, rounds


def bench_shape(a, n, name, bufs):
    from sparsebev_amd import _lib
    from sparsebev_amd.image_geom import GeomParams, ImageGeometry, plan
    dev = 'cuda:0'
    H, W, (fH, fW) = CONF['H'], CONF['W'], CONF['final_dim']
    resize, dims, crop, flip = TRANSFORMS[name]
    geom = ImageGeometry(CONF)
    p = GeomParams(resize, dims, crop, flip)
    pl = plan(H, W, fH, fW, dims, crop[:2], flip, table=True)[0]
    out = torch.empty((n, 3, fH, fW), dtype=torch.uint8, device=dev)
    table = geom.upload([p], dev, n=n)
    rows_bytes = (n + 3) // 4 * 16
    lib = _lib.load()
    turn = [0]

    def launch(src):
        _lib.check(lib.sbev_image_geom(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, H, W, fH, fW,
                                       ctypes.c_void_p(table.data_ptr() + rows_bytes), ctypes.c_void_p(table.data_ptr()), 1,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_image_geom')

    def rotating():
        turn[0] = (turn[0] + 1) % len(bufs)
        launch(bufs[turn[0]][:n])

    def torch_leg():
        x = bufs[0][:n].permute(0, 3, 1, 2).float()
        y = F.interpolate(x, size=(dims[1], dims[0]), mode='bicubic', antialias=True, align_corners=False)
        y = y[:, :, max(crop[1], 0):crop[3], max(crop[0], 0):min(crop[2], dims[0])]
        if flip:
            y = y.flip(-1)
        return y.round().clamp(0, 255).to(torch.uint8)

    # the launch equals forward() (checked bit for bit against Pillow's arithmetic by the tests); torch's leg is close, not equal
    want = geom(bufs[0][:n], [dict()], params=[p])
    launch(bufs[0][:n])
    assert torch.equal(out, want)
    t = torch_leg()
    x0 = fW - t.shape[-1] if flip else 0
    torch_diff = (out[:, :, :, x0:x0 + t.shape[-1]].int() - t.int()).abs()
    med, rounds = measure({'rotating': (rotating, a.iters), 'same_buffer': (lambda: launch(bufs[0][:n]), a.iters),
                           'torch_interpolate_crop': (torch_leg, max(2, a.iters // 10))})
    read, written = n * pl.src_bytes, n * 3 * fH * fW
    rate = (read + written) / (med['rotating'] * 1e-3)
    return {'images': n, 'transform': name, 'resize_dims': dims, 'crop': crop, 'flip': flip, 'ksize': [pl.ksize_x, pl.ksize_y],
            'workgroups': n * pl.workgroups, 'input_buffers_rotated': len(bufs),
            'median_ms': {k: round(v, 4) for k, v in med.items()}, 'rounds_ms': {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            'bytes_read_per_image': pl.src_bytes, 'bytes_written_per_image': 3 * fH * fW, 'source_rows_read': pl.src_rows,
            'rotating_TBps': round(rate / 1e12, 3), 'rotating_fraction_of_copy_rate': round(rate / COPY_RATE, 3),
            'same_buffer_TBps': round((read + written) / (med['same_buffer'] * 1e-3) / 1e12, 3),
            'torch_over_launch': round(med['torch_interpolate_crop'] / med['rotating'], 1),
            'torch_interpolate_max_abs_difference': int(torch_diff.max()), 'torch_interpolate_bytes_differing': round(float((torch_diff != 0).float().mean()), 4)}


def bench_copies(a):
    """pinned host -> device: six raw frames beside six pre-resized ones"""
    dev = 'cuda:0'
    raw = torch.empty((6, 900, 1600, 3), dtype=torch.uint8).pin_memory()
    small = torch.empty((6, 3, 256, 704), dtype=torch.uint8).pin_memory()
    d_raw, d_small = torch.empty_like(raw, device=dev), torch.empty_like(small, device=dev)
    med, rounds = measure({'h2d_six_raw_frames': (lambda: d_raw.copy_(raw, non_blocking=True), a.iters),
                           'h2d_six_resized_frames': (lambda: d_small.copy_(small, non_blocking=True), a.iters)})
    return {'bytes': {'h2d_six_raw_frames': raw.numel(), 'h2d_six_resized_frames': small.numel()},
            'median_ms': {k: round(v, 4) for k, v in med.items()}, 'rounds_ms': {k: [round(x, 4) for x in v] for k, v in rounds.items()}}


def bench_pillow():
    try:
        from PIL import Image
    except ImportError:
        return 'NOT measured (Pillow does not import on this host)'
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, size=(900, 1600, 3)).astype(np.uint8))
    out = {}
    for name, (_, dims, crop, flip) in TRANSFORMS.items():
        times = []
        for _ in range(7):
            t0 = time.perf_counter()
            im = img.resize(dims).crop(crop)
            if flip:
                im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
            np.array(im)
            times.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(statistics.median(times), 3)
    return {'one_frame_one_core_median_ms': out, 'note': 'host CPU of the GPU machine, shared with other work'}


def launch_only():
    from sparsebev_amd.image_geom import GeomParams, ImageGeometry
    geom = ImageGeometry(CONF)
    resize, dims, crop, flip = TRANSFORMS['eval_0.44']
    img = torch.randint(0, 256, (48, 900, 1600, 3), dtype=torch.uint8, device='cuda:0')
    for _ in range(5):
        geom(img, [dict()], params=[GeomParams(resize, dims, crop, flip)])
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_geom.json'))
    ap.add_argument('--resources-only', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    a = ap.parse_args()
    if a.launch_only:
        return launch_only()
    res = kernel_resources()
    rec = {'tool': 'bench_image_geom', 'kernel_resources': res, 'instantiations': len(res),
           'scratch_free': all(v.get('scratch_bytes_per_lane') == 0 for v in res.values()),
           'copy_rate_TBps': COPY_RATE / 1e12, 'copy_rate_source': 'profiles/optim_step.json (update launch)'}
    if a.resources_only or not torch.cuda.is_available():
        rec.update(device=None, shapes='NOT measured (no GPU run)', copies='NOT measured (no GPU run)', pillow='NOT measured (no GPU run)')
    else:
        prop = torch.cuda.get_device_properties(0)
        g = torch.Generator(device='cuda:0').manual_seed(1)
        shapes = []
        for n, count in ((6, 21), (48, 3)):                # 21 x 26 MB and 3 x 207 MB: more than 512 MB walked between two uses
            bufs = [torch.randint(0, 256, (n, 900, 1600, 3), dtype=torch.uint8, device='cuda:0', generator=g) for _ in range(count)]
            shapes += [bench_shape(a, n, name, bufs) for name in TRANSFORMS]
            del bufs
        rec.update(device=torch.cuda.get_device_name(0), compute_units=prop.multi_processor_count,
                   clock_rate_khz=getattr(prop, 'clock_rate', None), hip=torch.version.hip, torch=torch.__version__, iters=a.iters, rounds=3,
                   timing='HIP events, legs interleaved in one process, median of the rounds\' medians',
                   shapes=shapes, copies=bench_copies(a), pillow=bench_pillow())
    line = json.dumps(rec)
    print(line)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
