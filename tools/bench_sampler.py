"""Micro-benchmark of the sampling kernel alone at a BASELINE config (default c2): algorithmic GB/s
(SURVEY.md section 8d byte model) from HIP-event timing on the launch stream.  Dev tool; bench.py is the
contract."""
import argparse
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsebev_amd import ops, synthetic as S   # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))


def sampler_inputs(pyramid, B, Q, T, P, seed=0):
    """tests/test_gpu_sampling.py::c2_inputs for any pyramid and point count: random fp32 features [B', 6, H, W, 64], sample locations
    projected from seeded queries through the synthetic camera rig (clustered like a real step's), level weights."""
    import numpy as np
    dev = 'cuda:0'
    ih, iw, sizes = S.PYRAMIDS[pyramid]
    G, L = 4, len(sizes)
    g = torch.Generator(device=dev).manual_seed(seed)
    feats = [torch.randn(B * T * G, 6, h, w, 64, generator=g, device=dev) for h, w in sizes]
    bbox, feat = S.make_queries(B, Q, seed=seed)
    params = S.make_params(seed, num_frames=T, num_points=P, num_levels=L)
    metas = S.make_img_metas(B, T, ih, iw)
    l2i = torch.from_numpy(np.asarray([m['lidar2img'] for m in metas]).astype(np.float32))
    td = torch.tensor([[0.5 * t for t in range(T)]] * B)
    off = torch.nn.functional.linear(feat, params['sampling.sampling_offset.weight'], params['sampling.sampling_offset.bias'])
    lg = torch.nn.functional.linear(feat, params['sampling.scale_weights.weight'], params['sampling.scale_weights.bias'])
    pts, wbp = ops.sampling_front(bbox.to(dev), off.to(dev), lg.to(dev), td.to(dev), S.PC_RANGE, T, G, P, L)
    loc = ops.project_select(pts, l2i.to(dev), ih, iw, G, P)
    return feats, loc, wbp, G


def bench_deterministic(a):
    """Medians over --iters of: the atomic kernel (sbev_msmv_bwd_ex with feature buffers); the same kernel without them (grad_loc /
    grad_weights only: the first launch of the deterministic path); sbev_msmv_bwd_taps; torch.sort(stable); sbev_msmv_bwd_sum_sorted; and
    the four deterministic launches as one bracket.  Every iteration runs all of them, in this order, on one stream."""
    import ctypes
    import json
    from sparsebev_amd import _lib
    lib = _lib.load()
    feats, loc, wbp, G = sampler_inputs(a.pyramid, a.B, a.Q, a.T, a.P)
    if a.uniform:
        loc = torch.rand_like(loc)
        loc[..., 2] = torch.randint(0, 6, loc.shape[:-1], device=loc.device).float() / 5
    Bp, N, _, _, C = feats[0].shape
    _, Q, P, _ = loc.shape
    mix = a.layout == 'mix'
    layout = ops.OUT_MIX if mix else ops.OUT_REF
    gout = torch.randn(a.B, Q, G, a.T * P, C, device=loc.device) if mix else torch.randn(Bp, Q, C, P, device=loc.device)
    gfeats = [torch.zeros_like(f) for f in feats]
    gloc, gw = torch.empty_like(loc), torch.empty_like(wbp)
    (c_feats, c_hw, L), strides = ops._pyramid(feats, N)
    c_gfeats = ops._level_ptrs(gfeats)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = lib.sbev_msmv_bwd_tap_count(Bp, Q, P, L)
    keys = torch.empty(n, device=loc.device, dtype=torch.int64)
    coefs = torch.empty(n, device=loc.device)
    state = {}

    def bwd(gf):
        _lib.check(lib.sbev_msmv_bwd_ex(c_feats, gf, c_hw, L, Bp, N, C, Q, P, *strides, p(loc), p(wbp), p(gout), layout, a.T, G, p(gloc), p(gw), st), 'bwd')

    def taps():
        _lib.check(lib.sbev_msmv_bwd_taps(c_feats, c_hw, L, Bp, N, C, Q, P, *strides, p(loc), p(wbp), p(keys), p(coefs), st), 'taps')

    def sort():
        state['sk'], state['order'] = torch.sort(keys, stable=True)

    def total():
        _lib.check(lib.sbev_msmv_bwd_sum_sorted(c_gfeats, L, p(state['sk']), p(state['order']), p(coefs), n, p(gout), layout, Bp, C, Q, P, a.T, G, st), 'sum')

    stages = [('atomic', lambda: bwd(c_gfeats)), ('loc_w_only', lambda: bwd(None)), ('taps', taps), ('sort', sort), ('sum', total)]
    for _ in range(3):
        for _, fn in stages:
            fn()
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = [[ev() for _ in range(len(stages) + 1)] for _ in range(a.iters)]
    for row in marks:
        row[0].record()
        for i, (_, fn) in enumerate(stages):
            fn()
            row[i + 1].record()
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2] * 1e3          # us
    res = {name: round(med([row[i].elapsed_time(row[i + 1]) for row in marks]), 1) for i, (name, _) in enumerate(stages)}
    res['deterministic_total'] = round(med([row[1].elapsed_time(row[-1]) for row in marks]), 1)
    live = int((keys != torch.iinfo(torch.int64).max).sum())
    out = dict(tool='bench_sampler --bwd --deterministic', pyramid=a.pyramid, B=a.B, Q=Q, T=a.T, P=P, L=L, C=C, layout=a.layout,
               uniform=bool(a.uniform), iters=a.iters, taps=n, live_taps=live, destinations=int(torch.unique(state['sk']).numel()) - (live < n),
               median_us=res, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pyramid', default='r50_704x256')
    ap.add_argument('--B', type=int, default=1)
    ap.add_argument('--Q', type=int, default=900)
    ap.add_argument('--T', type=int, default=8)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('--layout', default='ref', choices=['ref', 'mix'])
    ap.add_argument('--uniform', action='store_true', help='replace the projected sample locations by uniform random ones (no clustering)')
    ap.add_argument('--bwd', action='store_true', help='time sbev_msmv_bwd (the backward kernel alone, grad buffers pre-zeroed once)')
    ap.add_argument('--deterministic', action='store_true',
                    help='with --bwd: the atomics-free feature gradient (taps / sort / sum, separately and together) interleaved with the '
                         'atomic kernel in the same process; --layout is grad_out\'s; any --pyramid, --P')
    ap.add_argument('--P', type=int, default=4, help='sample points per (query, frame, group); --deterministic only')
    ap.add_argument('--out', default=None, help='--deterministic: append the JSON result line to this file')
    a = ap.parse_args()
    if a.deterministic:
        if not a.bwd:
            ap.error('--deterministic needs --bwd')
        return bench_deterministic(a)
    from test_gpu_sampling import c2_inputs
    import test_gpu_sampling as tg
    ih, iw, sizes = S.PYRAMIDS[a.pyramid]
    feats, pts, l2i, loc, wbp, _, (ih, iw, B, Q, T, G, P, L) = c2_inputs(a.B, a.Q, a.T) if a.pyramid == 'r50_704x256' else (None,) * 7
    if a.bf16:
        feats = [f.to(torch.bfloat16) for f in feats]
    if a.uniform:
        loc = torch.rand_like(loc)
        loc[..., 2] = torch.randint(0, 6, loc.shape[:-1], device=loc.device).float() / 5
    layout = ops.OUT_REF if a.layout == 'ref' else ops.OUT_MIX
    if a.bwd:
        import ctypes
        from sparsebev_amd import _lib
        lib = _lib.load()
        Bp, N, _, _, C = feats[0].shape
        _, Qn, Pn, _ = loc.shape
        gout = torch.randn(Bp, Qn, C, Pn, device=loc.device)
        gfeats = [torch.zeros_like(f) for f in feats]
        gloc, gw = torch.empty_like(loc), torch.empty_like(wbp)
        (c_feats, c_hw, Ln), strides = ops._pyramid(feats, N)
        c_gfeats = ops._level_ptrs(gfeats)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = lambda: lib.sbev_msmv_bwd(c_feats, c_gfeats, c_hw, Ln, Bp, N, C, Qn, Pn, *strides, p(loc), p(wbp), p(gout), p(gloc), p(gw), st)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for s_, e_ in evs:
            s_.record(); fn(); e_.record()
        torch.cuda.synchronize()
        ts = sorted(s_.elapsed_time(e_) for s_, e_ in evs)
        npts = loc.shape[0] * loc.shape[1] * loc.shape[2]
        # per point: L taps x 4 corners x C floats read AND atomically added, C grad_out floats, coords / weights in, their grads out
        bytes_ = npts * (Ln * 4 * C * 4 * 2 + C * 4 + 12 + 4 * Ln + 12 + 4 * Ln)
        print('BWD points %d  bytes %.1f MB  median %.1f us  min %.1f us  -> %.0f GB/s algorithmic; %.2f G atomic dwords/s'
              % (npts, bytes_ / 1e6, ts[len(ts) // 2] * 1e3, ts[0] * 1e3, bytes_ / ts[len(ts) // 2] / 1e6, npts * Ln * 4 * C / ts[len(ts) // 2] / 1e6))
        return
    for _ in range(5):
        ops.msmv_sampling(feats, loc, wbp, out_layout=layout, T=T, G=G)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for s, e in evs:
        s.record()
        ops.msmv_sampling(feats, loc, wbp, out_layout=layout, T=T, G=G)
        e.record()
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    npts = loc.shape[0] * loc.shape[1] * loc.shape[2]
    sf = 2 if a.bf16 else 4
    bytes_ = npts * (L * 4 * 64 * sf + 12 + 4 * L + 64 * 4)
    med = ts[len(ts) // 2]
    print('points %d  bytes %.1f MB  median %.1f us  min %.1f us  -> %.0f GB/s algorithmic (%.1f%% of 8 TB/s)'
          % (npts, bytes_ / 1e6, med * 1e3, ts[0] * 1e3, bytes_ / med / 1e6, bytes_ / med / 1e6 / 80))


if __name__ == '__main__':
    main()
