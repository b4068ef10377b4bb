"""Streaming decoder step through the keyed frame pool beside the same step through the positional ring (config c2: B = 1, T = 8).

Both caches hold the same frames and take ONE new frame (6 NCHW images) per step, as ``bench.py --online`` does; the ring has
n_slots = T = 8 (one captured graph per ring phase), the pool n_slots = 16 (one captured graph, the step's slot table uploaded into
the pool's persistent device table).  A third leg feeds a pool of its own through ``FramePool.step``: the new frame goes into its slot
inside the captured step (sbev_pool_insert_frames, K = 1) instead of through ``put``'s eager launches in front of it.  Two more legs take
the frame as a channels_last fp16 backbone hands it over -- channels-last fp16 memory for fp32 slots: through ``FramePool.stream`` (the same
in-graph launch, widening on the way) and, beside it, through ``FramePool.step``, which stores such frames by eager launches in
front of the replay (B x L of them).  The legs run interleaved on one
GPU, round by round, with the warm-up and timing discipline of bench.py: warm-up steps first (captures included), device synchronised,
wall clock over ``--steps`` steps, device synchronised.  Prints one JSON line.  Usage: python tools/bench_pool.py [--steps 50] [--warmup 40] [--rounds 3] [--config c2]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {'c2': ('r50_704x256', 900, 8), 'small': ('tiny', 64, 4)}      # pyramid, queries, frames (B = 1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', choices=sorted(CONFIGS), default='c2')
    ap.add_argument('--steps', type=int, default=50, help='timed steps per round and cache')
    ap.add_argument('--warmup', type=int, default=40, help='untimed steps per cache before the first round (the ring captures one graph per phase from its second lap on)')
    ap.add_argument('--rounds', type=int, default=3, help='interleaved rounds: ring, pool, pool fed through step(), the two channels-last fp16 legs, ring, ...')
    ap.add_argument('--ring-slots', type=int, default=None, help='ring n_slots (default: T)')
    ap.add_argument('--pool-slots', type=int, default=16)
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0 or args.rounds < 1:
        ap.error('--steps and --rounds must be at least 1, --warmup at least 0')
    if not 1 <= args.pool_slots <= 16:
        ap.error('--pool-slots must be in 1 .. 16')
    return args


def summarise(ring_ms, pool_ms, pool_step_ms=None, pool_stream_ms=None, pool_eager_ms=None):
    """the JSON line's figures from the per-round step times (ms); ``pool_step_ms``: the leg fed through FramePool.step, compared with
    the ``put`` leg of the same run; ``pool_stream_ms`` / ``pool_eager_ms``: channels-last fp16 frames for fp32 slots through
    FramePool.stream and through the eager store, compared with each other and with the ``put`` leg"""
    med = lambda v: sorted(v)[len(v) // 2]
    r, p = med(ring_ms), med(pool_ms)
    out = {'ring_ms_per_step': [round(v, 4) for v in ring_ms], 'pool_ms_per_step': [round(v, 4) for v in pool_ms],
           'ring_median_ms': round(r, 4), 'pool_median_ms': round(p, 4), 'pool_over_ring': round(p / r, 4)}
    if pool_step_ms is not None:
        s = med(pool_step_ms)
        out.update({'pool_step_ms_per_step': [round(v, 4) for v in pool_step_ms], 'pool_step_median_ms': round(s, 4),
                    'pool_step_over_pool': round(s / p, 4)})
    if pool_stream_ms is not None and pool_eager_ms is not None:
        f, e = med(pool_stream_ms), med(pool_eager_ms)
        out.update({'pool_stream_ms_per_step': [round(v, 4) for v in pool_stream_ms], 'pool_stream_median_ms': round(f, 4),
                    'pool_eager_ms_per_step': [round(v, 4) for v in pool_eager_ms], 'pool_eager_median_ms': round(e, 4),
                    'pool_stream_over_eager': round(f / e, 4), 'pool_stream_over_pool': round(f / p, 4)})
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    from sparsebev_amd import runtime, synthetic as S
    from sparsebev_amd.cache import FrameFeatureCache, FramePool
    from sparsebev_amd.transformer import SparseBEVTransformer

    pyr, Q, T = CONFIGS[args.config]
    B, dev = 1, torch.device('cuda:0')
    ih, iw, sizes = S.PYRAMIDS[pyr]
    L = len(sizes)
    params = S.make_params(0, embed_dims=256, num_frames=T, num_points=4, num_levels=L)

    def model():
        m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=6, num_levels=L, num_classes=10, code_size=10, pc_range=S.PC_RANGE)
        m.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in params.items()})
        return m.to(dev).eval()

    feats = S.make_features(B, T, sizes, seed=0, device=dev)
    per_frame = [[f[:, t * 6:(t + 1) * 6].contiguous() for f in feats] for t in range(T)]
    bbox, qfeat = [t.to(dev) for t in S.make_queries(B, Q, seed=0)]
    metas = S.make_img_metas(B, T, ih, iw)

    # the same frames as a channels_last fp16 backbone emits them: [B, 6, C, H, W] views of channels-last fp16 memory
    per_frame_cl = [[f.half().permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in fr] for fr in per_frame]

    m_ring, m_pool, m_step, m_stream, m_eager = [model() for _ in range(5)]          # one runtime (and graph cache) each
    ring = FrameFeatureCache(T, n_slots=args.ring_slots or T)
    pool, pool_s, pool_f, pool_e = [FramePool(T, n_slots=args.pool_slots) for _ in range(4)]
    for fr in reversed(per_frame):
        ring.push(fr)
    tick = {'ring': 0, 'pool': T - 1, 'step': T - 1, 'stream': T - 1, 'eager': T - 1}
    keys0 = [list(range(T - 1, -1, -1))]       # frame number = key; t = 0 newest
    pool_f.stream(keys0, {t: per_frame_cl[t] for t in range(T)}).materialise()      # the scene's first window: T frames in one launch
    for b, k in pool_e.missing(keys0):
        pool_e.put(b, k, [f[0] for f in per_frame_cl[T - 1 - k]])
    for p in (pool, pool_s):
        for b, k in p.missing(keys0):
            p.put(b, k, [f[0] for f in per_frame[T - 1 - k]])

    def ring_step():
        ring.push(per_frame[tick['ring'] % T])
        tick['ring'] += 1
        return m_ring(bbox, qfeat, ring.pyramid(), None, metas)

    def pool_step():
        tick['pool'] += 1
        n = tick['pool']
        keys = [[n - t for t in range(T)]]
        for b, k in pool.missing(keys):        # one miss per step: the new frame
            pool.put(b, k, [f[0] for f in per_frame[(n - T) % T]])
        return m_pool(bbox, qfeat, pool.pyramid(keys), None, metas)

    def pool_step_step():
        tick['step'] += 1
        n = tick['step']
        keys = [[n - t for t in range(T)]]
        return m_step(bbox, qfeat, pool_s.step(keys, per_frame[(n - T) % T]), None, metas)      # the new frame goes in inside the step

    def pool_stream_step():
        tick['stream'] += 1
        n = tick['stream']
        keys = [[n - t for t in range(T)]]
        return m_stream(bbox, qfeat, pool_f.stream(keys, {0: per_frame_cl[(n - T) % T]}), None, metas)      # channels-last fp16, widened inside the step

    def pool_eager_step():
        tick['eager'] += 1
        n = tick['eager']
        keys = [[n - t for t in range(T)]]
        return m_eager(bbox, qfeat, pool_e.step(keys, per_frame_cl[(n - T) % T]), None, metas)      # the same frames: stored by eager launches in front of the replay

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    for _ in range(args.warmup):
        ring_step()
        pool_step()
        pool_step_step()
        pool_stream_step()
        pool_eager_step()
    ring_ms, pool_ms, step_ms, stream_ms, eager_ms = [], [], [], [], []
    for _ in range(args.rounds):
        ring_ms.append(timed(ring_step))
        pool_ms.append(timed(pool_step))
        step_ms.append(timed(pool_step_step))
        stream_ms.append(timed(pool_stream_step))
        eager_ms.append(timed(pool_eager_step))
    runtime.check_pair_faults()
    g = {name: {'captures': m.decoder._runtime.step_graphs.captures, 'replays': m.decoder._runtime.step_graphs.replays}
         for name, m in (('ring', m_ring), ('pool', m_pool), ('pool_step', m_step), ('pool_stream', m_stream), ('pool_eager', m_eager))}
    out = {'metric': 'streaming decoder step, frame pool vs frame ring', 'config': args.config, 'B': B, 'Q': Q, 'T': T, 'pyramid': pyr,
           'ring_slots': ring.n_slots, 'pool_slots': pool.n_slots, 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds,
           'graphs': g, 'device': torch.cuda.get_device_name(0)}
    out.update(summarise(ring_ms, pool_ms, step_ms, stream_ms, eager_ms))
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
