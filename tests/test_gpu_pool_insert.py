"""The frame pool's insert inside the step: sbev_pool_insert against torch, and FramePool.step against FramePool.put.  Every comparison
is bitwise -- the insert is byte movement, and the decoder afterwards runs the same kernels on the same slot contents -- so no tolerance
appears anywhere.  Shapes are the tiny pyramid's: vector planes (8 x 22, 4 x 11, 2 x 6) and a scalar one (1 x 3) in one launch, a partial
pixel tile (176 = 2 * 64 + 48), several blocks per level."""
import copy
import ctypes

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

from sparsebev_amd import cache, synthetic as S  # noqa: E402
from sparsebev_amd.cache import FramePool  # noqa: E402
from sparsebev_amd.transformer import SparseBEVTransformer  # noqa: E402

DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
N = 6
SIZES = S.PYRAMIDS['tiny'][2]
# bit patterns no input holds: NaNs with a payload (randn and its roundings to fp16 / bf16 are finite)
PATTERN = {torch.float32: (torch.int32, 0x7fc12345), torch.float16: (torch.int16, 0x7e01), torch.bfloat16: (torch.int16, 0x7fc1)}


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the kernel against torch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('indirect', [False, True])
@pytest.mark.parametrize('dtype,C', [(torch.float32, 256), (torch.float16, 256), (torch.bfloat16, 256), (torch.bfloat16, 64),
                                     (torch.float32, 7), (torch.bfloat16, 12)])          # (the last two: the scalar channel forms)
def test_pool_insert_kernel_equals_torch(dtype, C, indirect):
    B, n_slots = 3, 4
    assert list(SIZES) == [(8, 22), (4, 11), (2, 6), (1, 3)]
    g = torch.Generator(device=DEV).manual_seed(5 + C)
    frames = [torch.randn(B, N, C, h, w, generator=g, device=DEV).to(dtype) for h, w in SIZES]
    ity, pat = PATTERN[dtype]
    bufs = [torch.empty(B, n_slots, N, h, w, C, device=DEV, dtype=dtype) for h, w in SIZES]

    def run(insert):
        for buf in bufs:
            buf.view(ity).fill_(pat)
        row = torch.tensor(insert, device=DEV, dtype=torch.int32)
        if indirect:
            table = torch.tensor([0, 0, 0] + [f.data_ptr() for f in frames], device=DEV, dtype=torch.int64)
            cache.pool_insert(frames, bufs, row, n_slots, stream(), table=ctypes.c_void_p(table.data_ptr()), index=list(range(3, 3 + len(frames))))
        else:
            cache.pool_insert(frames, bufs, row, n_slots, stream())
        torch.cuda.synchronize()

    run([2, -1, 0])
    for f, buf in zip(frames, bufs):
        assert not (f.view(ity) == pat).any()
        want = torch.full_like(buf.view(ity), pat)
        want[0, 2] = f[0].permute(0, 2, 3, 1).contiguous().view(ity)
        want[2, 0] = f[2].permute(0, 2, 3, 1).contiguous().view(ity)
        assert torch.equal(buf[0, 2], f[0].permute(0, 2, 3, 1)) and torch.equal(buf[2, 0], f[2].permute(0, 2, 3, 1))
        assert torch.equal(buf.view(ity), want)                                # ... and every other element of the buffer is untouched
    # the frames entry with K = 1, NCHW, the same type is the same call: the same bytes in every level, untouched ones included
    twins = [torch.empty_like(buf) for buf in bufs]
    for twin in twins:
        twin.view(ity).fill_(pat)
    row = torch.tensor([2, -1, 0], device=DEV, dtype=torch.int32)
    cache.pool_insert_frames(frames, twins, row.view(1, B), n_slots, stream())
    torch.cuda.synchronize()
    for buf, twin in zip(bufs, twins):
        assert torch.equal(buf.view(ity), twin.view(ity))
    run([n_slots, -5, -1])                                                     # outside [0, n_slots): nothing is written, nothing is clamped
    for buf in bufs:
        assert bool((buf.view(ity) == pat).all())
    run([3, 3, 3])                                                             # every sample, the last slot: the far end of every buffer
    for f, buf in zip(frames, bufs):
        assert torch.equal(buf[:, 3], f.permute(0, 1, 3, 4, 2)) and bool((buf[:, :3].view(ity) == pat).all())


# ---- the decoder step ----------------------------------------------------------------------------------------------------------------

def build(T, L, seed, num_layers=2, graph=False):
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=L)
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=num_layers, num_levels=L, num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = graph
    return m


class Frames:
    """key -> one sample's frame (list over levels of [6, C, H, W] NCHW), generated once and kept"""

    def __init__(self, seed, dtype=torch.float32, C=256):
        self.g, self.dtype, self.C, self.frames = torch.Generator(device=DEV).manual_seed(seed), dtype, C, {}

    def __getitem__(self, key):
        if key not in self.frames:
            self.frames[key] = [torch.randn(N, self.C, h, w, generator=self.g, device=DEV).to(self.dtype) for h, w in SIZES]
        return self.frames[key]

    def newest(self, keys, channels_last=False):
        """what a backbone hands over for the batch's newest images: list over levels of NEW [B, 6, C, H, W] tensors"""
        out = [torch.stack([self[row[0]][l] for row in keys], 0) for l in range(len(SIZES))]
        return [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in out] if channels_last else out


def put_feed(pool, frames, keys):
    for b, k in pool.missing(keys):
        pool.put(b, k, frames[k])
    return pool.pyramid(keys)


def windows(i, T, change=5, repeat=8):
    """keys of step i for two samples: sample 1 changes scene at step ``change`` (its window padded by duplicates), step ``repeat`` repeats
    the step before it"""
    n = i if i < repeat else i - 1
    first1, scene1 = (change, 1) if n >= change else (0, 0)
    return [[('a', 0, max(n - t, 0)) for t in range(T)], [('b', scene1, max(n - t, first1)) for t in range(T)]]


def run_streams(steps, graph, layerwise=False, change=5, repeat=8, dtype=torch.float32, channels_last=False):
    """the same stream through put() and through step(), two models of equal weights and two pools; asserts equal outputs step by step and
    returns (put model, step model, step pool, frame tensor addresses seen)"""
    B, Q, T, n_slots = 2, 49, 4, 6
    ih, iw, _ = S.PYRAMIDS['tiny']
    m_put, m_step = build(T, len(SIZES), 21, graph=graph), build(T, len(SIZES), 21, graph=graph)
    frames = Frames(210, dtype)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=22)]
    metas = S.make_img_metas(B, T, ih, iw)
    p_put, p_step = FramePool(T, n_slots=n_slots, dtype=dtype), FramePool(T, n_slots=n_slots, dtype=dtype)
    kw = dict(layerwise=True) if layerwise else {}
    seen, alive, ptr = set(), [], None
    for i in range(steps):
        keys = windows(i, T, change, repeat)
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas, **kw)
        new = frames.newest(keys, channels_last)                       # allocated for this step and kept: no address comes back
        alive.append(new)
        seen.add(new[0].data_ptr())
        pyr = p_step.step(keys, new)
        ptr = ptr or pyr.slot_table.data_ptr()
        assert pyr.slot_table.data_ptr() == ptr == p_step.slot_table.data_ptr() and tuple(pyr.slot_table.shape) == (B, T) and pyr.slot_table.is_contiguous()
        assert p_step.insert_row.data_ptr() == ptr + 4 * B * T           # behind the table, in the same allocation
        assert (pyr.insert is None) == channels_last
        if i == repeat:
            assert p_step.insert_row.tolist() == [-1] * B              # nothing new: the step's launch is a no-op
        got = m_step(bbox, feat, pyr, None, metas, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
        assert torch.equal(p_step.slot_table, p_put.slot_table) and got[0].abs().max() > 0
    assert len(seen) == steps
    return m_put, m_step, p_step


def test_stream_through_step_equals_put_one_graph():
    from sparsebev_amd.runtime import CapturedStep
    steps = 12
    m_put, m_step, pool = run_streams(steps, graph=True)
    sg, sp = m_step.decoder._runtime.step_graphs, m_put.decoder._runtime.step_graphs
    graphs = [v for v in sg.entries.values() if isinstance(v, CapturedStep)]
    put_graphs = [v for v in sp.entries.values() if isinstance(v, CapturedStep)]
    print('step() stream: %d steps, captures %d, replays of the one graph %s, nodes %s (put: %s)'
          % (steps, sg.captures, [v.replays for v in graphs], [v.graph.num_nodes for v in graphs], [v.graph.num_nodes for v in put_graphs]))
    # step 0 is the shape's first sighting (eager: the insert is materialised), step 1 captures and launches, every later step replays
    assert sg.captures == 1 and len(graphs) == 1 and graphs[0].replays == steps - 2
    assert sp.captures == 1 and len(put_graphs) == 1
    assert graphs[0].graph.num_nodes == put_graphs[0].graph.num_nodes + 1


def test_captured_step_holds_none_of_the_callers_frames():
    import gc
    import weakref
    B, Q, T = 2, 49, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    m = build(T, len(SIZES), 23, graph=True)
    frames = Frames(230)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=24)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool = FramePool(T, n_slots=6)
    refs = []
    for i in range(3):                                                 # sighting, capture, replay
        new = frames.newest(windows(i, T))
        refs.append(weakref.ref(new[0]))
        m(bbox, feat, pool.step(windows(i, T), new), None, metas)
        del new
    assert m.decoder._runtime.step_graphs.captures == 1
    gc.collect()
    assert refs[0]() is None and refs[1]() is None                    # the capturing call's frames went with the next step()
    assert refs[2]() is not None                                       # the live pyramid keeps its frames until the next step() / pyramid()
    pool.pyramid(windows(2, T))
    gc.collect()
    assert refs[2]() is None


@pytest.mark.parametrize('mode', ['graphs_off', 'layerwise'])
def test_stream_eager_placement(mode):
    run_streams(7, graph=False, layerwise=mode == 'layerwise', change=3, repeat=5)


def test_same_pyramid_twice():
    B, Q, T = 2, 49, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    m, m_put = build(T, len(SIZES), 25, graph=True), build(T, len(SIZES), 25, graph=True)
    frames = Frames(250)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=26)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool, p_put = FramePool(T, n_slots=6), FramePool(T, n_slots=6)
    for i in range(3):
        keys = windows(i, T)
        pyr = pool.step(keys, frames.newest(keys))
        a = m(bbox, feat, pyr, None, metas)                            # i = 0: eager then capture on ONE pyramid; later: two replays
        b = m(bbox, feat, pyr, None, metas)
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], want[0]) and torch.equal(a[1], want[1]), i
        pyr.materialise()                                              # ... and by hand, for readers outside the decoder: the same bytes again
        for buf_s, buf_p, in zip(pool.buffers, p_put.buffers):
            for s in range(B):
                slot, slot_p = int(pool.slot_table[s, 0]), int(p_put.slot_table[s, 0])
                assert torch.equal(buf_s[s, slot], buf_p[s, slot_p])
    assert m.decoder._runtime.step_graphs.captures == 1


def test_fp16_pool_through_step_equals_put():
    run_streams(4, graph=True, change=2, repeat=3, dtype=torch.float16)


def test_channels_last_frames_take_the_eager_store():
    run_streams(4, graph=True, change=2, repeat=3, channels_last=True)


def test_head_on_step_pyramid_equals_dense():
    from sparsebev_amd.head import SparseBEVHead
    B, T = 2, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    torch.manual_seed(0)
    head = SparseBEVHead(num_classes=10, in_channels=256, num_query=64, code_size=10,
                         transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=T, num_points=4, num_layers=2, num_levels=len(SIZES),
                                          num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                         bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=30,
                                         score_threshold=None, num_classes=10, pc_range=S.PC_RANGE)).to(DEV).eval()
    frames = Frames(270)
    metas = S.make_img_metas(B, T, ih, iw)
    pool = FramePool(T, n_slots=5)
    for i in range(3):                                                 # eager, capture, replay
        keys = windows(i, T)
        out_p = head(pool.step(keys, frames.newest(keys)), copy.deepcopy(metas))
        dense = [torch.stack([torch.cat([frames[k][l] for k in row], 0) for row in keys], 0) for l in range(len(SIZES))]
        out_d = head(dense, copy.deepcopy(metas))
        res_p, res_d = head.get_bboxes(out_p, metas), head.get_bboxes(out_d, metas)
        assert torch.equal(out_p['all_cls_scores'], out_d['all_cls_scores']) and torch.equal(out_p['all_bbox_preds'], out_d['all_bbox_preds']), i
        assert len(res_p) == len(res_d) == B and sum(r[0].shape[0] for r in res_p) > 0
        for (bb, ss, ll), (rb, rs, rl) in zip(res_p, res_d):
            assert torch.equal(bb, rb) and torch.equal(ss, rs) and torch.equal(ll, rl)
