"""Several frames per step, channels-last and widened: sbev_pool_insert_frames against torch, and FramePool.stream against FramePool.put.
Every comparison is bitwise -- the insert is byte movement or an exact widening (fp16 / bf16 -> fp32), and the decoder afterwards runs the
same kernels on the same slot contents -- so no tolerance appears anywhere.  Shapes are the tiny pyramid's: vector planes (8 x 22, 4 x 11,
2 x 6) and a scalar one (1 x 3, NCHW) in one launch, a partial pixel tile (176 = 2 * 64 + 48), several blocks per level."""
import ctypes

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

from sparsebev_amd import cache, synthetic as S  # noqa: E402
from sparsebev_amd.cache import FramePool  # noqa: E402
from sparsebev_amd.transformer import SparseBEVTransformer  # noqa: E402
from sparsebev_amd.utils import FrameInsert  # noqa: E402

DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
N = 6
SIZES = S.PYRAMIDS['tiny'][2]
L = len(SIZES)
# bit patterns no input holds: NaNs with a payload (randn, its roundings to fp16 / bf16 and their widenings are finite)
PATTERN = {torch.float32: (torch.int32, 0x7fc12345), torch.float16: (torch.int16, 0x7e01), torch.bfloat16: (torch.int16, 0x7fc1)}
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def channels_last(f):
    """the same [..., C, H, W] values in channels-last memory"""
    d = f.dim()
    return f.permute(*range(d - 3), d - 2, d - 1, d - 3).contiguous().permute(*range(d - 3), d - 1, d - 3, d - 2)


# ---- 1. the kernel against torch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [256, 64])
@pytest.mark.parametrize('src,dst', [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)])
@pytest.mark.parametrize('nhwc', [False, True])
def test_pool_insert_frames_kernel_equals_torch(nhwc, src, dst, C):
    B, n_slots = 3, 4
    assert list(SIZES) == [(8, 22), (4, 11), (2, 6), (1, 3)]
    g = torch.Generator(device=DEV).manual_seed(7 + C)
    sets = [[torch.randn(B, N, C, h, w, generator=g, device=DEV).to(src) for h, w in SIZES] for _ in range(3)]
    if nhwc:
        sets = [[channels_last(f) for f in fs] for fs in sets]
        assert not sets[0][0].is_contiguous() and sets[0][0].permute(0, 1, 3, 4, 2).is_contiguous()
    ity, pat = PATTERN[dst]
    bufs = [torch.empty(B, n_slots, N, h, w, C, device=DEV, dtype=dst) for h, w in SIZES]
    want_of = [[f.permute(0, 1, 3, 4, 2).to(dst).contiguous().view(ity) for f in fs] for fs in sets]      # [k][l] -> [B, 6, H, W, C] bits
    assert not any(bool((w == pat).any()) for ws in want_of for w in ws)

    def run(rows, K, indirect):
        for buf in bufs:
            buf.view(ity).fill_(pat)
        flat = [f for fs in sets[:K] for f in fs]
        dev_rows = torch.tensor(rows, device=DEV, dtype=torch.int32)
        assert tuple(dev_rows.shape) == (K, B)
        if indirect:
            table = torch.tensor([0, 0, 0] + [f.data_ptr() for f in flat], device=DEV, dtype=torch.int64)
            cache.pool_insert_frames(flat, bufs, dev_rows, n_slots, stream(), nhwc, table=ctypes.c_void_p(table.data_ptr()), index=list(range(3, 3 + K * L)))
        else:
            cache.pool_insert_frames(flat, bufs, dev_rows, n_slots, stream(), nhwc)
        torch.cuda.synchronize()

    def check(rows):
        for l, buf in enumerate(bufs):
            want = torch.full_like(buf.view(ity), pat)
            for k, row in enumerate(rows):
                for b, slot in enumerate(row):
                    if 0 <= slot < n_slots:
                        want[b, slot] = want_of[k][l][b]
            assert torch.equal(buf.view(ity), want), (l, rows)          # written slots bit-equal, every other element untouched

    for indirect in (False, True):
        for K, rows in ((1, [[2, -1, 0]]), (3, [[2, -1, 0], [0, -1, 1], [-1, -1, 3]])):      # sample 1: none; sample 2: three frames at once
            run(rows, K, indirect)
            check(rows)
            run([[n_slots, -5, -1]] * K, K, indirect)                      # outside [0, n_slots): nothing is written, nothing is clamped
            check([[-1] * B] * K)
            for k in range(K):                                             # every sample, the last slot, for every k: the far end of every buffer
                rows_k = [[n_slots - 1] * B if j == k else [-1] * B for j in range(K)]
                run(rows_k, K, indirect)
                check(rows_k)
                for l, buf in enumerate(bufs):
                    assert torch.equal(buf[:, n_slots - 1].view(ity), want_of[k][l])


def test_pool_insert_frames_scalar_forms():
    """sizes no vector form takes, in both layouts: 5 channels (NCHW: not a multiple of 4 / 8; channels-last: a sample's run of
    6 * hw * 5 two-byte elements is no multiple of 16 bytes at hw = 3 and hw = 1)"""
    B, n_slots, C = 2, 3, 5
    sizes = [(3, 3), (1, 3), (1, 1)]
    g = torch.Generator(device=DEV).manual_seed(11)
    for src, dst in ((F32, F32), (BF16, BF16), (F16, F32), (BF16, F32)):
        for nhwc in (False, True):
            frames = []
            for h, w in sizes:
                f = torch.randn(B, N, C, h, w, generator=g, device=DEV).to(src)
                frames.append(channels_last(f) if nhwc else f)
            assert all(f.data_ptr() % 16 == 0 for f in frames)
            ity, pat = PATTERN[dst]
            bufs = [torch.empty(B, n_slots, N, h, w, C, device=DEV, dtype=dst) for h, w in sizes]
            for buf in bufs:
                buf.view(ity).fill_(pat)
            rows = torch.tensor([[2, 0]], device=DEV, dtype=torch.int32)
            cache.pool_insert_frames(frames, bufs, rows, n_slots, stream(), nhwc)
            torch.cuda.synchronize()
            for f, buf in zip(frames, bufs):
                want = torch.full_like(buf.view(ity), pat)
                want[0, 2] = f[0].permute(0, 2, 3, 1).to(dst).contiguous().view(ity)
                want[1, 0] = f[1].permute(0, 2, 3, 1).to(dst).contiguous().view(ity)
                assert torch.equal(buf.view(ity), want), (src, dst, nhwc, tuple(f.shape))


# ---- the decoder step ----------------------------------------------------------------------------------------------------------------

def build(T, seed, num_layers=2, graph=False):
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=L)
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=num_layers, num_levels=L, num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = graph
    return m


class Frames:
    """key -> one sample's frame (list over levels of [6, C, H, W] NCHW, of the backbone's type), generated once and kept"""

    def __init__(self, seed, dtype=F32, C=256):
        self.g, self.dtype, self.C, self.frames = torch.Generator(device=DEV).manual_seed(seed), dtype, C, {}

    def __getitem__(self, key):
        if key not in self.frames:
            self.frames[key] = [torch.randn(N, self.C, h, w, generator=self.g, device=DEV).to(self.dtype) for h, w in SIZES]
        return self.frames[key]

    def at(self, keys, t, nhwc=False):
        """what a backbone hands over for the batch's images of window position t: list over levels of NEW [B, 6, C, H, W] tensors"""
        out = [torch.stack([self[row[t]][l] for row in keys], 0) for l in range(L)]
        return [channels_last(f) for f in out] if nhwc else out


def put_feed(pool, frames, keys):
    """the put() flow; 2-byte frames are widened first (exactly), as fp32 NCHW maps are what put() takes for fp32 slots"""
    for b, k in pool.missing(keys):
        pool.put(b, k, [f.to(pool.dtype) for f in frames[k]])
    return pool.pyramid(keys)


CHANGES = {4: 1, 7: 0, 9: 1}          # step -> the sample that changes scene there, to a window of T distinct keys
REPEAT = 6                            # this step repeats the one before it


def windows(i, T):
    """keys of step i for two samples.  Step 0: one frame, the window padded by duplicates.  At a scene change the sample's window is T
    distinct keys of the new scene, none of them seen before; step REPEAT repeats the step before it."""
    n = i if i < REPEAT else i - 1
    rows = []
    for b in range(2):
        since = [c for c, who in CHANGES.items() if who == b and c <= i]
        rows.append([(b, len(since), n - t) for t in range(T)] if since else [(b, 0, max(n - t, 0)) for t in range(T)])
    return rows


def offered_positions(pool, keys):
    """what the caller brings: per missing key the lowest position that carries it; nothing missing: the newest frame anyway (a no-op launch)"""
    return sorted({min(t for t, k in enumerate(keys[b]) if k == key) for b, key in pool.missing(keys)} or {0})


def run_streams(steps, graph, layerwise=False, src=F32, nhwc=False):
    """the same stream through put() and through stream(), two models of equal weights and two pools (fp32 slots); asserts equal outputs
    and slot tables step by step and returns (put model, stream model, the K of every step)"""
    B, Q, T, n_slots = 2, 49, 4, 6
    ih, iw, _ = S.PYRAMIDS['tiny']
    m_put, m_new = build(T, 21, graph=graph), build(T, 21, graph=graph)
    frames = Frames(310, src)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=22)]
    metas = S.make_img_metas(B, T, ih, iw)
    p_put, p_new = FramePool(T, n_slots=n_slots), FramePool(T, n_slots=n_slots)
    kw = dict(layerwise=True) if layerwise else {}
    seen, alive, ptr, Ks = set(), [], None, []
    for i in range(steps):
        keys = windows(i, T)
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas, **kw)
        ts = offered_positions(p_new, keys)
        assert ts == (list(range(T)) if i in CHANGES else [0]), (i, ts)
        new = {t: frames.at(keys, t, nhwc) for t in ts}                  # allocated for this step and kept: no address comes back
        alive.append(new)
        seen.add(new[ts[0]][0].data_ptr())
        pyr = p_new.stream(keys, new)
        ptr = ptr or pyr.slot_table.data_ptr()
        assert pyr.slot_table.data_ptr() == ptr == p_new.slot_table.data_ptr() and tuple(pyr.slot_table.shape) == (B, T)
        assert isinstance(pyr.insert, FrameInsert) and pyr.insert.nhwc == nhwc and tuple(pyr.insert.rows.shape) == (len(ts), B)
        assert pyr.insert.rows.data_ptr() == p_new.insert_row.data_ptr() == ptr + 4 * B * T and tuple(p_new.insert_row.shape) == (B,)
        live = pyr.insert.rows.tolist()
        if i == REPEAT:
            assert live == [[-1] * B]                                   # nothing new: the step's launch is a no-op
        if i in CHANGES:                                                 # the changed sample takes T frames, the other its newest only
            b = CHANGES[i]
            assert all(live[t][b] >= 0 for t in range(T)) and len({live[t][b] for t in range(T)}) == T
            assert live[0][1 - b] >= 0 and all(live[t][1 - b] == -1 for t in range(1, T))
        got = m_new(bbox, feat, pyr, None, metas, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
        assert torch.equal(p_new.slot_table, p_put.slot_table) and got[0].abs().max() > 0
        Ks.append(len(ts))
    assert len(seen) == steps
    for buf_n, buf_p in zip(p_new.buffers, p_put.buffers):             # the streams end with the same resident frames in the same slots
        for b in range(B):
            for s in set(p_new.slot_table[b].tolist()):
                assert torch.equal(buf_n[b, s], buf_p[b, s])
    return m_put, m_new, Ks


@pytest.mark.parametrize('src,nhwc', [(F16, True), (F32, False), (BF16, False)], ids=['nhwc_f16', 'nchw_f32', 'nchw_bf16'])
def test_stream_through_stream_equals_put_one_graph_per_offered_shape(src, nhwc):
    from sparsebev_amd.runtime import CapturedStep
    steps = 12
    m_put, m_new, Ks = run_streams(steps, graph=True, src=src, nhwc=nhwc)
    sg, sp = m_new.decoder._runtime.step_graphs, m_put.decoder._runtime.step_graphs
    graphs = [v for v in sg.entries.values() if isinstance(v, CapturedStep)]
    put_graphs = [v for v in sp.entries.values() if isinstance(v, CapturedStep)]
    print('stream() stream: %d steps, K per step %s, captures %d, replays %s, nodes %s (put: %s)'
          % (steps, Ks, sg.captures, [v.replays for v in graphs], [v.graph.num_nodes for v in graphs], [v.graph.num_nodes for v in put_graphs]))
    # two offered shapes: K = 1 (9 steps) and the scene start, K = T (3 steps).  Of each the first step is the shape's first sighting
    # (eager: the insert is materialised), the second captures and launches, every later one replays
    assert Ks.count(1) == 9 and Ks.count(4) == 3 and len(CHANGES) == 3
    assert sg.captures == 2 and len(graphs) == 2 and sorted(v.replays for v in graphs) == [3 - 2, 9 - 2]
    assert sg.replays == steps - 2 and sp.captures == 1 and len(put_graphs) == 1
    for v in graphs:
        assert v.graph.num_nodes == put_graphs[0].graph.num_nodes + 1


@pytest.mark.parametrize('mode', ['graphs_off', 'layerwise'])
@pytest.mark.parametrize('src,nhwc', [(F16, True), (F32, False), (BF16, False)], ids=['nhwc_f16', 'nchw_f32', 'nchw_bf16'])
def test_stream_eager_placement(src, nhwc, mode):
    m_put, m_new, Ks = run_streams(10, graph=False, layerwise=mode == 'layerwise', src=src, nhwc=nhwc)
    assert m_new.decoder._runtime is None or m_new.decoder._runtime.step_graphs.captures == 0


def test_two_byte_pool_through_stream_equals_put():
    """fp16 slots take fp16 frames as bytes, either layout; fp32 frames for them are refused, as put() refuses them"""
    B, T = 2, 4
    keys = windows(4, T)
    frames = Frames(330, F16)
    for nhwc in (False, True):
        p_put, p_new = FramePool(T, n_slots=6, dtype=F16), FramePool(T, n_slots=6, dtype=F16)
        put_feed(p_put, frames, keys)
        pyr = p_new.stream(keys, {t: frames.at(keys, t, nhwc) for t in range(T)})
        assert isinstance(pyr.insert, FrameInsert)
        pyr.materialise()
        assert torch.equal(p_new.slot_table, p_put.slot_table)
        for buf_n, buf_p in zip(p_new.buffers, p_put.buffers):
            for b in range(B):
                for s in set(p_new.slot_table[b].tolist()):
                    assert torch.equal(buf_n[b, s], buf_p[b, s])
    with pytest.raises(RuntimeError, match='takes torch.float16 frames only'):
        FramePool(T, n_slots=6, dtype=F16).stream(keys, {t: Frames(331, F32).at(keys, t) for t in range(T)})


def test_step_and_stream_k1_share_one_graph():
    """step(keys, new) is stream(keys, {0: new}): once the window is full, even steps go through step() and odd ones through stream(), new
    frame tensors every step.  Both hand out a FrameInsert with K = 1, NCHW, the rows at the insert row's address, so the one graph
    captured at step 1 (through stream()) is replayed by both; outputs are bitwise those of a put()-fed twin model at every step."""
    B, Q, T, n_slots, steps = 2, 49, 4, 6, 8
    ih, iw, _ = S.PYRAMIDS['tiny']
    m_put, m_new = build(T, 29, graph=True), build(T, 29, graph=True)
    frames = Frames(370)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=30)]
    metas = S.make_img_metas(B, T, ih, iw)
    p_put, pool = FramePool(T, n_slots=n_slots), FramePool(T, n_slots=n_slots)
    alive, through_step = [], []
    for i in range(steps):
        keys = [[(b, 0, max(i - t, 0)) for t in range(T)] for b in range(B)]      # one new frame per sample and step, no scene change
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas)
        new = frames.at(keys, 0)                                         # allocated for this step and kept: no address comes back
        alive.append(new)
        through_step.append(i >= T - 1 and i % 2 == 0)
        pyr = pool.step(keys, new) if through_step[-1] else pool.stream(keys, {0: new})
        assert isinstance(pyr.insert, FrameInsert) and pyr.insert.K == 1 and pyr.insert.nhwc is False
        assert pyr.insert.rows.data_ptr() == pool.insert_row.data_ptr() and tuple(pyr.insert.rows.shape) == (1, B)
        assert all(s >= 0 for s in pyr.insert.rows.tolist()[0])
        got = m_new(bbox, feat, pyr, None, metas)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
        assert torch.equal(pool.slot_table, p_put.slot_table) and got[0].abs().max() > 0
    assert len({f[0].data_ptr() for f in alive}) == steps and through_step.count(True) >= 2
    from sparsebev_amd.runtime import CapturedStep
    sg = m_new.decoder._runtime.step_graphs
    graphs = [v for v in sg.entries.values() if isinstance(v, CapturedStep)]
    # step 0 is the shape's first sighting (eager), step 1 captures and launches, every later step replays -- whichever method fed it
    assert sg.captures == 1 and len(graphs) == 1 and graphs[0].replays == steps - 2


# ---- 3. the captured step holds none of the caller's frames --------------------------------------------------------------------------

def test_captured_step_holds_none_of_the_callers_frames():
    import gc
    import weakref
    B, Q, T = 2, 49, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    m = build(T, 23, graph=True)
    frames = Frames(340, F16)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=24)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool = FramePool(T, n_slots=6)
    refs = []
    for i in range(3):                                                 # sighting, capture, replay
        new = {0: frames.at(windows(i, T), 0, nhwc=True)}
        refs.append(weakref.ref(new[0][0]))
        m(bbox, feat, pool.stream(windows(i, T), new), None, metas)
        del new
    assert m.decoder._runtime.step_graphs.captures == 1
    gc.collect()
    assert refs[0]() is None and refs[1]() is None                    # the capturing call's frames went with the next stream()
    assert refs[2]() is not None                                       # the live pyramid keeps its frames until the next stream() / step() / pyramid()
    pool.pyramid(windows(2, T))
    gc.collect()
    assert refs[2]() is None


# ---- 4. the same pyramid handed to the decoder twice ---------------------------------------------------------------------------------

def test_same_pyramid_twice():
    B, Q, T = 2, 49, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    m, m_put = build(T, 25, graph=True), build(T, 25, graph=True)
    frames = Frames(350, F16)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=26)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool, p_put = FramePool(T, n_slots=6), FramePool(T, n_slots=6)
    for i in range(3):
        keys = windows(i, T)
        pyr = pool.stream(keys, {0: frames.at(keys, 0, nhwc=True)})
        a = m(bbox, feat, pyr, None, metas)                            # i = 0: eager then capture on ONE pyramid; later: two replays
        b = m(bbox, feat, pyr, None, metas)
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], want[0]) and torch.equal(a[1], want[1]), i
        pyr.materialise()                                              # ... and by hand, for readers outside the decoder: the same bytes again
        pyr.materialise()
        for buf_s, buf_p, in zip(pool.buffers, p_put.buffers):
            for s in range(B):
                slot, slot_p = int(pool.slot_table[s, 0]), int(p_put.slot_table[s, 0])
                assert torch.equal(buf_s[s, slot], buf_p[s, slot_p])
    assert m.decoder._runtime.step_graphs.captures == 1


# ---- 5. frames the kernel refuses take the eager store -------------------------------------------------------------------------------

@pytest.mark.parametrize('what', ['strided', 'mixed_layouts', 'misaligned'])
def test_frames_the_kernel_refuses_take_the_eager_store(what):
    B, Q, T = 2, 49, 4
    ih, iw, _ = S.PYRAMIDS['tiny']
    m, m_put = build(T, 27, graph=True), build(T, 27, graph=True)
    frames = Frames(360)
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=28)]
    metas = S.make_img_metas(B, T, ih, iw)
    pool, p_put = FramePool(T, n_slots=6), FramePool(T, n_slots=6)

    def spoil(fs):
        if what == 'strided':                  # rows of W + 1 elements: neither NCHW-contiguous nor channels-last
            out = []
            for f in fs:
                wide = torch.zeros(f.shape[:-1] + (f.shape[-1] + 1,), device=DEV, dtype=f.dtype)
                wide[..., :-1] = f
                out.append(wide[..., :-1])
            return out
        if what == 'mixed_layouts':            # level 0 channels-last, the others NCHW
            return [channels_last(fs[0])] + fs[1:]
        out = []                               # contiguous NCHW memory 4 bytes off a 16-byte boundary
        for f in fs:
            flat = torch.zeros(f.numel() + 1, device=DEV, dtype=f.dtype)
            flat[1:] = f.reshape(-1)
            out.append(flat[1:].view(f.shape))
        return out

    for i in (0, 1, 2, 4):                     # step 4: a scene change, T frames
        keys = windows(i, T)
        ts = offered_positions(pool, keys)
        new = {t: spoil(frames.at(keys, t)) for t in ts}
        assert pool._frames_layout([f for t in ts for f in new[t]]) is None
        pyr = pool.stream(keys, new)
        assert pyr.insert is None                                        # stored here and now, as put() stores
        got = m(bbox, feat, pyr, None, metas)
        want = m_put(bbox, feat, put_feed(p_put, frames, keys), None, metas)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
        assert torch.equal(pool.slot_table, p_put.slot_table)
    # the same frames, not spoiled, are the kernel's
    keys = windows(5, T)
    assert isinstance(pool.stream(keys, {0: frames.at(keys, 0)}).insert, FrameInsert)
