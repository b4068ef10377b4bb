"""ResNetBackbone on the device against the fp64 restatement of its definition (resnet_cases.py), into NaN-filled destinations
throughout.  Integers make the structural tests exact (torch.equal): one convolution of every kind at every column tile and epilogue,
the fold + pack image bit for bit, the stem and the pool.  Real-valued data is held launch by launch against fp64 on the device's own
input activations, inside the worst-case fp32 accumulation bound; then the pack's version key, capture, and the hand-over to FPNNeck,
FeaturePyramid and a decoder step."""
import functools

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

import fpn_cases as FC  # noqa: E402
import resnet_cases as RC  # noqa: E402
from sparsebev_amd import resnet as R  # noqa: E402

DEV = 'cuda:0'
F16, F32 = torch.float16, torch.float32
R50 = (3, 4, 6, 3)


# ---- 1. one convolution, exact on integers -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def integer_conv(name):
    """integer data, its fold and the fp64 restatement per epilogue, computed once per case and never written to"""
    case = RC.CONV_BY_NAME[name]
    x, res, layer = RC.integer_conv_data(case, seed=11)
    wq, bq = RC.fold32(*layer)
    want = {e: RC.conv_layer(x, wq, bq, case.stride, case.k // 2, e, res)[0] for e in RC.EPILOGUES}
    return x, res, layer, wq, bq, want


@pytest.mark.parametrize('epilogue', RC.EPILOGUES)
@pytest.mark.parametrize('name', [c.name for c in RC.CONV_CASES])
def test_conv_exact_on_integers(name, epilogue):
    case = RC.CONV_BY_NAME[name]
    x, res, layer, wq, bq, want = integer_conv(name)
    # the premises of exactness, on the CPU first: the fold gives integers, every result is an fp16 integer, the ReLU has work to do
    assert torch.equal(wq.float(), wq.float().round()) and torch.equal(bq, bq.round()) and float(wq.float().abs().max()) == 2.0
    assert all(float(w.abs().max()) < 2 ** 11 and torch.equal(w, w.round()) for w in want.values())
    assert float(want['bias'].min()) < -8 and float(want['relu'].min()) == 0.0 and not torch.equal(want['relu'], want['residual_relu'])
    pack, offs, _ = R.pack_layers([tuple(t.to(DEV) for t in layer)])
    gw, gb = RC.unpack_fragments(pack, offs[0], case.cout, case.cin, case.k)
    assert torch.equal(gw, wq) and torch.equal(gb, bq)
    xd, rd = RC.nhwc(x, DEV), RC.nhwc(res, DEV)
    n, _, h, w = want[epilogue].shape
    for ct in RC.col_tiles(case.cout):
        y = torch.full((n, h, w, case.cout), float('nan'), dtype=F16, device=DEV)
        R.conv_f16(xd, pack, rd if epilogue == 'residual_relu' else None, y, case.k ** 2, case.stride, epilogue, ct)
        assert torch.equal(y.permute(0, 3, 1, 2).cpu().double(), want[epilogue]), 'col_tile %d' % ct


def test_fold_and_pack_restated_bit_for_bit():
    """real-valued weights and statistics: the image holds exactly fold32's w' and b' (fp32 and fp16 weights; 1 x 1, 3 x 3 and the stem)"""
    g = torch.Generator().manual_seed(21)
    layers = []
    for cout, cin, k in ((64, 3, 7), (128, 64, 3), (192, 128, 1)):
        layers.append((torch.randn(cout, cin, k, k, generator=g), 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g),
                       torch.randn(cout, generator=g), 0.01 + 4 * torch.rand(cout, generator=g)))
    for dtype in (F32, F16):
        cast = [(l[0].to(dtype),) + l[1:] for l in layers]
        pack, offs, _ = R.pack_layers([tuple(t.to(DEV) for t in l) for l in cast], eps=RC.EPS)
        for l, off in zip(cast, offs):
            wq, bq = RC.fold32(*l)
            gw, gb = RC.unpack_fragments(pack, off, *l[0].shape[:3])
            assert torch.equal(gw, wq) and torch.equal(gb, bq), (dtype, tuple(l[0].shape))


# ---- 2. stem + pool ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [F32, F16], ids=['in32', 'in16'])
@pytest.mark.parametrize('H,W', [(9, 13), (32, 64)])
def test_stem_and_pool_exact_on_integers(H, W, dtype):
    blocks = (1,)
    params = RC.integer_params(blocks, seed=12)
    x = torch.randint(-2, 3, (2, 3, H, W), generator=torch.Generator().manual_seed(13)).float()
    want = RC.reference(x, params, blocks)[:2]
    assert 2 ** 11 > float(want[0].max()) > 2 ** 4 and torch.equal(want[0], want[0].round()) and float(want[0].min()) == 0.0
    net = RC.make_backbone(blocks, params, DEV)
    keep = []
    out = net(x.to(device=DEV, dtype=dtype), out=RC.nan_outputs([(2, 256, want[1].shape[2], want[1].shape[3])], DEV), keep=keep)
    assert len(keep) == 6 and keep[5].data_ptr() == out[0].data_ptr()
    assert torch.equal(keep[0].cpu().double(), want[0]), 'stem'
    assert torch.equal(keep[1].cpu().double(), want[1]), 'pool'


def test_fp32_images_round_to_nearest_even():
    blocks = (1, 1)
    params = RC.real_params(blocks, seed=14)
    x = torch.randn(2, 3, 17, 23, generator=torch.Generator().manual_seed(15))
    ties = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25])
    for c in range(3):
        x[:, c].reshape(2, -1)[:, :len(ties)] = ties
        x[1, c, 8, 5:5 + len(ties)] = ties
    assert not torch.equal(x.half().float(), x)
    net = RC.make_backbone(blocks, params, DEV)
    a, b = [], []
    net(x.to(DEV), keep=a)
    a = [t.clone() for t in a]
    net(x.half().to(DEV), keep=b)
    assert len(a) == len(b) == 10
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q) and bool(torch.isfinite(p).all()), i


# ---- 3. the whole network, launch by launch ------------------------------------------------------------------------------------------

def test_resnet50_real_data_launch_by_launch():
    """ResNet-50 on 2 images of 3 x 40 x 72 (planes 10 x 18, 5 x 9, 3 x 5, 2 x 3: odd at every stride-2 step).  Bound
    (resnet_cases.layer_bound): |got - s| <= 2^-11 |s| + 2^-25 + (K + 4) 2^-23 A, s = fp64 on the device's own input activations,
    K = taps x Cin, A = sum of absolute products + |b'| + |residual|: the worst case of fp32 accumulation with a factor 2 for additions
    inside the matrix core that do not round to nearest."""
    params = RC.real_params(R50, seed=5)
    x = torch.randn(2, 3, 40, 72, generator=torch.Generator().manual_seed(6))
    cpu = RC.reference(x, params, R50)
    assert max(float(a.abs().max()) for a in cpu) < 6e4 and min(float(a.abs().max()) for a in cpu) > 1e-2
    net = RC.make_backbone(R50, params, DEV)
    shapes = [(2, 256, 10, 18), (2, 512, 5, 9), (2, 1024, 3, 5), (2, 2048, 2, 3)]
    out = RC.nan_outputs(shapes, DEV)
    keep = []
    got = net(x.to(DEV), out=out, keep=keep)
    assert len(keep) == 54
    for g, o, s, e in zip(got, out, shapes, RC.stage_ends(R50)):
        assert g.data_ptr() == o.data_ptr() == keep[e].data_ptr() and tuple(g.shape) == s and g.dtype == F16
        assert g.permute(0, 2, 3, 1).is_contiguous()
    rows = RC.layer_errors(keep, x, params, R50)
    worst = {}
    for r in rows:
        worst[r['kind']] = max(worst.get(r['kind'], 0.0), r['ratio'])
    print('largest error / bound per launch kind:', {k: round(v, 4) for k, v in worst.items()})
    for r in rows:
        assert r['finite'] and r['ratio'] <= 1.0, r
    # without keep the activations ping-pong in five regions: the same bits
    again = net(x.to(DEV), out=RC.nan_outputs(shapes, DEV))
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    # and only some stages, into tensors of the call's own
    some = RC.make_backbone(R50, params, DEV, out_indices=(1, 3))(x.to(DEV))
    assert torch.equal(some[0], got[1]) and torch.equal(some[1], got[3]) and some[0].permute(0, 2, 3, 1).is_contiguous()


# ---- 4. the pack follows the weights and the statistics ------------------------------------------------------------------------------

def test_weights_move():
    blocks = (1, 1)
    params = RC.real_params(blocks, seed=16)
    x = torch.randn(2, 3, 17, 23, generator=torch.Generator().manual_seed(17))
    net = RC.make_backbone(blocks, params, DEV)
    xd = x.to(DEV)

    def run_and_check(p):
        keep = []
        out = [o.clone() for o in net(xd, keep=keep)]
        rows = RC.layer_errors(keep, x, p, blocks)
        assert all(r['finite'] and r['ratio'] <= 1.0 for r in rows), [r for r in rows if not r['ratio'] <= 1.0]
        return out

    base = run_and_check(params)
    image = net.pack()
    before = image.clone()
    net(xd)
    assert net.pack() is image and torch.equal(image, before)          # nothing changed: no repack between two calls
    # a statistic written in place ...
    net.layer1[0].bn2.running_var[3:40].mul_(4)
    moved = {k: v.clone() for k, v in params.items()}
    moved['layer1.0.bn2.running_var'][3:40] *= 4
    got = run_and_check(moved)
    assert not torch.equal(net.pack(), before) and not torch.equal(got[0], base[0])
    assert net.pack().data_ptr() == image.data_ptr()          # repacked in place: an already captured forward reads the new image
    # ... a convolution weight written in place ...
    net.layer2[0].conv3.weight.mul_(0.5)
    moved['layer2.0.conv3.weight'] *= 0.5
    got2 = run_and_check(moved)
    assert torch.equal(got2[0], got[0]) and not torch.equal(got2[1], got[1])
    # ... and load_state_dict
    net.load_state_dict(params, strict=True)
    back = run_and_check(params)
    assert all(torch.equal(a, b) for a, b in zip(back, base))


def test_a_forward_that_needs_a_gradient_is_refused():
    blocks = (1,)
    net = RC.make_backbone(blocks, RC.real_params(blocks, seed=18), DEV)
    x = torch.randn(1, 3, 8, 8, device=DEV)
    with torch.enable_grad():                                     # the suite runs under no_grad
        with pytest.raises(RuntimeError, match='backward is not built'):
            net(x.clone().requires_grad_(True))
        net.conv1.weight.requires_grad_(True)
        with pytest.raises(RuntimeError, match='backward is not built'):
            net(x)
        with torch.no_grad():
            assert bool(torch.isfinite(net(x)[0]).all())
    net.conv1.weight.requires_grad_(False)
    with pytest.raises(ValueError, match='NCHW-contiguous'):
        net(torch.randn(1, 3, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last))
    with pytest.raises(TypeError, match='fp32 or fp16'):
        net(x.double())
    assert [tuple(o.shape) for o in net(x[:0])] == [(0, 256, 2, 2)]


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------

def test_capture_and_replay():
    """one forward captured with out=: no allocation in the call; a replay after the image was overwritten in place equals the eager
    call bit for bit"""
    blocks = (1, 1, 1, 1)
    params = RC.real_params(blocks, seed=19)
    g = torch.Generator().manual_seed(20)
    x1, x2 = torch.randn(2, 3, 40, 72, generator=g), torch.randn(2, 3, 40, 72, generator=g)
    net = RC.make_backbone(blocks, params, DEV)
    shapes = [(2, 256, 10, 18), (2, 512, 5, 9), (2, 1024, 3, 5), (2, 2048, 2, 3)]
    x, out = x1.to(DEV), RC.nan_outputs(shapes, DEV)
    net(x, out=out)                                               # packs, allocates the workspace
    torch.cuda.synchronize()
    allocs = torch.cuda.memory_stats(DEV)['allocation.all.allocated']
    net(x, out=out)
    assert torch.cuda.memory_stats(DEV)['allocation.all.allocated'] == allocs
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net(x, out=out)
    x.copy_(x2.to(DEV))                                           # new values at the captured address
    for o in out:
        o.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    eager = net(x2.to(DEV), out=RC.nan_outputs(shapes, DEV))
    first = net(x1.to(DEV))
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(replayed, eager))
    assert not torch.equal(first[0], eager[0])


# ---- 6. hand-over --------------------------------------------------------------------------------------------------------------------

def test_neck_pyramid_and_decoder_take_the_outputs_in_place():
    from sparsebev_amd import FPNNeck
    from sparsebev_amd import synthetic as S
    from sparsebev_amd.transformer import FeaturePyramid, SparseBEVTransformer
    B, T, Q = 1, 2, 49
    ih, iw, sizes = S.PYRAMIDS['tiny']                            # images of 32 x 88 give exactly these planes
    params = RC.real_params(R50, seed=22)
    net = RC.make_backbone(R50, params, DEV)
    x = torch.randn(B * T * 6, 3, 32, 88, generator=torch.Generator().manual_seed(23)).to(DEV)
    stages = net(x)
    assert [tuple(s.shape[2:]) for s in stages] == [tuple(s) for s in sizes]
    ptrs = [s.data_ptr() for s in stages]
    clones = [FC.channels_last(s.clone()) for s in stages]
    torch.manual_seed(24)
    neck = FPNNeck([256, 512, 1024, 2048], 256, 4).to(DEV).eval()
    with torch.no_grad():
        pyramid = neck(stages, out_dtype=F32)
        want = neck(clones, out_dtype=F32)
    assert [s.data_ptr() for s in stages] == ptrs and all(torch.equal(s, c) for s, c in zip(stages, clones))      # read in place, unchanged
    assert all(torch.equal(p, w) and bool(torch.isfinite(p).all()) for p, w in zip(pyramid, want))
    feats = [p.view(B, T * 6, 256, h, w) for p, (h, w) in zip(pyramid, sizes)]
    pyr = FeaturePyramid(feats)
    assert pyr.copied == 0 and all(level.data_ptr() == p.data_ptr() for level, p in zip(pyr.levels, pyramid))
    dec = S.make_params(3, embed_dims=256, num_frames=T, num_points=4, num_levels=len(sizes))
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=2, num_levels=len(sizes), num_classes=10, code_size=10, pc_range=S.PC_RANGE)
    m.load_state_dict({'decoder.decoder_layer.' + k: v for k, v in dec.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = False
    bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=4)]
    got = m(bbox, feat, feats, None, S.make_img_metas(B, T, ih, iw))
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
