"""The image front end on the device (csrc/image_front.hip behind sparsebev_amd.ImageFrontEnd): the plain path bit for bit against
torch's separate ops, the written padding, GridMask exhaustively at a small size, the reference's recording (fixture G16), every
transform on its own against the fp64 restatement, one captured launch replayed with two tables, the input forms, and one call whose
offsets pass 2^31."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_front_cases as C
from conftest import load_golden
from sparsebev_amd.image_front import FrontParams, ImageFrontEnd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4          # the project's fp32-vs-golden tolerance; outputs are O(1-5)


def metas_for(B):
    return [dict() for _ in range(B)]


def make_front(training, **kw):
    return ImageFrontEnd.from_data_aug(C.DATA_AUG, **kw).train(training)


# ---------------------------------------------------------------- plain path
PLAIN_SHAPES = [(1, 3, 1, 1), (13, 3, 37, 45), (2, 3, 64, 96), (3, 3, 33, 16)]


@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('src', ['uint8', 'float32'])
@pytest.mark.parametrize('shape', PLAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_plain_path_is_bit_equal_and_writes_the_padding(shape, src, to_rgb):
    """No colour aug, no mask: ((x.float()[:, perm] - mean) / std) padded by F.pad with torch on the same device, bit for bit, fp16 =
    .half() of it; the output buffer is NaN beforehand and no NaN survives."""
    img = torch.from_numpy(C.make_images(shape, 5, special=False)).to(DEV)
    if src == 'float32':
        g = torch.Generator(device=DEV).manual_seed(6)
        img = img.float() + torch.rand(shape, device=DEV, generator=g) - 0.5
    mean, std = torch.tensor(C.MEAN, device=DEV).view(1, 3, 1, 1), torch.tensor(C.STD, device=DEV).view(1, 3, 1, 1)
    x = img.float()
    if to_rgb:
        x = x[:, [2, 1, 0]]
    n, _, H, W = shape
    Hp, Wp = C.padded(H, W, 32)
    ref = F.pad((x - mean) / std, [0, Wp - W, 0, Hp - H], value=0)
    for out_dtype in (torch.float32, torch.float16):
        front = ImageFrontEnd(dict(mean=C.MEAN, std=C.STD, to_rgb=to_rgb), dict(size_divisor=32), out_dtype=out_dtype).eval()
        out = torch.full((n, 3, Hp, Wp), float('nan'), dtype=out_dtype, device=DEV)
        got = front(img, metas_for(1), out=out)
        assert got is out and not torch.isnan(out).any()
        assert torch.equal(out, ref if out_dtype == torch.float32 else ref.half()), (out.float() - ref).abs().max().item()
    # without an img_pad_cfg the output has the input's size
    front = ImageFrontEnd(dict(mean=C.MEAN, std=C.STD, to_rgb=to_rgb)).eval()
    assert torch.equal(front(img, metas_for(1)), ref[:, :, :H, :W])


# ---------------------------------------------------------------- GridMask
def mask_triples(Hp, cap=512):
    out = []
    for d in range(2, Hp):
        for st_h in range(d):
            for st_w in range(d):
                out.append((d, st_h, st_w))
                if len(out) == cap:
                    return out
    return out


@pytest.mark.parametrize('H,W,div', [(8, 40, 32), (8, 12, 1)])
def test_grid_mask_exhaustive(H, W, div):
    """One image per (d, st_h, st_w), all ones, identity normalisation: every image IS its mask (times the unpadded area)."""
    Hp, Wp = C.padded(H, W, div)
    triples = mask_triples(Hp)
    n = len(triples)
    assert n == (512 if div == 32 else 139)
    p = FrontParams(n)
    for i, (d, st_h, st_w) in enumerate(triples):
        p.mask[i] = (1, d, min(max(int(d * 0.5 + 0.5), 1), d - 1), st_h, st_w)
    img = np.ones((n, 3, H, W), dtype=np.uint8)
    front = ImageFrontEnd(None, dict(size_divisor=div)).train()
    out = front(torch.from_numpy(img).to(DEV), metas_for(1), params=p)
    want = C.pipeline_f64(img, [0, 0, 0], [1, 1, 1], False, div, rows=p.rows)
    assert out.shape == want.shape and 0 < want.mean() < 1
    bad = (out.cpu().double() != torch.from_numpy(want)).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, 'mask differs for (d, st_h, st_w) = %s' % [triples[i] for i in bad[:8]]


# ---------------------------------------------------------------- the reference's recording
@pytest.fixture(scope='module')
def g16():
    return load_golden('g16_image_front')


@pytest.mark.parametrize('call', C.G16_CALLS)
def test_fixture_parity(g16, call):
    """The kernel with ``draw`` under the recorded seed against the reference's recorded fp32 output: 1e-4 absolute, no pixel excluded.
    Printed beside it: the error against the fp64 record and the reference's own fp32-vs-fp64 figure."""
    n, _, H, W = C.G16_SHAPES[call]
    N = C.G16_VIEWS[call]
    front = make_front(C.G16_TRAINING[call])
    np.random.seed(int(g16['seeds'][C.G16_CALLS.index(call)]))
    metas = metas_for(n // N)
    out = front(g16[call + '_img'].to(DEV).view(n // N, N, 3, H, W), metas).cpu()
    ref = g16[call + '_out']
    ref64 = ref.double() + g16[call + '_d64'].double() / 2.0 ** 20
    assert out.shape == ref.shape and out.dtype == torch.float32
    err = (out - ref).abs().max().item()
    err64, own = (out.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
    print('image front %-8s max |kernel - reference fp32| %.3g; vs the fp64 record: kernel %.3g, reference fp32 %.3g (all calls %.3g)'
          % (call, err, err64, own, float(g16['ref_fp32_vs_fp64'])))
    assert err < TOL
    assert metas[0]['pad_shape'] == [tuple(s) for s in g16[call + '_meta_pad_shape'][0].tolist()]
    assert isinstance(metas[0]['input_shape'], torch.Size) and list(metas[0]['input_shape']) == g16[call + '_meta_input_shape'].tolist()


# ---------------------------------------------------------------- one transform at a time
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
BRANCHES = ([('brightness', dict(flags=C.BRIGHT, delta=21.5)), ('contrast mode 0', dict(flags=C.CONTRAST, mode=0, alpha=1.37)),
             ('contrast mode 1', dict(flags=C.CONTRAST, mode=1, alpha=0.61)), ('saturation', dict(flags=C.SAT, sat=1.43)),
             ('hue +18', dict(flags=C.HUE, hue=18.0)), ('hue -18', dict(flags=C.HUE, hue=-18.0))],
            [('permutation %s' % (p,), dict(flags=C.SWAP, perm=p)) for p in PERMS])


@pytest.mark.parametrize('group', [0, 1], ids=['colour', 'permutations'])
def test_each_transform_alone(group):
    """[6, 3, 8, 16], table rows written by hand, exactly one transform per image, against the fp64 restatement at 1e-4."""
    cases = BRANCHES[group]
    img = C.make_images((6, 3, 8, 16), 31 + group, special=False)
    p = FrontParams(6)
    for i, (_, fields) in enumerate(cases):
        for k, v in fields.items():
            getattr(p, k)[i] = v
    front = make_front(True, use_grid_mask=False)
    out = front(torch.from_numpy(img).to(DEV), metas_for(1), params=p).cpu().double()
    want = torch.from_numpy(C.pipeline_f64(img, C.MEAN, C.STD, True, 32, rows=p.rows, colour=True))
    for i, (name, _) in enumerate(cases):
        err = (out[i] - want[i]).abs().max().item()
        print('image front, %s alone: max err %.3g' % (name, err))
        assert err < TOL, name
    assert out.shape == (6, 3, 32, 32) and not out[:, :, 8:].any() and not out[:, :, :, 16:].any()


# ---------------------------------------------------------------- one captured launch, two tables
def test_captured_launch_serves_two_tables():
    img = torch.from_numpy(C.make_images((4, 3, 37, 45), 41)).to(DEV)
    front = make_front(True)
    rng = np.random.RandomState(3)
    A, B = front.draw(4, 64, rng=rng), front.draw(4, 64, rng=rng)
    A.mask[:] = (1, 9, 5, 2, 7)                  # both masked, differently
    B.mask[:] = (1, 23, 12, 20, 1)
    assert not np.array_equal(A.table(), B.table())
    eager = [front(img, metas_for(1), params=t).clone() for t in (A, B)]
    assert not torch.equal(eager[0], eager[1])
    front.upload(A)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        out = front(img, metas_for(1))
    for t, want in ((A, eager[0]), (B, eager[1])):
        front.upload(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ---------------------------------------------------------------- input forms
def test_input_forms_and_cpu_refusal():
    raw = C.make_images((4, 3, 9, 20), 51, special=False)
    flat = torch.from_numpy(raw).to(DEV)
    front = make_front(False, out_dtype=torch.float16)
    want = front(flat, metas_for(2))
    assert want.shape == (4, 3, 32, 32) and want.dtype == torch.float16
    m5, ml = metas_for(2), metas_for(2)
    assert torch.equal(front(flat.view(2, 2, 3, 9, 20), m5), want)
    assert torch.equal(front([flat[:2], flat[2:]], ml), want)
    assert m5 == ml and m5[1]['img_shape'] == [(32, 32, 3)] * 2 and m5[1]['ori_shape'] == [(9, 20, 3)] * 2
    with pytest.raises(RuntimeError, match='device tensors'):
        front(torch.from_numpy(raw), metas_for(2))
    with pytest.raises(TypeError):
        front(flat.to(torch.int32), metas_for(2))
    with pytest.raises(ValueError, match='contiguous'):
        front(flat[:, :, :, ::2], metas_for(2))


# ---------------------------------------------------------------- offsets beyond 2^31
def test_offsets_beyond_32_bits():
    """n * 3 * H * W > 2^31 elements on both sides: single images of the big call equal the same images on their own."""
    n, H, W = 10930, 256, 256
    assert n * 3 * H * W > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(7)
    img = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=DEV, generator=g)
    front = make_front(True, use_grid_mask=False, out_dtype=torch.float16)
    p = front.draw(n, H, rng=np.random.RandomState(9))
    out = front(img, metas_for(1), params=p)
    for i in (0, n // 2 + 1, n - 1):
        one = FrontParams(1)
        one.rows[:] = p.rows[i:i + 1]
        assert torch.equal(front(img[i:i + 1], metas_for(1), params=one), out[i:i + 1]), i
