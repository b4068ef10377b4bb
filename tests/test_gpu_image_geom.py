"""The image geometry on the device (csrc/image_geom.hip behind sparsebev_amd.ImageGeometry): every case ``torch.equal`` to the numpy
restatement of Pillow's resampler (tests/image_geom_cases.py, pinned to Pillow and to the reference's recording by the host test), the
G17 calls also ``torch.equal`` to the recording itself; two samples with different transforms in one launch, full camera frames, one
captured launch replayed with two tables, the chain into ImageFrontEnd, source offsets beyond 2^31, and the refusals under a capture."""
import numpy as np
import pytest
import torch

import image_front_cases as F
import image_geom_cases as C
from conftest import load_golden
from sparsebev_amd.image_front import ImageFrontEnd
from sparsebev_amd.image_geom import GeomParams, ImageGeometry

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def conf_of(c):
    return dict(H=c['H'], W=c['W'], final_dim=(c['fH'], c['fW']), resize_lim=(1.0, 1.0), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=False)


def params_of(c):
    return GeomParams(c['resize_dims'][0] / c['W'], c['resize_dims'], c['crop'], c['flip'])


def restated(imgs, p):
    return torch.from_numpy(np.stack([C.transform(im, p.resize_dims, p.crop, p.flip) for im in imgs]))


def differing(got, want):
    bad = (got != want).nonzero()
    return '%d bytes differ, first at %s' % (len(bad), bad[0].tolist() if len(bad) else None)


@pytest.fixture(scope='module')
def g17():
    return load_golden('g17_image_geom')


# ---------------------------------------------------------------- the case list
@pytest.mark.parametrize('c', C.CASES, ids=lambda c: c['name'])
def test_case_equals_the_restatement(c):
    """Two images of one sample per launch: random bytes and the 0 / 255 pattern that drives both clamps.  The output buffer holds
    another value at every byte beforehand."""
    imgs = np.stack([C.random_bytes((c['H'], c['W'], 3), 11), C.extremes((c['H'], c['W'], 3), 12)])
    geom, p = ImageGeometry(conf_of(c)), params_of(c)
    want = restated(imgs, p)
    out = (~want).to(DEV)
    got = geom(torch.from_numpy(imgs).to(DEV), [dict()], params=[p], out=out)
    assert got is out and got.shape == (2, 3, c['fH'], c['fW']) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want), differing(got.cpu(), want)
    if c['name'] == 'overhang_right':
        assert not got[:, :, :, 34:].any() and got[:, :, :, 33].any()
    if c['name'] == 'overhang_mirror':
        assert not got[:, :, :, :11].any() and got[:, :, :, 11].any()
    if c['name'] == 'negative_crop_y':
        assert not got[:, :, :5].any() and got[:, :, 5].any()


# ---------------------------------------------------------------- the reference's recording
@pytest.mark.parametrize('conf', list(C.G17_CONFS))
def test_recorded_calls(g17, conf):
    """Each recorded call with ``draw`` under the recorded seed: the images equal the recording and the restatement, the metas equal
    what the reference left in ``results``."""
    raw = g17[conf + '_img']
    for call in C.G17_CALLS:
        geom = ImageGeometry(C.G17_CONFS[conf], training=call != 'eval')
        if call != 'eval':
            np.random.seed(int(call[5:]))
        metas = [dict(lidar2img=[m.copy() for m in g17[conf + '_l2i'].numpy()])]
        got = geom(raw.to(DEV).view(1, C.G17_VIEWS, *raw.shape[1:]), metas).cpu()
        want = g17['%s_%s_out' % (conf, call)].permute(0, 3, 1, 2)
        assert torch.equal(got, want), (call, differing(got, want))
        _, dims, crop, flip, _ = C.g17_params(g17, conf, call)
        assert torch.equal(got, restated(raw.numpy(), GeomParams(0.0, dims, crop, flip))), call
        after = g17['%s_%s_l2i_after' % (conf, call)].numpy()
        assert np.array_equal(np.stack(metas[0]['lidar2img']), after) and metas[0]['lidar2img'][0].dtype == after.dtype
        shapes = [tuple(s) for s in g17['%s_%s_shapes' % (conf, call)].tolist()]
        assert metas[0]['img_shape'] == metas[0]['ori_shape'] == metas[0]['pad_shape'] == shapes


# ---------------------------------------------------------------- two samples, two transforms, one launch
def test_two_samples_with_different_transforms():
    conf = dict(H=61, W=167, final_dim=(17, 65), resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True)
    geom = ImageGeometry(conf)
    a = GeomParams(0.47, (78, 28), (6, 5, 71, 22), False)
    b = GeomParams(0.41, (68, 25), (1, 8, 66, 25), True)
    imgs = C.random_bytes((6, 61, 167, 3), 21)
    metas = [dict(lidar2img=[np.eye(4) for _ in range(3)]) for _ in range(2)]
    got = geom(torch.from_numpy(imgs).to(DEV).view(2, 3, 61, 167, 3), metas, params=[a, b]).cpu()
    want = torch.cat([restated(imgs[:3], a), restated(imgs[3:], b)])
    for i in range(6):
        assert torch.equal(got[i], want[i]), (i, differing(got[i], want[i]))
    assert not torch.equal(restated(imgs[3:4], a), want[3:4])               # a wrong image -> block mapping would show
    assert np.array_equal(metas[0]['lidar2img'][2], geom.ida_mat(a)) and np.array_equal(metas[1]['lidar2img'][0], geom.ida_mat(b))
    assert [len(m['img_shape']) for m in metas] == [3, 3]
    # the flat form gives the same
    assert torch.equal(geom(torch.from_numpy(imgs).to(DEV), [dict(), dict()], params=[a, b]).cpu(), want)


# ---------------------------------------------------------------- full camera frames
@pytest.mark.parametrize('c', [C.FULL_EVAL, C.FULL_038], ids=lambda c: c['name'])
def test_full_frame(c):
    geom = ImageGeometry(C.R50_CONF, training=False)
    img = C.random_bytes((1, 900, 1600, 3), 31)
    img[0, 300:500] = C.extremes((200, 1600, 3), 32)
    p = params_of(c)
    if c is C.FULL_EVAL:
        assert geom.draw(1)[0][1:4] == (p.resize_dims, p.crop, False)         # the r50 config's eval transform
    got = geom(torch.from_numpy(img).to(DEV), [dict()], params=[p]).cpu()
    want = restated(img, p)
    assert got.shape == (1, 3, 256, 704) and torch.equal(got, want), differing(got, want)


# ---------------------------------------------------------------- one captured launch, two draws
def test_captured_launch_serves_two_draws():
    conf = dict(H=61, W=167, final_dim=(17, 65), resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True)
    geom = ImageGeometry(conf)
    rng = np.random.RandomState(4)
    A, B = geom.draw(2, rng=rng), geom.draw(2, rng=rng)
    assert A != B
    img = torch.from_numpy(C.random_bytes((4, 61, 167, 3), 41)).to(DEV)
    eager = [geom(img, [dict(), dict()], params=t).clone() for t in (A, B)]
    assert not torch.equal(eager[0], eager[1])
    geom.upload(A)                                        # n: two images per sample, as in the last forward
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        out = geom(img, [dict(), dict()])
        with pytest.raises(RuntimeError, match='capturing'):
            geom.upload(A)
        with pytest.raises(RuntimeError, match='takes no params'):
            geom(img, [dict(), dict()], params=A)
    for t, want in ((A, eager[0]), (B, eager[1])):
        geom.upload(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ---------------------------------------------------------------- the chain into the front end
def test_chain_into_the_front_end(g17):
    """front(geom(raw)) in eval mode equals front applied to the restatement's uint8 image; the metas after the chain hold the
    reference's recorded lidar2img and the front end's shapes."""
    conf = 'no_flip'
    raw = g17[conf + '_img']
    geom = ImageGeometry(C.G17_CONFS[conf], training=False)
    front = ImageFrontEnd.from_data_aug(F.DATA_AUG).eval()
    metas = [dict(lidar2img=[m.copy() for m in g17[conf + '_l2i'].numpy()])]
    got = front(geom(raw.to(DEV), metas), metas)
    p, = geom.draw(1)
    ref_metas = [dict()]
    want = front(restated(raw.numpy(), p).to(DEV), ref_metas)
    assert torch.equal(got, want) and got.shape == (2, 3, 32, 32)
    assert torch.equal(want[:, :, :16, :30].cpu(), ((g17[conf + '_eval_out'].permute(0, 3, 1, 2).float()[:, [2, 1, 0]]
                                                       - torch.tensor(F.MEAN).view(1, 3, 1, 1)) / torch.tensor(F.STD).view(1, 3, 1, 1)))
    assert np.array_equal(np.stack(metas[0]['lidar2img']), g17[conf + '_eval_l2i_after'].numpy())
    for key in ('img_shape', 'ori_shape', 'pad_shape', 'input_shape'):
        assert metas[0][key] == ref_metas[0][key], key
    assert metas[0]['ori_shape'] == [(16, 30, 3)] * 2 and metas[0]['pad_shape'] == [(32, 32, 3)] * 2


# ---------------------------------------------------------------- offsets beyond 2^31
def test_source_offsets_beyond_32_bits():
    """500 frames of 900 x 1600 x 3 are 2.16e9 bytes: the last two frames start beyond 2^31."""
    n, H, W = 500, 900, 1600
    assert (n - 2) * H * W * 3 > 2 ** 31
    conf = dict(C.R50_CONF, final_dim=(20, 70))
    geom = ImageGeometry(conf)
    g = torch.Generator(device=DEV).manual_seed(5)
    img = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=DEV, generator=g)
    p = GeomParams(0.44, (704, 396), (301, 203, 371, 223), True)
    got = geom(img, [dict()], params=[p]).cpu()
    for i in (0, n - 2, n - 1):
        want = restated(img[i:i + 1].cpu().numpy(), p)
        assert torch.equal(got[i:i + 1], want), (i, differing(got[i:i + 1], want))


# ---------------------------------------------------------------- refusals that need the device
def test_device_side_refusals():
    geom = ImageGeometry(C.G17_CONFS['r50_small'])
    img = torch.zeros(2, 36, 64, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError, match='uint8'):
        geom(img.float(), [dict()])
    with pytest.raises(ValueError, match='HWC'):
        geom(img.permute(0, 3, 1, 2).contiguous(), [dict()])
    with pytest.raises(ValueError, match='HWC'):
        geom(img[:, :35], [dict()])
    with pytest.raises(ValueError, match='contiguous'):
        geom(torch.zeros(2, 36, 64, 6, dtype=torch.uint8, device=DEV)[..., ::2], [dict()])
    with pytest.raises(ValueError, match='params for 1 samples'):
        geom(img, [dict()], params=geom.draw(2))
    with pytest.raises(ValueError, match='out must be'):
        geom(img, [dict()], out=torch.zeros(2, 3, 10, 30, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        geom(img.cpu(), [dict()])
