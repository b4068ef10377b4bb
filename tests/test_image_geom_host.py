"""The image geometry's host side, without a GPU: sbev_image_geom_plan's tables against the numpy restatement of Pillow's resampler
(tests/image_geom_cases.py), the restatement against the reference's recording (fixture G17) and against a live Pillow where it imports,
``draw`` / ``ida_mat`` / the ``lidar2img`` update against G17, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import image_geom_cases as C
from conftest import load_golden
from sparsebev_amd import _lib, image_geom
from sparsebev_amd.image_geom import GeomParams, ImageGeometry


@pytest.fixture(scope='module')
def g17():
    return load_golden('g17_image_geom')


def np_(v):
    return v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


# ---------------------------------------------------------------- plan == restatement
@pytest.mark.parametrize('c', C.CASES + [C.FULL_EVAL, C.FULL_038], ids=lambda c: c['name'])
def test_plan_tables_equal_the_restatement(c):
    p, block = image_geom.plan(c['H'], c['W'], c['fH'], c['fW'], c['resize_dims'], c['crop'][:2], c['flip'], table=True)
    header, xb, yb, xk, yk = image_geom.split_block(block, c['fH'], c['fW'])
    want = C.tables(c['H'], c['W'], c['resize_dims'], c['crop'])
    for name, got, ref in zip(('column bounds', 'row bounds', 'column coefficients', 'row coefficients'), (xb, yb, xk, yk), want):
        assert np.array_equal(got, ref), name
    ks = (C.ksize_of(c['W'], c['resize_dims'][0]), C.ksize_of(c['H'], c['resize_dims'][1]))
    assert header.tolist() == [*c['resize_dims'], c['crop'][0], c['crop'][1], int(c['flip']), *ks, 0]
    assert (p.ksize_x, p.ksize_y) == ks and (p.tile_w, p.tile_h) == (C.TILE_W, C.TILE_H)
    assert p.block_bytes == block.nbytes and p.block_bytes % 16 == 0
    assert p.workgroups == -(-c['fW'] // C.TILE_W) * -(-c['fH'] // C.TILE_H)
    # the sizes-only call agrees, and the taps never leave the source
    q = image_geom.plan(c['H'], c['W'], c['fH'], c['fW'], c['resize_dims'], c['crop'][:2], c['flip'])
    assert q[:4] == p[:4] and q.src_bytes == 0
    assert (xb[:, 0] >= 0).all() and (xb.sum(1) <= c['W']).all() and (yb[:, 0] >= 0).all() and (yb.sum(1) <= c['H']).all()
    assert xb[:, 1].max() <= ks[0] and yb[:, 1].max() <= ks[1]


def test_case_list_is_what_it_says():
    by = {c['name']: c for c in C.CASES}
    assert (C.ksize_of(53, by['down_041']['resize_dims'][0]), C.ksize_of(37, by['down_041']['resize_dims'][1])) == (13, 11)
    _, xb, yb, xk, yk = image_geom.split_block(image_geom.plan(33, 47, 22, 31, (47, 33), (5, 7), table=True)[1], 22, 31)
    for k in (xk, yk):                                    # factor 1.0: the identity, 2^22 on one tap
        assert ((k != 0).sum(1) == 1).all() and (k.max(1) == 1 << 22).all()
    assert C.ksize_of(23, by['enlarge_13']['resize_dims'][1]) == 5
    xb = C.tables(30, 60, (34, 17), (0, 1, 45, 14))[0]
    assert (xb[34:, 1] == 0).all() and len(xb[34:]) == 11 and (xb[:34, 1] > 0).all()
    _, yb = C.tables(30, 60, (34, 17), (4, -5, 30, 15))[:2]
    assert (yb[:5, 1] == 0).all() and (yb[5:, 1] > 0).all()
    assert C.ksize_of(1600, 608) == 13 and C.ksize_of(1600, 704) == 11


# ---------------------------------------------------------------- restatement == the reference's recording == Pillow
@pytest.mark.parametrize('conf,call', C.G17_KEYS, ids=lambda v: str(v))
def test_restatement_equals_the_recording(g17, conf, call):
    _, dims, crop, flip, _ = C.g17_params(g17, conf, call)
    img, want = np_(g17[conf + '_img']), np_(g17['%s_%s_out' % (conf, call)])
    for v in range(C.G17_VIEWS):
        assert np.array_equal(C.transform(img[v], dims, crop, flip), want[v].transpose(2, 0, 1)), v


def pillow(img, c):
    Image = pytest.importorskip('PIL.Image')
    im = Image.fromarray(img).resize(c['resize_dims']).crop(c['crop'])
    if c['flip']:
        im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
    return np.ascontiguousarray(np.array(im).transpose(2, 0, 1))


@pytest.mark.parametrize('c', C.CASES + [C.FULL_EVAL, C.FULL_038], ids=lambda c: c['name'])
def test_restatement_equals_live_pillow(c):
    pytest.importorskip('PIL')
    for gen in (C.random_bytes, C.extremes):
        img = gen((c['H'], c['W'], 3), 7)
        assert np.array_equal(C.transform(img, c['resize_dims'], c['crop'], c['flip']), pillow(img, c)), gen.__name__


def test_extremes_drive_both_clamps():
    """on the 0 / 255 pattern the unclamped horizontal sums leave [0, 255] on both sides"""
    img = C.extremes((37, 53, 3), 7).astype(np.int64)
    b, k = C.coeffs(53, 21)
    lo = hi = 0
    for xx, (first, count) in enumerate(b):
        acc = (1 << 21) + sum(img[:, first + t] * int(k[xx, t]) for t in range(count))
        lo, hi = min(lo, int((acc >> 22).min())), max(hi, int((acc >> 22).max()))
    assert lo < 0 and hi > 255


# ---------------------------------------------------------------- draw, ida_mat, metas
@pytest.mark.parametrize('conf', list(C.G17_CONFS))
def test_draw_reproduces_the_recorded_tuples(g17, conf):
    geom = ImageGeometry(C.G17_CONFS[conf], training=True)
    for call in C.G17_CALLS:
        want = C.g17_params(g17, conf, call)
        if call == 'eval':
            state = np.random.get_state()[1].copy()
            p, = geom.eval().draw(1)
            assert np.array_equal(np.random.get_state()[1], state)           # the deterministic branch draws nothing
            geom.train()
        else:
            np.random.seed(int(call[5:]))
            p, = geom.draw(1)
            q, = geom.draw(1, rng=np.random.RandomState(int(call[5:])))
            assert p == q
        assert (p.resize, p.resize_dims, p.crop, p.flip, p.rotate) == want, call
    # several samples continue the same stream, one transform each
    np.random.seed(1)
    a, b = geom.draw(2)
    np.random.seed(1)
    assert (a, b) == (geom.draw(1)[0], geom.draw(1)[0]) and a != b


def test_rand_flip_off_draws_one_number_fewer():
    conf = dict(C.G17_CONFS['r50_small'], rand_flip=False)
    rng = np.random.RandomState(5)
    p, = ImageGeometry(conf).draw(1, rng=rng)
    ref = np.random.RandomState(5)
    resize, _, _, rot = ref.uniform(*conf['resize_lim']), ref.uniform(0, 0), ref.uniform(0, 1), ref.uniform(0, 0)
    assert p.resize == resize and p.flip is False
    assert rng.uniform() == ref.uniform()                 # four draws, no choice()
    rng, ref = np.random.RandomState(5), np.random.RandomState(5)
    ImageGeometry(C.G17_CONFS['r50_small']).draw(1, rng=rng)
    [ref.uniform() for _ in range(3)], ref.choice([0, 1]), ref.uniform()
    assert rng.uniform() == ref.uniform()


@pytest.mark.parametrize('conf,call', C.G17_KEYS, ids=lambda v: str(v))
def test_ida_mat_and_lidar2img_equal_the_recording(g17, conf, call):
    geom = ImageGeometry(C.G17_CONFS[conf], training=call != 'eval')
    p = GeomParams(*C.g17_params(g17, conf, call))
    mat = geom.ida_mat(p)
    assert mat.dtype == np.float32 and np.array_equal(mat, np_(g17['%s_%s_ida' % (conf, call)]))
    for key, dtype in (('l2i_after', np.float64), ('l2i32_after', np.float32)):
        metas = [dict(lidar2img=[m.astype(dtype) for m in np_(g17[conf + '_l2i'])], box_type_3d='x')]
        geom.update_metas(metas, [p], views=C.G17_VIEWS)
        got, want = np.stack(metas[0]['lidar2img']), np_(g17['%s_%s_%s' % (conf, call, key)])
        assert got.dtype == want.dtype == dtype and np.array_equal(got, want)
        shapes = [tuple(s) for s in np_(g17['%s_%s_shapes' % (conf, call)]).tolist()]
        assert metas[0]['img_shape'] == metas[0]['ori_shape'] == metas[0]['pad_shape'] == shapes and metas[0]['box_type_3d'] == 'x'


# ---------------------------------------------------------------- the table
def test_table_maps_each_image_to_its_sample():
    geom = ImageGeometry(C.G17_CONFS['r50_small'])
    params = geom.draw(2, rng=np.random.RandomState(0))
    t = geom.table(params, 6)
    assert t.dtype == np.int32 and t[:8].tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
    blocks = [image_geom.plan(36, 64, 10, 30, p.resize_dims, p.crop[:2], p.flip, table=True)[1] for p in params]
    assert np.array_equal(t[8:], np.concatenate(blocks))
    with pytest.raises(ValueError, match='do not divide'):
        geom.table(params, 5)


# ---------------------------------------------------------------- refusals
def test_rotation_is_refused():
    conf = dict(C.G17_CONFS['r50_small'], rot_lim=(-5.4, 5.4))
    with pytest.raises(NotImplementedError, match='rotation'):
        ImageGeometry(conf).draw(1, rng=np.random.RandomState(0))
    geom = ImageGeometry(C.G17_CONFS['r50_small'])
    p = GeomParams(0.5, (32, 18), (0, 8, 30, 18), False, 3.0)
    for f in (geom.ida_mat, lambda q: geom.table([q], 1)):
        with pytest.raises(NotImplementedError, match='rotation'):
            f(p)


def test_too_many_taps_are_refused_not_truncated():
    with pytest.raises(_lib.SbevError, match='filter taps, above the capacity SBEV_GEOM_KMAX = 16'):
        image_geom.plan(900, 1600, 256, 704, (320, 180), (0, 0))                  # factor 0.2: ksize 21
    geom = ImageGeometry(dict(C.R50_CONF, resize_lim=(0.2, 0.2), final_dim=(64, 64)))
    with pytest.raises(_lib.SbevError, match='filter taps'):
        geom.table(geom.draw(1, rng=np.random.RandomState(0)), 1)
    assert image_geom.plan(900, 1600, 256, 704, (458, 258), (0, 0)).ksize_x == 15           # just inside
    with pytest.raises(_lib.SbevError):
        image_geom.plan(900, 1600, 256, 704, (457, 257), (0, 0))                  # 1600 / 457 > 3.5: 17 taps


def test_c_entry_refusals_without_gpu():
    lib = _lib.load()
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    base = dict(src=0x1000, dst=0x2000, n=2, H=8, W=8, fH=4, fW=4, table=0x3000, rows=0x4000, nt=1)

    def call(**o):
        d = dict(base, **o)
        st = lib.sbev_image_geom(vp(d['src']), vp(d['dst']), d['n'], d['H'], d['W'], d['fH'], d['fW'], vp(d['table']), vp(d['rows']), d['nt'], None)
        return st, (lib.sbev_last_error().decode() if st else '')

    for overrides, text in [
        (dict(src=None), 'null pointer'), (dict(dst=None), 'null pointer'), (dict(table=None), 'null pointer'), (dict(rows=None), 'null pointer'),
        (dict(n=0), 'n and n_transforms must be >= 1'), (dict(nt=0), 'n and n_transforms must be >= 1'),
        (dict(H=0), 'must be >= 1'), (dict(W=-3), 'must be >= 1'), (dict(fH=0), 'must be >= 1'), (dict(fW=0), 'must be >= 1'),
        (dict(W=1 << 22), 'above 2^22 - 1'),
        (dict(table=0x3008), 'not 16-byte aligned'), (dict(rows=0x4002), '4-byte aligned'), (dict(src=0x1001), 'src is not 4-byte aligned'),
        (dict(n=1 << 30, fH=1 << 12, fW=1 << 12), 'too many for one launch'),
    ]:
        st, err = call(**overrides)
        assert st == -1 and err.startswith('sbev_image_geom: ') and text in err, (overrides, st, err)

    out = (ctypes.c_int64 * 8)()
    plan = lambda *a: lib.sbev_image_geom_plan(*a)
    assert plan(8, 8, 4, 4, 4, 4, 0, 0, 0, None, None) == -1 and b'null out' in lib.sbev_last_error()
    assert plan(0, 8, 4, 4, 4, 4, 0, 0, 0, None, out) == -1 and b'sbev_image_geom_plan: H, W, fH, fW must be >= 1' in lib.sbev_last_error()
    assert plan(8, 8, 4, 4, 0, 4, 0, 0, 0, None, out) == -1 and b'resize to 0 x 4' in lib.sbev_last_error()
    assert plan(8, 8, 4, 4, 4, 4, 1 << 23, 0, 0, None, out) == -1 and b'crop origin' in lib.sbev_last_error()
    assert plan(80, 80, 4, 4, 8, 8, 0, 0, 0, None, out) == -1 and b'filter taps' in lib.sbev_last_error()
    assert plan(8, 8, 4, 4, 4, 4, 0, 0, 0, None, out) == 0 and out[0] > 0 and out[1] == 1


def test_host_side_input_refusals():
    geom = ImageGeometry(C.G17_CONFS['r50_small'])
    raw = torch.zeros(2, 36, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        geom(raw, [dict()])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        geom.upload(geom.draw(1), device='cpu')
    with pytest.raises(TypeError, match='uint8'):
        geom(raw.float(), [dict()])
    with pytest.raises(ValueError, match='HWC'):
        geom(raw.permute(0, 3, 1, 2).contiguous(), [dict()])                    # CHW is not what the decoder hands over


def test_exports():
    import sparsebev_amd
    assert sparsebev_amd.ImageGeometry is ImageGeometry and 'ImageGeometry' in sparsebev_amd.__all__
    assert 'sbev_image_geom' in _lib.SIGNATURES and 'sbev_image_geom_plan' in _lib.SIGNATURES
    assert image_geom.KMAX == C.KMAX == 16
