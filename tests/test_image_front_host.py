"""The image front end's host side, without a GPU: ``draw`` against the random-call log of the reference (fixture G16), the plan
against pad_multiple's arithmetic, the refusals of sbev_image_front (all returned before any launch), the meta updates, and the
numpy restatement of tests/image_front_cases.py against the fixture's fp64 record."""
import ctypes

import numpy as np
import pytest
import torch

import image_front_cases as C
from conftest import load_golden
from sparsebev_amd import _lib, image_front
from sparsebev_amd.image_front import ImageFrontEnd


@pytest.fixture(scope='module')
def g16():
    return load_golden('g16_image_front')


class LoggedState:
    """a RandomState whose calls are written down like the fixture's log"""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def _call(self, name, *a):
        v = getattr(self.rs, name)(*a)
        self.log.append((name, np.atleast_1d(np.asarray(v, dtype=np.float64))))
        return v

    def randint(self, *a):
        return self._call('randint', *a)

    def uniform(self, *a):
        return self._call('uniform', *a)

    def permutation(self, *a):
        return self._call('permutation', *a)

    def rand(self):
        return self._call('rand')


def front(training, **kw):
    f = ImageFrontEnd.from_data_aug(C.DATA_AUG, **kw)
    return f.train(training)


def drawn(g16, call, rng=None):
    i = C.G16_CALLS.index(call)
    n, _, H, W = C.G16_SHAPES[call]
    Hp, _ = C.padded(H, W, 32)
    f = front(C.G16_TRAINING[call])
    if rng is None:
        np.random.seed(int(g16['seeds'][i]))
        return f.draw(n, Hp)
    return f.draw(n, Hp, rng=rng)


@pytest.mark.parametrize('call', C.G16_CALLS)
def test_draw_reproduces_the_reference_random_log(g16, call):
    rng = LoggedState(int(g16['seeds'][C.G16_CALLS.index(call)]))
    drawn(g16, call, rng)
    names, vals = [str(s) for s in g16[call + '_log_name']], g16[call + '_log_val'].numpy()
    assert [k for k, _ in rng.log] == names
    for (k, v), want in zip(rng.log, vals):
        assert np.array_equal(v, want[:len(v)]) and np.isnan(want[len(v):]).all(), (k, v, want)
    if call == 'eval':
        assert names == ['rand']                         # consumed although no mask is applied
    # and the global generator, which the reference uses, gives the same parameters
    assert np.array_equal(drawn(g16, call).table(), drawn(g16, call, np.random.RandomState(int(g16['seeds'][C.G16_CALLS.index(call)]))).table())


def test_fixture_takes_every_branch(g16):
    a, b = drawn(g16, 'train_a'), drawn(g16, 'train_b')
    flags = np.concatenate([a.flags, b.flags])
    mode = np.concatenate([a.mode, b.mode])
    for bit in (C.BRIGHT, C.SAT, C.HUE, C.SWAP):
        assert (flags & bit).any() and not (flags & bit).all()
    assert ((flags & C.CONTRAST) != 0)[mode == 0].any() and ((flags & C.CONTRAST) != 0)[mode == 1].any()
    perm = np.concatenate([a.perm, b.perm])[(flags & C.SWAP) != 0]
    assert (perm != np.arange(3)).any()
    assert sorted([int(a.mask[0, 0]), int(b.mask[0, 0])]) == [0, 1]           # GridMask applied in one call, skipped in the other
    assert not drawn(g16, 'eval').mask.any() and not drawn(g16, 'eval').flags.any()


def test_table_layout():
    p = image_front.FrontParams(2)
    assert p.table().shape == (128,) and image_front.ROW_DTYPE.itemsize == 64
    p.flags[1], p.mode[1], p.delta[1], p.alpha[1], p.sat[1], p.hue[1] = 31, 1, 1.5, 0.75, 1.25, -18.0
    p.perm[1] = (2, 0, 1)
    p.mask[1] = (1, 9, 4, 3, 2)
    words = p.table()[64:].view(np.int32)
    assert list(words[[0, 1, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]]) == [31, 1, 2, 0, 1, 1, 9, 4, 3, 2, 0, 0]
    assert list(p.table()[64:].view(np.float32)[2:6]) == [1.5, 0.75, 1.25, -18.0]
    fresh = p.table()[:64]
    assert list(fresh.view(np.int32)[[0, 1, 6, 7, 8, 9]]) == [0, 0, 0, 1, 2, 0]


@pytest.mark.parametrize('div', [1, 32])
def test_plan_is_pad_multiple_arithmetic(div):
    for H in (1, 31, 32, 33, 37, 45, 64):
        for W in (1, 31, 32, 33, 37, 45, 64):
            pad_h = 0 if H % div == 0 else div - H % div
            pad_w = 0 if W % div == 0 else div - W % div
            Hp, Wp, elems, table_bytes, grid = image_front.plan(5, H, W, div)
            assert (Hp, Wp) == (H + pad_h, W + pad_w) == C.padded(H, W, div)
            assert elems == 5 * 3 * Hp * Wp and table_bytes == 5 * 64
            assert grid == 5 * -(-(Hp * -(-Wp // 16)) // 256)                # 16 pixels per lane, 256 lanes, whole workgroups per image


def test_refusals_without_gpu():
    lib = _lib.load()
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    base = dict(src=0x1000, sdt=3, dst=0x2000, ddt=0, n=2, H=8, W=8, div=32, mean=f3(0, 0, 0), std=f3(1, 1, 1), to_rgb=1, colour=0, table=0x3000)
    vp = lambda v: None if v is None else ctypes.c_void_p(v)

    def call(**o):
        d = dict(base, **o)
        st = lib.sbev_image_front(vp(d['src']), d['sdt'], vp(d['dst']), d['ddt'], d['n'], d['H'], d['W'], d['div'], d['mean'], d['std'],
                                  d['to_rgb'], d['colour'], vp(d['table']), None)
        return st, (lib.sbev_last_error().decode() if st else '')

    table = [
        (dict(src=None), 'null pointer'), (dict(dst=None), 'null pointer'), (dict(mean=None), 'null pointer'), (dict(std=None), 'null pointer'),
        (dict(n=0), 'n, H, W must be >= 1'), (dict(H=0), 'n, H, W must be >= 1'), (dict(W=-1), 'n, H, W must be >= 1'),
        (dict(div=0), 'size divisor 0 < 1'),
        (dict(sdt=1), 'src_dtype 1'), (dict(sdt=2), 'src_dtype 2'), (dict(sdt=4), 'src_dtype 4'),
        (dict(ddt=1), 'dst_dtype 1'), (dict(ddt=3), 'dst_dtype 3'), (dict(ddt=-1), 'dst_dtype -1'),
        (dict(std=f3(1, 0, 1)), 'std[1] is 0'),
        (dict(table=0x3008), 'the table is not 16-byte aligned'),
        (dict(table=None, colour=1), 'colour_on needs a table'),
        (dict(sdt=0, src=0x1002), 'not aligned to their element size'), (dict(ddt=2, dst=0x2001), 'not aligned to their element size'),
        (dict(H=1 << 29, W=1 << 29, div=1), 'too many for one launch'), (dict(H=1 << 30, div=1), 'too large'),
    ]
    for overrides, text in table:
        st, err = call(**overrides)
        assert st == -1 and err.startswith('sbev_image_front: ') and text in err, (overrides, st, err)
    out = (ctypes.c_int64 * 5)()
    assert lib.sbev_image_front_plan(1, 1, 1, 0, out) == -1 and b'sbev_image_front_plan: size divisor' in lib.sbev_last_error()
    assert lib.sbev_image_front_plan(1, 1, 1, 1, None) == -1
    assert lib.sbev_image_front_plan(0, 1, 1, 1, out) == -1


@pytest.mark.parametrize('call', C.G16_CALLS)
def test_meta_updates_match_the_reference(g16, call):
    n, _, H, W = C.G16_SHAPES[call]
    N = C.G16_VIEWS[call]
    B = n // N
    metas = [dict(ori_shape=[(900, 1600, 3)] * N, box_type_3d='x') for _ in range(B)]
    assert image_front.update_metas(metas, B, N, H, W, 32) == C.padded(H, W, 32)
    for key in ('img_shape', 'ori_shape', 'pad_shape'):
        want = g16[call + '_meta_' + key].tolist()
        got = [m[key] for m in metas]
        assert all(isinstance(m[key], list) and all(isinstance(s, tuple) for s in m[key]) for m in metas)
        assert [[list(s) for s in per] for per in got] == want, key
    for m in metas:
        assert isinstance(m['input_shape'], torch.Size) and list(m['input_shape']) == g16[call + '_meta_input_shape'].tolist()
        assert m['box_type_3d'] == 'x'
    # without an img_pad_cfg nothing is padded and pad_shape is not written
    metas = [dict() for _ in range(B)]
    assert image_front.update_metas(metas, B, N, H, W, None) == (H, W)
    assert 'pad_shape' not in metas[0] and metas[0]['img_shape'] == [(H, W, 3)] * N and tuple(metas[0]['input_shape']) == (H, W)


def test_cpu_tensors_raise():
    f = front(False)
    with pytest.raises(RuntimeError, match='device tensors'):
        f(torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), [dict()])


def test_exports():
    import sparsebev_amd
    assert sparsebev_amd.ImageFrontEnd is ImageFrontEnd and 'ImageFrontEnd' in sparsebev_amd.__all__
    assert 'sbev_image_front' in _lib.SIGNATURES and 'sbev_image_front_plan' in _lib.SIGNATURES
    assert image_front.ROW_BYTES == 64


@pytest.mark.parametrize('call', C.G16_CALLS)
def test_restatement_agrees_with_the_fp64_record(g16, call):
    """tests/image_front_cases.py::pipeline_f64 with the drawn (fp32-rounded) parameters against the reference's fp64 run.  The record
    used the unrounded draws: delta and hue differ by up to 2^-24 * 32 = 2e-6, alpha and sat by 2^-24 * 1.5 relative to values of up
    to ~400 (4e-5 before the division by std ~ 57): 1e-5 after it, with the fixture's own 1e-8 quantisation."""
    p = drawn(g16, call)
    img = g16[call + '_img'].numpy()
    ref = g16[call + '_out'].numpy().astype(np.float64) + g16[call + '_d64'].numpy().astype(np.float64) / 2.0 ** 20
    got = C.pipeline_f64(img, C.MEAN, C.STD, True, 32, rows=p.rows, colour=C.G16_TRAINING[call])
    assert got.shape == ref.shape
    err = np.abs(got - ref).max()
    print('restatement vs fp64 record (%s): %.3g' % (call, err))
    assert err < 1e-5
