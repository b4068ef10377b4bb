"""sbev_resnet_repack_plan (csrc/resnet_repack.hip) is a pure host function: its table is checked here, on fake aligned pointers, against
the offsets the two existing pack entries use -- the running sum of resnet.pack_layers and sbev_resnet_backward_plan's pack_offset.  No
GPU: nothing is ever read through a pointer."""
import ctypes

import pytest
import torch

from sparsebev_amd import _lib, resnet as R
import resnet_bwd_cases as BC


def conv_shapes(blocks, base=64):
    """(cin, cout, k) of every convolution in launch order"""
    out = [(3, base, 7)]
    cin = base
    for s, nb in enumerate(blocks):
        mid = base << s
        for b in range(nb):
            out += [(cin, mid, 1), (mid, mid, 3)] + ([(cin, 4 * mid, 1)] if b == 0 else []) + [(mid, 4 * mid, 1)]
            cin = 4 * mid
    return out


def fake_pointers(n, first=0x10000):
    """five distinct 256-byte aligned addresses per convolution"""
    return [tuple(first + 256 * (5 * i + j) for j in range(5)) for i in range(n)]


@pytest.mark.parametrize('blocks', [None, BC.HOST_BLOCKS])
@pytest.mark.parametrize('fts', [1, 2, 3, 4, 5])
def test_table_matches_the_existing_pack_offsets(blocks, fts):
    shapes = conv_shapes(R.STAGE_BLOCKS[50] if blocks is None else blocks)
    ptrs = fake_pointers(len(shapes))
    p = R.repack_plan(50, ptrs, torch.float32, stage_blocks=blocks, first_trainable_stage=fts)
    assert len(p['layers']) == len(shapes) and p['table'][0] == len(shapes)
    assert len(p['table']) == R.REPACK_HEAD + R.REPACK_LAYER_WORDS * len(shapes)
    # the forward image: pack_layers' running sum (fragments, then the fp32 bias, layer after layer)
    at = 0
    for l, (cin, cout, k), ptr in zip(p['layers'], shapes, ptrs):
        frag = (160 if k == 7 else k * k * cin) * cout * 2
        assert (l['w'], l['gamma'], l['beta'], l['mean'], l['var']) == ptr
        assert (l['cin'], l['cout'], l['taps']) == (cin, cout, k * k)
        assert l['offset'] == at and l['bias_offset'] == at + frag
        at += frag + 4 * cout
    fwd = R.plan(50, 1, 32, 32, stage_blocks=blocks)
    assert p['pack_bytes'] == at == fwd['pack_bytes']
    # the backward image: the backward plan's offsets (launch i is convolution i - 1 from the pool on); none at all for a frozen net
    if fts <= 4:
        bp = R.backward_plan(50, 1, 32, 32, stage_blocks=blocks, first_trainable_stage=fts)
        want = [bp['layers'][0]['pack_offset']] + [l['pack_offset'] for l in bp['layers'][2:]]
        assert [l['bwd_offset'] for l in p['layers']] == want
        assert p['pack_bwd_bytes'] == bp['pack_bytes'] > 0
        assert any(o >= 0 for o in want) and want[0] == -1
    else:
        assert all(l['bwd_offset'] == -1 for l in p['layers']) and p['pack_bwd_bytes'] == 0
    # the work items: 32 output channels x 64 reduction indices each; the prefix increases and ends at the grid
    first = [l['first_item'] for l in p['layers']]
    assert first[0] == 0 and all(a < b for a, b in zip(first, first[1:]))
    counts = [(cout // 32) * (3 if k == 7 else cin // 64) for cin, cout, k in shapes]
    assert [b - a for a, b in zip(first, first[1:] + [p['items']])] == counts
    assert p['table'][1] == p['items'] and p['table'][2] == p['pack_bytes'] and p['table'][3] == p['pack_bwd_bytes']


def test_fp16_weights_need_only_two_byte_alignment():
    shapes = conv_shapes((1, 1, 1, 1))
    ptrs = [(a + 2, b, c, d, e) for a, b, c, d, e in fake_pointers(len(shapes))]
    assert R.repack_plan(50, ptrs, torch.float16, stage_blocks=(1, 1, 1, 1))['table'][4] == 2
    with pytest.raises(_lib.SbevError, match='sbev_resnet_repack_plan: layer 0: misaligned tensor'):
        R.repack_plan(50, ptrs, torch.float32, stage_blocks=(1, 1, 1, 1))


def test_refusals_come_under_the_plans_own_name():
    lib = _lib.load()
    blocks = (1, 1, 1, 1)
    n = len(conv_shapes(blocks))
    good = fake_pointers(n)

    def call(ptrs=good, w_dtype=0, fts=2, depth=50, num_stages=4, table=True):
        cols = [(ctypes.c_void_p * n)(*[p[j] for p in ptrs]) for j in range(5)]
        tab, out = (ctypes.c_int64 * R.REPACK_WORDS)(), (ctypes.c_int64 * 4)()
        st = lib.sbev_resnet_repack_plan(depth, (ctypes.c_int32 * 4)(*blocks), num_stages, 64, fts, *cols, w_dtype, tab if table else None, out)
        return st, (lib.sbev_last_error().decode() if st else '')

    assert call() == (0, '')
    swap = lambda i, j, v: [tuple(v if (a, b) == (i, j) else x for b, x in enumerate(p)) for a, p in enumerate(good)]
    assert call(ptrs=swap(3, 0, None)) == (-1, 'sbev_resnet_repack_plan: layer 3: null pointer')
    assert call(ptrs=swap(n - 1, 4, None)) == (-1, 'sbev_resnet_repack_plan: layer %d: null pointer' % (n - 1))
    assert call(ptrs=swap(2, 0, good[2][0] + 2)) == (-1, 'sbev_resnet_repack_plan: layer 2: misaligned tensor')
    assert call(ptrs=swap(5, 2, good[5][2] + 1)) == (-1, 'sbev_resnet_repack_plan: layer 5: misaligned tensor')
    assert call(w_dtype=1) == (-1, 'sbev_resnet_repack_plan: w_dtype 1 (SBEV_F32 or SBEV_F16)')
    assert call(w_dtype=7)[0] == -1
    st, err = call(depth=34)
    assert st == -1 and err.startswith('sbev_resnet_repack_plan: depth=34 is a BasicBlock net')
    st, err = call(fts=0)
    assert st == -1 and err.startswith('sbev_resnet_repack_plan: first_trainable_stage=0')
    st, err = call(fts=6)
    assert st == -1 and err.startswith('sbev_resnet_repack_plan: first_trainable_stage=6 not in 1 .. num_stages')
    assert call(table=False) == (-1, 'sbev_resnet_repack_plan: null table / out')
    # the launch's own host checks, before any GPU call
    one = ctypes.c_void_p(0x1000)
    assert lib.sbev_resnet_repack(None, one, one, 1e-5, None) == -1 and lib.sbev_last_error() == b'sbev_resnet_repack: null pointer'
    assert lib.sbev_resnet_repack(one, ctypes.c_void_p(0x1008), one, 1e-5, None) == -1 and lib.sbev_last_error() == b'sbev_resnet_repack: 16-byte alignment'
    assert lib.sbev_resnet_repack(one, one, one, -1.0, None) == -1 and lib.sbev_last_error().startswith(b'sbev_resnet_repack: eps=')
