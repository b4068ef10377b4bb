"""sbev_resnet_repack (csrc/resnet_repack.hip): both weight images of the backbone by one launch, compared BYTE for byte with what the two
existing entries write on the same tensors (resnet.pack_layers, resnet.pack_layers_bwd: the eager path).  Both destinations are prefilled
with 0xFF and followed by a 4 KB guard of 0xA5 that must come back untouched; the comparison is of bytes, so a NaN pattern counts too."""
import ctypes

import pytest
import torch

from sparsebev_amd import _lib, resnet as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-5
GUARD = 4096


def conv_shapes(blocks, base=64):
    out = [(3, base, 7)]
    cin = base
    for s, nb in enumerate(blocks):
        mid = base << s
        for b in range(nb):
            out += [(cin, mid, 1), (mid, mid, 3)] + ([(cin, 4 * mid, 1)] if b == 0 else []) + [(mid, 4 * mid, 1)]
            cin = 4 * mid
    return out


def make_layers(blocks, dtype, seed):
    """(w, gamma, beta, mean, var) per convolution, with the fold's edge cases planted in every layer: gamma negative and zero, var down
    to 1e-12 (s up to ~316 gamma), weights whose w' is an fp16 subnormal, rounds to zero, overflows to +-inf, and a NaN"""
    g = torch.Generator().manual_seed(seed)
    layers = []
    for cin, cout, k in conv_shapes(blocks):
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        gamma = torch.rand(cout, generator=g) + 0.5
        gamma[1::7] *= -1.0
        gamma[3::11] = 0.0
        var = torch.rand(cout, generator=g) + 0.25
        var[2::13] = 1e-12
        var[5::17] = 0.0
        flat = w.view(cout, -1)
        flat[:, 0] = 3e-6           # w' an fp16 subnormal (and, times a small s, zero)
        flat[:, 1] = -2e-8
        flat[0::5, 2] = 7e4         # w' = +-inf in fp16 wherever |s| >= 1
        flat[0::5, 3] = -300.0      # x 316: beyond 65504 only where var is tiny
        flat[4, 4] = float('nan')
        layers.append(tuple(t.to(DEV).contiguous() for t in (w.to(dtype), gamma, torch.randn(cout, generator=g), torch.randn(cout, generator=g), var)))
    return layers


def reference(layers, blocks, fts):
    """the existing entries on the same tensors: (forward image, backward image or None)"""
    fwd = R.pack_layers(layers, EPS)[0]
    if fts > len(blocks):
        return fwd, None
    bp = R.backward_plan(50, 1, 32, 32, stage_blocks=blocks, first_trainable_stage=fts)
    order = sorted((l['pack_offset'], i) for i, l in enumerate(bp['layers']) if l['pack_offset'] >= 0)
    todo = [(layers[i - 1][0], layers[i - 1][1], layers[i - 1][4]) for _, i in order]
    bwd, offs = R.pack_layers_bwd(todo, EPS)
    assert offs == [o for o, _ in order] and bwd.numel() == bp['pack_bytes']
    return fwd, bwd


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = 0xA5
    return buf


def plan_and_table(layers, blocks, fts):
    p = R.repack_plan(50, [tuple(t.data_ptr() for t in l) for l in layers], layers[0][0].dtype, stage_blocks=blocks, first_trainable_stage=fts)
    return p, torch.tensor(p['table'], dtype=torch.int64).to(DEV)


def check(fwd_buf, bwd_buf, p, ref_fwd, ref_bwd):
    nf, nb = p['pack_bytes'], p['pack_bwd_bytes']
    assert nf == ref_fwd.numel() and nb == (0 if ref_bwd is None else ref_bwd.numel())
    assert torch.equal(fwd_buf[:nf], ref_fwd.view(torch.uint8)[:nf])
    assert bool((fwd_buf[nf:] == 0xA5).all())
    if ref_bwd is not None:
        assert torch.equal(bwd_buf[:nb], ref_bwd.view(torch.uint8)[:nb])
    assert bool((bwd_buf[nb:] == 0xA5).all())


_LAYERS = {}


def layers_of(blocks, dtype):
    key = (blocks, dtype)
    if key not in _LAYERS:
        _LAYERS[key] = make_layers(blocks, dtype, seed=len(_LAYERS) + 1)
    return _LAYERS[key]


@pytest.mark.parametrize('fts', [1, 2, 4, 5])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('blocks', [(1, 1, 1, 1), (1, 2, 2, 1)], ids=['1111', '1221'])
def test_both_images_equal_the_existing_entries(blocks, dtype, fts):
    layers = layers_of(blocks, dtype)
    ref_fwd, ref_bwd = reference(layers, blocks, fts)
    # the planted edge cases reach the image: infinities, NaN, subnormals (as fp16 bit patterns of the first layer behind the stem)
    halves = ref_fwd.view(torch.int16)[:1 << 20].to(torch.int32) & 0x7FFF
    assert bool((halves == 0x7C00).any()) and bool((halves > 0x7C00).any()) and bool(((halves > 0) & (halves < 0x0400)).any())
    p, table = plan_and_table(layers, blocks, fts)
    fwd_buf, bwd_buf = guarded(p['pack_bytes']), guarded(p['pack_bwd_bytes'])
    R.repack(table, fwd_buf, bwd_buf if ref_bwd is not None else None, EPS)
    torch.cuda.synchronize()
    check(fwd_buf, bwd_buf, p, ref_fwd, ref_bwd)
    if ref_bwd is None:          # nothing trains: the launch wrote the forward image only
        assert p['pack_bwd_bytes'] == 0 and bool((bwd_buf == 0xA5).all())


def test_resnet50_once():
    blocks = R.STAGE_BLOCKS[50]
    layers = make_layers(blocks, torch.float32, seed=50)
    assert len(layers) == 53
    ref_fwd, ref_bwd = reference(layers, blocks, 2)
    p, table = plan_and_table(layers, blocks, 2)
    fwd_buf, bwd_buf = guarded(p['pack_bytes']), guarded(p['pack_bwd_bytes'])
    R.repack(table, fwd_buf, bwd_buf, EPS)
    torch.cuda.synchronize()
    check(fwd_buf, bwd_buf, p, ref_fwd, ref_bwd)


def test_capture_one_kernel_node_and_replay_on_new_weights():
    """the launch takes no host array, so it records: ONE kernel node; after the weights and statistics were overwritten IN PLACE a replay
    writes the images of the new values"""
    blocks = (1, 2, 2, 1)
    layers = [tuple(t.clone() for t in l) for l in layers_of(blocks, torch.float32)]
    p, table = plan_and_table(layers, blocks, 2)
    fwd_buf, bwd_buf = guarded(p['pack_bytes']), guarded(p['pack_bwd_bytes'])
    lib = _lib.load()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    handle = ctypes.c_void_p()
    with torch.cuda.stream(side):
        sp = ctypes.c_void_p(side.cuda_stream)
        _lib.check(lib.sbev_capture_begin(sp), 'sbev_capture_begin')
        try:
            R.repack(table, fwd_buf, bwd_buf, EPS)
        finally:
            st = lib.sbev_capture_end(sp, ctypes.byref(handle))
        _lib.check(st, 'sbev_capture_end')
    torch.cuda.current_stream().wait_stream(side)
    try:
        assert lib.sbev_graph_num_nodes(handle) == 1
        assert bool((fwd_buf[:p['pack_bytes']] == 0xFF).all())          # a capture executes nothing
        g = torch.Generator().manual_seed(77)
        for l in layers:
            for j, t in enumerate(l):
                new = torch.rand(t.shape, generator=g) + 0.1 if j == 4 else torch.randn(t.shape, generator=g) * (0.05 if j == 0 else 1.0)
                t.copy_(new.to(DEV))
        ref_fwd, ref_bwd = reference(layers, blocks, 2)
        _lib.check(lib.sbev_graph_launch(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_graph_launch')
        torch.cuda.synchronize()
    finally:
        lib.sbev_graph_destroy(handle)
    check(fwd_buf, bwd_buf, p, ref_fwd, ref_bwd)
