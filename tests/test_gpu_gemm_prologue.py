"""The prologues of the two big mixing GEMMs (csrc/gemm_bf16s.hip): what runs in front of the first MFMA.

Out-projection (gemm_bf16s_out4_kernel / gemm_bf16s_out8_kernel, X pre-split into fp16 pairs): the prologue stages k-steps 0 and 1 and
requests X of 2 and 3 and W of 0 and 1 for a loop whose waits are counted by hand.  (Entering the loop with X of 2 and 3 still in flight
was built and measured equal -- profiles/gemm_prologue.json -- and is not in; these cases were written for it and pin the prologue that
is.)  Checked on integers fp16 holds exactly -- every product and every partial sum is exact, so the result must be BIT-EQUAL to the
integer GEMM whatever the order -- at the shortest K-chunks the library plans (4, 5 and 6 k-steps per phase group of the 128-row kernel:
at and above the depth of the operand pipeline, clamped dummy requests past the end), with the unequal last step of the K-half split, at
1 .. 4 row fragments per tile on the 128-row kernel and at the 256-row kernel's own threshold.  (Fewer than 4 k-steps per phase group
cannot be reached: sbev_linear_bf16s_out_ok takes K >= 256 and a chunk has at least 8 k-steps.)

Generator (gemm_f16s_gen_ws_kernel) with the on-demand relayout's scan riding UNDER its weight load (lazy_relayout.hpp:
lazy_scan_share_under): the same step with the scan as a launch of its own (sbev_decoder_lazy_scan_launch(1)) must give the same
outputs, move the same units (NaN poison) and leave the same workspace behind, bit for bit -- the generated parameters among it."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

import linear_fwd_cases as C  # noqa: E402
from sparsebev_amd import _lib, dense, synthetic as S  # noqa: E402
from sparsebev_amd import transformer as TR  # noqa: E402
from sparsebev_amd.transformer import SparseBEVTransformer  # noqa: E402

DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'
N = 256
UP = 11           # X 2^11: |x| <= 3 -> fp16 hi exact, lo = 0

# K -> K // 128 chunks of the K / 16 k-steps, each walked as two K halves (128-row kernel; the second half multiplies zeros in the last
# step of an odd chunk) or whole by both row halves (256-row kernel):
#   256: 2 x 8 = halves 4 + 4     288: 2 x 9 = 5 + 4     320: 2 x 10 = 5 + 5     352: 2 x 11 = 6 + 5     416: 8, 9, 9 = 4 + 4, 5 + 4, 5 + 4
OUT_K = [256, 288, 320, 352, 416]


@pytest.mark.parametrize('K', OUT_K)
@pytest.mark.parametrize('M', [1, 33, 128, 129, 1025])
def test_out_projection_on_pairs_is_the_integer_gemm(M, K):
    lib = _lib.load()
    assert lib.sbev_linear_bf16s_out_plan(M, N, K) == K // 128, 'the chunk count this case was chosen for'
    C.assert_exact(C.int_bound(K), 'K=%d' % K)                  # (times 2^UP and a row's 2^e in the accumulators: powers of two, exact)
    x, w, b = C.rows(M, K, 'int'), C.weights(N, K, 'int'), C.vector(N, 'int')
    want = (C.product(M, N, K, 'int') + b.double()).float()
    wf, wsc = dense.pack_f16s_frags(w.to(DEV))
    pairs = dense.f16s_pairs(x.to(DEV), UP)
    prev = lib.sbev_linear_out8_min_rows(1024)                  # the library's own threshold: 1025 rows run on 256-row tiles
    try:
        y = dense.linear_splitk_f16s(pairs, wf, wsc, b.to(DEV), nprod=3, x_up_log2=UP, x_is_pairs=True)
    finally:
        lib.sbev_linear_out8_min_rows(prev)
    assert torch.equal(y.cpu(), want)


# ---- the generator with the scan under its weight load ------------------------------------------------------------------------------------
def _model(T, L, seed, num_layers):
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=L)
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=num_layers, num_levels=L, num_classes=10, code_size=10,
                             pc_range=S.PC_RANGE)
    m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    m.decoder.static_graph = False
    return m


def _shifted(lidar2img):
    """u -> u + 10^6 pixels"""
    m = lidar2img.clone() if torch.is_tensor(lidar2img) else np.array(lidar2img, copy=True)
    m[0] = m[0] + 1e6 * m[2]
    return m


def _poisoned_like(feats):
    pyr = TR.FeaturePyramid.empty_like_nchw(feats)
    for lv in pyr.levels:
        lv.fill_(float('nan'))
    return pyr


def _moved_units(pyr):
    """per level bool [images, tiles, 4]: the unit (64 pixels x the 64 channels of one group) was written"""
    out = []
    for lv in pyr.levels:
        px = lv.reshape(-1, lv.shape[-3] * lv.shape[-2], 4, 64)[:, ::64, :, 0]
        out.append(~torch.isnan(px.float()).cpu())
    return out


def _worst_share(units, grid):
    """most units any workgroup of a `grid`-workgroup scan finds: tile t (levels, then images, then tiles) belongs to workgroup t % grid"""
    per_tile = torch.cat([u.reshape(-1, 4).sum(1) for u in units]).numpy()
    share = np.zeros(grid, dtype=np.int64)
    np.add.at(share, np.arange(per_tile.size) % grid, per_tile)
    return int(share.max())


def _gen_grid(rows, T):
    """workgroups of the weight-stationary generator launch at this shape (sbev_linear_gen_plan)"""
    lib = _lib.load()
    pgN = 4 * (64 * 64 + 4 * T * 128)
    out = (ctypes.c_int32 * 16)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.sbev_linear_gen_plan(rows, pgN, 256, pgN, 4, 1, cus, out, 16) >= 0 and out[0] == 0, 'the weight-stationary kernel'
    return int(out[9])


# case -> (B, Q, T, layers): rows = B Q
GEN_CASES = {
    # 37 rows: no multiple of 32, 2 fragments per task (fewer than the 3 the prologue requests ahead); scans in layers 1 and 2
    'ragged_rows': (1, 37, 2, 3),
    # every image lies 10^6 pixels beside its camera's axis: no sample point hits one, no flag is set, no workgroup finds a unit
    'nothing_marked': (1, 37, 2, 3),
    # the boxes start far above every image (layer 0 marks nothing) and are refined into the range: layer 1's scan finds nearly the whole
    # pyramid, 3 tiles = 12 units in a workgroup's share against its 8 wave tiles
    'crowded_share': (2, 37, 8, 2),
}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('case', list(GEN_CASES))
def test_scan_under_the_weight_load_equals_the_scan_as_a_launch(case, dtype):
    B, Q, T, layers = GEN_CASES[case]
    ih, iw, sizes = S.PYRAMIDS['tiny']
    feats = [f.to(DEV) for f in S.make_features(B, T, sizes, seed=3, dtype=dtype)]
    bbox, feat = [t[:, :Q].contiguous().to(DEV) for t in S.make_queries(B, 49, seed=5)]
    metas = S.make_img_metas(B, T, ih, iw)
    if case == 'nothing_marked':
        for m in metas:
            m['lidar2img'] = [_shifted(x) for x in m['lidar2img']]
    if case == 'crowded_share':
        bbox[..., 2] = 1000.0
    model = _model(T, len(sizes), 21, layers)
    model(bbox, feat, list(feats), None, copy.deepcopy(metas))       # binds the runtime
    rt = model.decoder._runtime
    ctx = TR.DecoderContext(metas, B, DEV)
    lib = _lib.load()

    def step(scan_launch):
        prev = lib.sbev_decoder_lazy_scan_launch(scan_launch)
        try:
            rt._ws.zero_()
            cls, box, pyr = rt.forward_lazy(bbox, feat, feats, ctx, buffers=_poisoned_like(feats))
            torch.cuda.synchronize()
        finally:
            lib.sbev_decoder_lazy_scan_launch(prev)
        return cls.clone(), box.clone(), _moved_units(pyr), [lv.clone() for lv in pyr.levels], rt._ws.clone()

    cls_l, box_l, units_l, levels_l, ws_l = step(1)
    cls_u, box_u, units_u, levels_u, ws_u = step(0)
    assert torch.isfinite(cls_u).all() and torch.isfinite(box_u).all(), 'a tap read a unit that was not moved (NaN poison)'
    assert torch.equal(cls_u, cls_l) and torch.equal(box_u, box_l)
    for l, (a, b) in enumerate(zip(units_u, units_l)):
        assert torch.equal(a, b), 'level %d: another set of units was moved' % l
    for l, (a, b) in enumerate(zip(levels_u, levels_l)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), 'level %d: moved units differ' % l
    # the workspace holds the layer's generated parameters (and every other intermediate of the step): the same bytes
    assert torch.equal(ws_u.view(torch.uint8), ws_l.view(torch.uint8)), 'the steps leave different workspaces behind'
    want = rt.forward(bbox, feat, TR.FeaturePyramid(feats), ctx)
    assert torch.equal(cls_u, want[0]) and torch.equal(box_u, want[1]), 'the dense relayout'

    n_moved = sum(int(u.sum()) for u in units_u)
    if case == 'nothing_marked':
        assert n_moved == 0
    else:
        assert n_moved > 0
    if case == 'crowded_share':
        model.decoder.num_layers = 1
        try:
            first = _poisoned_like(feats)
            rt.forward_lazy(bbox, feat, feats, ctx, buffers=first)
        finally:
            model.decoder.num_layers = layers
        late = [u & ~f for u, f in zip(units_u, _moved_units(first))]         # what the scan of layer 1 moved
        worst = _worst_share(late, _gen_grid(B * Q, T))
        print('crowded share: %d units in one workgroup' % worst)
        assert worst > 8, 'the case no longer gives a workgroup more units than it has wave tiles'
