"""CPU-side checks of the host logic around the C ABI (no GPU needed): module/state-dict compatibility with the
reference, per-call context (time_diff, lidar2img, velocity divisor), sharding helpers, loud failure modes."""
import numpy as np
import pytest
import torch

from sparsebev_amd import synthetic as S
from sparsebev_amd.transformer import SparseBEVTransformer, DecoderContext, FeaturePyramid

PREFIX = 'decoder.decoder_layer.'


def test_state_dict_keys_match_reference():
    m = SparseBEVTransformer(256, num_frames=8, pc_range=S.PC_RANGE)
    keys = sorted(m.state_dict())
    want = sorted(PREFIX + k for k in S.param_shapes())
    assert keys == want and len(keys) == 48
    m.init_weights()
    sd = m.state_dict()
    assert sd[PREFIX + 'mixing.parameter_generator.weight'].abs().sum() == 0
    assert sd[PREFIX + 'sampling.sampling_offset.weight'].abs().sum() == 0
    assert sd[PREFIX + 'self_attn.gen_tau.weight'].abs().sum() == 0
    assert abs(float(sd[PREFIX + 'cls_branch.6.bias'][0]) + 4.59512) < 1e-4


def test_decoder_context_matches_oracle_prologue():
    from oracle import sparsebev_oracle as O
    B, T = 2, 8
    metas = S.make_img_metas(B, T, 256, 704)
    for b, m in enumerate(metas):
        m['img_timestamp'] = [ts + 0.003 * ((i * 7 + b) % 6) for i, ts in enumerate(m['img_timestamp'])]
    ctx = DecoderContext(metas, B, torch.device('cpu'))
    td = O.time_diff_from_metas(metas, B)
    assert torch.equal(ctx.time_diff, td)                                  # float64 mean -> fp32, bit for bit
    assert ctx.lidar2img.shape == (B, T * 6, 4, 4) and ctx.lidar2img.dtype == torch.float32
    assert (ctx.image_h, ctx.image_w) == (256, 704)
    exp = td[:, 1].clone()
    exp[exp < 1e-5] = 1.0
    assert torch.equal(ctx.vel_div, exp)
    # the three constants are segments of ONE packed upload: contiguous views at 16-byte boundaries with the metas' values
    import numpy as np
    assert np.array_equal(ctx.lidar2img.numpy(), np.asarray([m['lidar2img'] for m in metas]).astype(np.float32))
    for t in (ctx.time_diff, ctx.lidar2img, ctx.vel_div):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
    assert ctx.lidar2img.data_ptr() - ctx.time_diff.data_ptr() == 4 * ((B * T + 3) // 4 * 4)
    assert 'time_diff' not in metas[0]                                     # the reference mutates img_metas[0]; we do not
    # T == 1: no velocity division (models/sparsebev_transformer.py:180)
    assert DecoderContext(S.make_img_metas(1, 1, 256, 704), 1, torch.device('cpu')).vel_div is None


def test_zero_time_diff_is_replaced_by_one():
    metas = S.make_img_metas(1, 2, 256, 704, frame_dt=0.0)                 # both frames share a timestamp
    ctx = DecoderContext(metas, 1, torch.device('cpu'))
    assert float(ctx.vel_div[0]) == 1.0


def test_product_refuses_cpu_features_in_eval_and_in_training():
    m = SparseBEVTransformer(256, num_frames=1, pc_range=S.PC_RANGE).eval()
    feats = S.make_features(1, 1, S.PYRAMIDS['tiny'][2])
    with pytest.raises(RuntimeError, match='no CPU path'):
        FeaturePyramid(feats)
    bbox, feat = S.make_queries(1, 4)
    m.train()
    with torch.enable_grad(), pytest.raises(RuntimeError, match='no CPU path'):    # the training path has no CPU fallback either
        m(bbox, feat, feats, None, S.make_img_metas(1, 1, 256, 704))
    with pytest.raises(AssertionError):
        SparseBEVTransformer(256, init_cfg=dict(type='Xavier'))            # same guard as the reference (:19-20)


def test_synthetic_rig_hit_statistics():
    """The bench rig must exercise 0-, 1- and 2-hit points in realistic proportions."""
    from oracle import sparsebev_oracle as O
    B, Q, T = 1, 400, 8
    ih, iw, _ = S.PYRAMIDS['r50_704x256']
    metas = S.make_img_metas(B, T, ih, iw)
    bbox, feat = S.make_queries(B, Q)
    prm = S.make_params(0)
    pts, _ = O.sampling_front(prm, bbox, feat, O.time_diff_from_metas(metas, B), S.PC_RANGE, T, 4, 4)
    l2i = torch.from_numpy(np.asarray([m['lidar2img'] for m in metas]).astype(np.float32))
    _, valid = O.project_points(pts.reshape(B, Q, T, 16, 3), l2i, ih, iw)
    hits = valid.sum(2)
    assert 0.85 < (hits >= 1).float().mean() < 0.99
    assert 0.01 < (hits >= 2).float().mean() < 0.15


def test_head_module_host_side():
    """SparseBEVHead / NMSFreeCoder host logic without a GPU: reference parameter names, the query grid of
    models/sparsebev_head.py:49-67, config-dict handling, loud failures (training, CPU tensors)."""
    from oracle import sparsebev_oracle as O
    from sparsebev_amd.head import NMSFreeCoder, SparseBEVHead, head_prepare
    post = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
    head = SparseBEVHead(num_classes=10, in_channels=256, num_query=900, code_size=10, code_weights=[2.0, 2.0] + [1.0] * 8,
                         transformer=dict(type='SparseBEVTransformer', embed_dims=256, num_frames=8, num_points=4, num_layers=6,
                                          num_levels=4, num_classes=10, code_size=10, pc_range=S.PC_RANGE),
                         bbox_coder=dict(type='NMSFreeCoder', post_center_range=post, max_num=300, score_threshold=0.05,
                                         num_classes=10, pc_range=S.PC_RANGE))
    keys = set(head.state_dict())
    assert {'init_query_bbox.weight', 'label_enc.weight', 'code_weights'} <= keys and len(keys) == 51
    assert all(k.startswith('transformer.decoder.decoder_layer.') for k in keys - {'init_query_bbox.weight', 'label_enc.weight', 'code_weights'})
    w = head.init_query_bbox.weight.detach()
    assert w.shape == (900, 10) and head.label_enc.weight.shape == (11, 255)
    ii, jj = torch.meshgrid(torch.arange(30), torch.arange(30), indexing='ij')
    assert torch.equal(w[:, 0], ((ii.reshape(-1).float() + 0.5) / 30)) and torch.equal(w[:, 1], ((jj.reshape(-1).float() + 0.5) / 30))
    assert float(w[:, 2].abs().max()) == 0 and float(w[:, 8:].abs().max()) == 0 and torch.all(w[:, 5] == 1.5)
    assert isinstance(head.bbox_coder, NMSFreeCoder) and head.bbox_coder.max_num == 300 and head.pc_range == S.PC_RANGE
    assert not head.code_weights.requires_grad and head.code_weights[0] == 2.0
    # the oracle's restatement of the eval-branch query init agrees with the module's parameters
    qb, qf = O.head_prepare(w, head.label_enc.weight.detach(), 10, 2)
    assert qb.shape == (2, 900, 10) and qf.shape == (2, 900, 256) and torch.equal(qf[0, 5, :255], head.label_enc.weight[10].detach())
    with pytest.raises(RuntimeError, match='no CPU path'):
        head_prepare(w, head.label_enc.weight.detach(), 10, 1)              # CPU tensors: the product has no fallback
    with pytest.raises(NotImplementedError):
        head.train()(S.make_features(1, 8, S.PYRAMIDS['tiny'][2]), S.make_img_metas(1, 8, 256, 704))
    with pytest.raises(NotImplementedError):
        head.loss()
    with pytest.raises(ValueError):
        SparseBEVHead(num_classes=10, in_channels=256, bbox_coder=dict(type='DETR3DCoder', pc_range=S.PC_RANGE),
                      transformer=dict(type='SparseBEVTransformer', embed_dims=256, pc_range=S.PC_RANGE))


def test_version_switch_reaches_the_library():
    """VERSION.name mirrors the reference's module-global switch and forwards to sbev_set_box_convention."""
    from sparsebev_amd import _lib
    from sparsebev_amd.utils import VERSION
    lib = _lib.load()
    assert VERSION.name == 'v1.0.0' and lib.sbev_get_box_convention() == 0
    try:
        VERSION.name = 'v0.17.1'
        assert lib.sbev_get_box_convention() == 1
        VERSION.require_supported()
        with pytest.raises(NotImplementedError):
            VERSION.name = 'v2'
        assert VERSION.name == 'v0.17.1'
    finally:
        VERSION.name = 'v1.0.0'
    assert lib.sbev_get_box_convention() == 0
    assert lib.sbev_set_box_convention(7) != 0 and b'convention' in lib.sbev_last_error()


# ---- what a decoder step enqueues is decided in one place (csrc/decoder.hip: plan_step) ------------------------------------------

_PLAN_PYRAMIDS = {4: [(64, 176), (32, 88), (16, 44), (8, 22)], 5: [(128, 352), (64, 176), (32, 88), (16, 44), (8, 22)]}


def _plan_config(gemm_mode, overlap, L, feat_dtype, B):
    from sparsebev_amd import runtime as R
    c = R.DecoderConfig()
    c.B, c.Q, c.T, c.N, c.G, c.P, c.L = B, 900, 8, 6, 4, 4, L
    c.D, c.H, c.ffn, c.num_classes, c.code_size, c.num_layers = 256, 8, 512, 10, 10, 6
    c.out_points, c.attn_in_rows, c.feat_dtype = 128, 3 * 256 + 8, feat_dtype
    for l, (h, w) in enumerate(_PLAN_PYRAMIDS[L]):
        c.hw[l][0], c.hw[l][1] = h, w
    c.image_h, c.image_w, c.eps_homo, c.gemm_mode, c.overlap = 256.0, 704.0, 1e-5, gemm_mode, overlap
    return c


# one line per (gemm_mode 0..5, row_chain 1 / 0, fuse_sample_mix 1 / 0, query_order 0 / 1 / 2) in itertools.product order; within a line
# (overlap 0 / 1 / 2) x (L=4 fp32, L=5 fp32, L=5 bf16) x (900, 3600, 7200 rows) x (chain_pack null, non-null), same order
_LAUNCHES_PER_LAYER = [
    '17 6 17 6 17 17 17 6 17 6 17 17 17 6 17 6 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '17 7 17 7 17 17 17 7 17 7 17 17 17 7 17 7 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '17 6 17 6 17 17 17 6 17 6 17 17 17 6 17 6 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17 17',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 8 18 8 18 18 18 8 18 8 18 18 18 8 18 8 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 8 18 8 18 18 18 8 18 8 18 18 18 8 18 8 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 8 18 8 18 18 18 8 18 8 18 18 18 8 18 8 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 8 19 8 19 19 19 8 19 8 19 19 19 8 19 8 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 6 18 6 18 18 18 6 18 6 18 18 18 6 18 6 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 6 18 6 18 18 18 6 18 6 18 18 18 6 18 6 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 6 18 6 18 18 18 6 18 6 18 18 18 6 18 6 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 7 18 7 18 18 18 7 18 7 18 18 18 7 18 7 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 6 18 6 18 18 18 6 18 6 18 18 18 6 18 6 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 7 19 7 19 19 19 7 19 7 19 19 19 7 19 7 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18 18',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
    '19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19 19',
]


def test_launches_per_layer_table_is_the_recorded_one():
    """sbev_decoder_launches_per_layer is the forward's own plan (csrc/decoder.hip: plan_step); its values for 3888 (mode, switches, shape,
    weights) cases + one invalid config equal the table recorded from the commit BEFORE the plan existed, when the entry point was a hand
    copy of the forward's conditions.  The table was printed by this very loop (the two `for` statements below with `row.append(got)` in
    place of the comparison, one `' '.join` per row) run against a build of that commit.  No device needed."""
    import ctypes
    import itertools
    from sparsebev_amd import _lib, runtime as R
    lib = _lib.load()
    before = R._switch_key()
    keep = ctypes.create_string_buffer(64)           # any non-null address: the entry point never reads through chain_pack
    table = [[int(v) for v in line.split()] for line in _LAUNCHES_PER_LAYER]
    assert len(table) == 72 and all(len(r) == 54 for r in table)
    n = 0
    try:
        for row, (mode, chain, fuse, order) in zip(table, itertools.product(range(6), (1, 0), (1, 0), (0, 1, 2))):
            lib.sbev_decoder_row_chain(chain)
            lib.sbev_decoder_fuse_sample_mix(fuse)
            lib.sbev_decoder_query_order(order)
            for want, (overlap, (L, dt), B, pack) in zip(row, itertools.product((0, 1, 2), ((4, 0), (5, 0), (5, 1)), (1, 4, 8), (False, True))):
                w = R.DecoderWeights()
                if pack:
                    w.chain_pack = ctypes.cast(keep, ctypes.c_void_p)
                got = lib.sbev_decoder_launches_per_layer(ctypes.byref(_plan_config(mode, overlap, L, dt, B)), ctypes.byref(w))
                assert got == want, (mode, chain, fuse, order, overlap, L, dt, B, pack, got, want)
                n += 1
    finally:
        lib.sbev_decoder_row_chain(before[0])
        lib.sbev_decoder_fuse_sample_mix(before[2])
        lib.sbev_decoder_query_order(before[4])
    assert n == 3888 and R._switch_key() == before
    bad = _plan_config(0, 0, 4, 0, 1)
    bad.gemm_mode = 6
    assert lib.sbev_decoder_launches_per_layer(ctypes.byref(bad), ctypes.byref(R.DecoderWeights())) == -1
    assert lib.sbev_decoder_launches_per_layer(ctypes.byref(_plan_config(4, 0, 4, 0, 1)), None) == -1


def test_every_switch_is_in_the_step_graph_key():
    """runtime._switch_key() -- the switch part of StepGraphs' key -- is the library's own reading (sbev_decoder_switches) + the two
    Python-side switches: toggling ANY switch changes it, restoring the switch restores it, and the raw C setter and the Python wrapper
    (where there is one) give the same key.  Includes the four the key used to miss: out8_min_rows, lazy_scan_launch,
    gen_weight_stationary, msmv_buffer_taps."""
    import ctypes
    from sparsebev_amd import _lib, runtime as R
    from sparsebev_amd.utils import VERSION
    lib = _lib.load()
    buf = (ctypes.c_int32 * 4)()
    assert lib.sbev_decoder_switches(buf, 4) == 11 and tuple(buf) == R._switch_key()[:4]       # (a short buffer is filled, never overrun)
    assert lib.sbev_decoder_switches(None, 0) == 11
    base = R._switch_key()
    assert len(base) == 13 and base[10] == lib.sbev_get_box_convention()

    def set_version(code):
        VERSION.name = {0: 'v1.0.0', 1: 'v0.17.1'}[code]

    # (position in the key, raw C setter, Python wrapper or None, another value)
    cases = [(0, lib.sbev_decoder_row_chain, R.row_chain, 1 - base[0]),
             (1, lib.sbev_decoder_chain_pair, R.chain_pair, 1 - base[1]),
             (2, lib.sbev_decoder_fuse_sample_mix, R.fuse_sample_mix, 1 - base[2]),
             (4, lib.sbev_decoder_query_order, R.query_order, 1 if base[4] != 1 else 2),
             (4, lib.sbev_decoder_query_order, R.query_order, 2 if base[4] != 2 else 0),
             (5, lib.sbev_decoder_lazy_scan_launch, None, 1 - base[5]),
             (6, lib.sbev_decoder_out_fold, R.out_fold, 1 - base[6]),
             (7, lib.sbev_linear_gen_weight_stationary, None, 1 - base[7]),
             (8, lib.sbev_linear_out8_min_rows, None, 0 if base[8] else 1024),
             (8, lib.sbev_linear_out8_min_rows, None, base[8] + 1024),
             (9, lib.sbev_msmv_buffer_taps, None, 1 - base[9]),
             (10, lib.sbev_set_box_convention, set_version, 1 - base[10])]
    seen = {base}
    for pos, c_set, py_set, other in cases:
        keys = []
        for setter in (c_set, py_set):
            if setter is None:
                continue
            try:
                setter(other)
                keys.append(R._switch_key())
            finally:
                setter(base[pos])
            assert R._switch_key() == base, (pos, other)
        changed = base[:pos] + (other,) + base[pos + 1:]
        assert all(k == changed for k in keys), (pos, other, keys)       # that switch moved, no other did, both ways of setting agree
        seen.add(changed)
    assert len(seen) == len(cases) + 1
    # the two switches Python owns
    prev = R.lazy_relayout(not base[11])
    try:
        assert prev == base[11] and R._switch_key() == base[:11] + (not base[11], base[12])
    finally:
        R.lazy_relayout(prev)
    R._STATE['relayout_multi'] = not base[12]
    try:
        assert R._switch_key() == base[:12] + (not base[12],)
    finally:
        R._STATE['relayout_multi'] = base[12]
    assert R._switch_key() == base
    # the one report-only entry that stays in _STATE follows query_order() and starts from the library's value
    assert R._STATE['order'] == base[4]


def _planner_cases():
    one_row = lambda n, segs=6: [('p%d' % i, 36, segs, False) for i in range(n)]
    cases = {'decoder-16': (one_row(40), 16), 'decoder-8': (one_row(40), 8)}
    for n in (8, 9, 16, 17):
        cases['%d-segments' % n] = ([('k', 36, n, False)], 16)
    cases['17-keys'] = (one_row(17), 16)
    cases['9-keys'] = (one_row(9), 8)
    cases['two-row-counts'] = ([('p%d' % i, 36 if i % 2 else 20, 9, False) for i in range(20)], 8)
    cases['has-buffer'] = ([('a', 36, 6, False), ('b', 36, 6, True), ('c', 36, 17, True)], 16)
    cases['zero-segments'] = ([('a', 36, 6, False), ('z', 36, 0, False), ('b', 36, 9, False)], 16)
    cases['empty'] = ([], 16)
    return [pytest.param(jobs, mj, id=name) for name, (jobs, mj) in cases.items()]


@pytest.mark.parametrize('jobs,max_jobs', _planner_cases())
def test_grouped_reduction_planner_covers_every_segment_once_and_orders_a_parameters_chunks(jobs, max_jobs):
    """autograd._plan_launches (what _group_bias_grads and _group_ln_grads marshal): every segment of every parameter in exactly one
    entry, <= 8 segments per entry, <= max_jobs entries and one row count per launch, a parameter at most once per launch and its
    chunks in increasing order over the launches (a later chunk adds to what the earlier one wrote), accumulate exactly for a later
    chunk or a parameter that had a buffer already."""
    from sparsebev_amd.autograd import _plan_launches
    max_segs = 8
    launches = _plan_launches(jobs, max_jobs, max_segs)
    rows_of = {k: r for k, r, _, _ in jobs}
    filled = {k: f for k, _, _, f in jobs}
    covered = {k: [] for k, _, n, _ in jobs}
    last_start = {}
    for rows, entries in launches:
        assert 1 <= len(entries) <= max_jobs
        keys = [e[0] for e in entries]
        assert len(set(keys)) == len(keys)
        for key, s0, s1, acc in entries:
            assert rows_of[key] == rows
            assert 0 < s1 - s0 <= max_segs
            assert s0 > last_start.get(key, -1)
            last_start[key] = s0
            assert acc == (s0 > 0 or filled[key])
            covered[key] += range(s0, s1)
    for key, _, nseg, _ in jobs:
        assert covered[key] == list(range(nseg)), key
    if not any(n for _, _, n, _ in jobs):
        assert launches == []


def test_grouped_reduction_planner_literal_case():
    """three parameters with 9, 2 and 1 segments, two of them at 36 rows and one at 20: the launch list spelled out -- the ninth segment
    of `a` accumulates in a launch AFTER the one that wrote its first eight"""
    from sparsebev_amd.autograd import _plan_launches
    jobs = [('a', 36, 9, False), ('b', 20, 2, False), ('c', 36, 1, False)]
    assert _plan_launches(jobs, 16) == [(20, [('b', 0, 2, False)]),
                                        (36, [('a', 0, 8, False), ('c', 0, 1, False)]),
                                        (36, [('a', 8, 9, True)])]
    assert _plan_launches(jobs, 1) == [(20, [('b', 0, 2, False)]), (36, [('a', 0, 8, False)]), (36, [('c', 0, 1, False)]),
                                       (36, [('a', 8, 9, True)])]
