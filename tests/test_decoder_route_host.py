"""The decoder call in Python, as far as it needs no device and no library: SparseBEVTransformerDecoder._route (which of the three bodies
a call takes, decided once), the GEMM mode's name-to-code step, and the one recipe of the packed weight rows that the training path and
DecoderRuntime._bind both take."""
import contextlib
import warnings

import pytest
import torch

from sparsebev_amd.runtime import GEMM_MODES
from sparsebev_amd.transformer import DecoderRoute, SparseBEVTransformerDecoder
from sparsebev_amd.utils import DUMP, frame_source
from test_step_host import Dense, Pool, Ring

PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def decoder(train=False, frozen=False, static_graph=True):
    dec = SparseBEVTransformerDecoder(256, num_frames=2, num_points=4, num_layers=2, num_levels=1, pc_range=PC_RANGE)
    dec.train(train)
    dec.static_graph = static_graph
    for p in dec.parameters():
        p.requires_grad_(not frozen)
    return dec


def feature_list(dtype=torch.float32):
    return [torch.zeros(1, 12, 256, 4, 4, dtype=dtype)]      # 2 frames, 1 level


def route(dec, feats, grad, layerwise=False, bbox_dtype=torch.float32):
    bbox, feat = torch.zeros(1, 4, 10, dtype=bbox_dtype), torch.zeros(1, 4, 256)
    with torch.enable_grad() if grad else torch.no_grad():
        return dec._route(bbox, feat, feats, layerwise)


@contextlib.contextmanager
def dump_enabled():
    DUMP.enabled = True
    try:
        yield
    finally:
        DUMP.enabled = False


# ---- the route -----------------------------------------------------------------------------------------------------------------------

def test_inference_calls_take_the_runtime_and_replay_only_fp32_queries_with_graphs_on():
    feats = feature_list()
    r = route(decoder(), feats, grad=False)                                                   # row 1
    assert r == DecoderRoute('runtime', True, frame_source(feats), False) and r.src.kind == 'list'
    assert route(decoder(static_graph=False), feats, grad=False)[:2] == ('runtime', False)    # row 2
    assert route(decoder(), feats, grad=False, bbox_dtype=torch.float16)[:2] == ('runtime', False)      # row 3
    # no_grad decides, whatever the mode and the parameters say
    assert route(decoder(train=True), feats, grad=False)[:2] == ('runtime', True)


def test_layerwise_and_the_dump_taps_take_the_layerwise_body():
    feats = feature_list()
    assert route(decoder(), feats, grad=False, layerwise=True) == DecoderRoute('layerwise', False, frame_source(feats), False)      # row 4
    assert not DUMP.enabled
    with dump_enabled():
        assert route(decoder(), feats, grad=False)[:2] == ('layerwise', False)                # row 5
    assert route(decoder(), feats, grad=False).path == 'runtime'


@pytest.mark.parametrize('train', (True, False))
def test_grad_enabled_and_something_requiring_grad_trains(train):
    feats = feature_list()
    assert route(decoder(train=train), feats, grad=True) == DecoderRoute('train', False, frame_source(feats), False)      # rows 6, 7
    # rows 12, 13: nothing requires grad -> inference, in either mode; one feature tensor does -> train
    assert route(decoder(train=train, frozen=True), feats, grad=True) == DecoderRoute('runtime', True, frame_source(feats), False)
    feats[0].requires_grad_(True)
    assert route(decoder(train=train, frozen=True), feats, grad=True)[:2] == ('train', False)
    dec, bbox = decoder(train=train, frozen=True), torch.zeros(1, 4, 10)
    with torch.enable_grad():                                 # (and so does a query that requires grad)
        assert dec._route(bbox, torch.zeros(1, 4, 256, requires_grad=True), feature_list()).path == 'train'


def test_layerwise_is_ignored_on_the_training_path():
    assert route(decoder(train=True), feature_list(), grad=True, layerwise=True)[:2] == ('train', False)      # row 14
    with dump_enabled():
        assert route(decoder(train=True), feature_list(), grad=True).path == 'train'


@pytest.mark.parametrize('make', (Ring, Pool, lambda: feature_list(torch.bfloat16)), ids=('ring', 'pool', 'bf16'))
def test_eval_with_grad_on_inputs_autograd_cannot_take_is_demoted_to_the_runtime(make):
    feats = make()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert route(decoder(), feats, grad=True) == DecoderRoute('runtime', True, frame_source(feats), True)      # rows 8, 9, 10
        assert route(decoder(), feats, grad=True, layerwise=True) == DecoderRoute('layerwise', False, frame_source(feats), True)      # row 15
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        # train() is not demoted: the call reaches forward_differentiable, which refuses such features (row 11)
        assert route(decoder(train=True), feats, grad=True) == DecoderRoute('train', False, frame_source(feats), False)
    # a dense pyramid of fp32 levels is something the autograd path can take
    assert route(decoder(), Dense(), grad=True) == DecoderRoute('train', False, frame_source(Dense()), False)


def test_the_demotion_warns_once_per_decoder():
    dec, other = decoder(), decoder()
    with pytest.warns(UserWarning, match='eval-mode call with grad enabled on ring / bf16 features: running the inference runtime'):
        assert route(dec, Ring(), grad=True).demoted
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert route(dec, Pool(), grad=True).demoted and route(dec, Ring(), grad=True, layerwise=True).demoted
        assert not route(dec, Ring(), grad=False).demoted     # (under no_grad there is nothing to demote)
    with pytest.warns(UserWarning, match='wrap inference in torch.no_grad'):
        assert route(other, Ring(), grad=True).demoted


# ---- the GEMM mode -------------------------------------------------------------------------------------------------------------------

def test_every_gemm_mode_name_and_code_resolves_to_its_code():
    dec = decoder()
    assert GEMM_MODES == {'f32': 0, 'bf16x3': 1, 'bf16x6': 2, 'bf16x3s': 3, 'f16x3': 4, 'f16x4': 5}
    for name, code in GEMM_MODES.items():
        for given in (name, code):
            dec.gemm_mode = given
            assert dec._gemm_mode_code() == code
            if code < 2:                                      # (from 2 on the runtime path asks the library whether the split kernels cover the rows)
                assert dec._gemm_mode_code(rows=4) == code


def test_an_unknown_gemm_mode_is_refused_on_the_runtime_path_only():
    dec = decoder()
    dec.gemm_mode = 'f8'
    with pytest.raises(ValueError) as e:
        dec._gemm_mode_code(rows=4)
    assert str(e.value) == "gemm_mode 'f8': expected one of ['bf16x3', 'bf16x3s', 'bf16x6', 'f16x3', 'f16x4', 'f32']"
    dec.gemm_mode = 6
    with pytest.raises(ValueError, match='gemm_mode 6: expected one of'):
        dec._gemm_mode_code(rows=4)
    assert dec._gemm_mode_code() == 6                         # the training path: no new error (autograd.AdaptiveMixing has its own rule)


# ---- the packed rows -----------------------------------------------------------------------------------------------------------------

def test_packed_rows_are_the_explicit_cat_padded_to_a_multiple_of_four():
    layer = decoder().decoder_layer
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    att, tau, smp = layer.self_attn.attention.attn, layer.self_attn.gen_tau, layer.sampling
    with torch.no_grad():                                     # as DecoderRuntime._bind takes them
        in_w, in_b, samp_w, samp_b = packed = layer.packed_train_weights()
    assert in_w.shape == (776, 256) and in_b.shape == (776,) and 776 == (3 * 256 + 8 + 3) // 4 * 4      # (8 heads: no pad row)
    assert torch.equal(in_w, torch.cat([att.in_proj_weight, tau.weight], 0))
    assert torch.equal(in_b, torch.cat([att.in_proj_bias, tau.bias], 0))
    assert torch.equal(samp_w, torch.cat([smp.sampling_offset.weight, smp.scale_weights.weight], 0)) and samp_w.shape == (4 * 4 * 3 + 4 * 4 * 1, 256)
    assert torch.equal(samp_b, torch.cat([smp.sampling_offset.bias, smp.scale_weights.bias], 0))
    assert all(t.is_contiguous() and not t.requires_grad for t in packed)
    with torch.enable_grad():                                 # the training path's: gradients reach the parameters through the cat
        assert all(t.requires_grad for t in layer.packed_train_weights())


def test_packed_rows_pad_with_zero_rows_when_the_head_count_is_no_multiple_of_four():
    layer = decoder().decoder_layer
    sa = layer.self_attn
    sa.num_heads, sa.gen_tau = 6, torch.nn.Linear(256, 6)     # 3 * 256 + 6 = 774 rows -> 776
    in_w, in_b, _, _ = layer.packed_train_weights()
    assert in_w.shape == (776, 256) and in_b.shape == (776,) and in_w.is_contiguous() and in_b.is_contiguous()
    assert torch.equal(in_w[:768], sa.attention.attn.in_proj_weight) and torch.equal(in_w[768:774], sa.gen_tau.weight)
    assert torch.equal(in_b[768:774], sa.gen_tau.bias) and not in_w[774:].any() and not in_b[774:].any()
