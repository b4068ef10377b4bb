"""The fixed-plan row-chain kernels (csrc/row_chain.hip, "fixed plans": the unit tables of config 2's launches compiled into the
kernel) against the run-time-table kernels they replace: the same arithmetic in the same order, so the whole model's outputs are equal
BIT FOR BIT between ``runtime.chain_fixed(True)`` and ``runtime.chain_fixed(False)``, on every layer, whatever the row count does to
the launch: dead rows, partial pairs, the tail with and without the next front, several samples, the largest pair launch -- and the
shapes whose key no fixed kernel covers."""
import copy
import math

import pytest
import torch

from sparsebev_amd import runtime, synthetic as S
from sparsebev_amd.transformer import SparseBEVTransformer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PREFIX = 'decoder.decoder_layer.'


def build(T, L, seed, num_layers):
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=4, num_levels=L)
    m = SparseBEVTransformer(256, num_frames=T, num_points=4, num_layers=num_layers, num_levels=L, num_classes=10, code_size=10,
                             pc_range=S.PC_RANGE)
    m.load_state_dict({PREFIX + k: v for k, v in params.items()}, strict=True)
    return m.to(DEV).eval(), params


def inputs(B, Q, T, pyr, seed):
    ih, iw, sizes = S.PYRAMIDS[pyr]
    feats = [f.to(DEV) for f in S.make_features(B, T, sizes, seed=seed)]
    side = math.isqrt(Q - 1) + 1            # make_queries lays the queries out on a square grid: the first Q of the next square
    bbox, feat = [t[:, :Q].contiguous().to(DEV) for t in S.make_queries(B, side * side, seed=seed + 1)]
    return feats, bbox, feat, S.make_img_metas(B, T, ih, iw), len(sizes)


def run_both(B, Q, T, pyr, layers, seed, fixed_per_step):
    """the model's outputs with the fixed kernels on / off, uncaptured (the switch is not part of the step-graph key);
    fixed_per_step: launches of a step that must take a fixed kernel with the switch on (none may with it off)"""
    feats, bbox, feat, metas, L = inputs(B, Q, T, pyr, seed)
    model, _ = build(T, L, seed + 1, layers)
    model.decoder.static_graph = False
    t0 = runtime.chain_pair_timeouts()
    prev = runtime.chain_fixed(True)
    try:
        n0 = runtime.chain_fixed_launches()
        on = [t.clone() for t in model(bbox, feat, list(feats), None, copy.deepcopy(metas))]
        n1 = runtime.chain_fixed_launches()
        assert runtime.chain_fixed(False) is True
        off = [t.clone() for t in model(bbox, feat, list(feats), None, copy.deepcopy(metas))]
        assert runtime.chain_fixed_launches() == n1 and n1 - n0 == fixed_per_step
        assert runtime.chain_fixed(True) is False
        again = model(bbox, feat, list(feats), None, copy.deepcopy(metas))
    finally:
        runtime.chain_fixed(prev)
    assert runtime.chain_pair_timeouts() == t0
    assert torch.isfinite(on[0]).all() and torch.isfinite(on[1]).all()
    assert on[0].shape[0] == layers and on[1].shape[0] == layers
    for l in range(layers):
        assert torch.equal(on[0][l], off[0][l]) and torch.equal(on[1][l], off[1][l]), l
    assert torch.equal(again[0], on[0]) and torch.equal(again[1], on[1])


@pytest.mark.parametrize('B,Q,T,pyr,layers', [
    (1, 1, 2, 'tiny', 2),         # one row: seven dead rows in a pair, three in the attention block
    (1, 4, 2, 'tiny', 1),         # exactly one 4-row block; last layer only: the tail runs without a front
    (1, 9, 2, 'tiny', 3),         # two pairs, a partial one; tail with front twice and without once
    (1, 65, 2, 'tiny', 2),        # nine pairs: the (li >> 1) * 8 + (b & 7) pair mapping leaves its first group of 8
    (2, 441, 2, 'tiny', 2),       # 882 rows across two samples: vel_div and per-sample metas
    (1, 1024, 1, 'tiny', 2),      # the largest pair launch; T = 1
])
def test_fixed_plan_kernels_are_bit_identical(B, Q, T, pyr, layers):
    run_both(B, Q, T, pyr, layers, 271, 1 + 2 * layers)         # the front, then an attention chain and a tail per layer


@pytest.mark.parametrize('B,Q,T,pyr,layers', [
    (1, 1089, 2, 'tiny', 2),      # too many pairs for one round: the single-workgroup tail on 8-row blocks
    (1, 100, 1, 'tiny5', 2),      # 5 levels
])
def test_other_keys_are_bit_identical_whichever_kernel_they_take(B, Q, T, pyr, layers):
    # 1089 rows: 8 rows per workgroup in all three chains, no fixed kernel.  100 rows on 5 levels: 128 sampling columns are 2 column
    # groups, the same key as 4 levels
    run_both(B, Q, T, pyr, layers, 281, 0 if B * Q > 1024 else 1 + 2 * layers)


def test_captured_step_with_fixed_kernels_replays_word_for_word():
    """One captured six-layer step at 9 rows with the switch on, replayed 20 times: every replay equals the first.  The fixed kernels need
    their dynamic-LDS attribute raised BEFORE the capture (kInst lists them, so sbev_decoder_chain_pack raises it)."""
    feats, bbox, feat, metas, L = inputs(1, 9, 2, 'tiny', 291)
    model, _ = build(2, L, 292, 6)
    t0 = runtime.chain_pair_timeouts()
    prev = runtime.chain_fixed(True)
    try:
        outs = [[t.clone() for t in model(bbox, feat, list(feats), None, copy.deepcopy(metas))] for _ in range(22)]     # eager, capture, 20 replays
        torch.cuda.synchronize()
        assert model.decoder._runtime.step_graphs.replays >= 20
        assert runtime.chain_fixed(False) is True
        model.decoder.static_graph = False
        off = model(bbox, feat, list(feats), None, copy.deepcopy(metas))
    finally:
        runtime.chain_fixed(prev)
    for i, o in enumerate(outs):
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), i
    assert torch.equal(off[0], outs[0][0]) and torch.equal(off[1], outs[0][1])
    assert runtime.chain_pair_timeouts() == t0
