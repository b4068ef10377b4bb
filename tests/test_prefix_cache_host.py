"""Prefix cache, host side (no GPU): the size of the caller's block (sbev_prefix_cache_bytes) and the rule that decides whether a step
uses one (sbev_decoder_prefix_planned: a cache was passed, row chains with the weight-stationary generator, no mask, no launch
profiling).  The config struct and the switch list keep their layout (tests/test_capi_pool.py, tests/test_host_logic.py)."""
import ctypes

import pytest

from sparsebev_amd import _lib
from sparsebev_amd.runtime import DecoderConfig, DecoderWeights, GEMM_F32, GEMM_F16X3, GEMM_F16X4, GEMM_BF16X6


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def config(B=1, Q=900, T=8, mode=GEMM_F16X3):
    cfg = DecoderConfig()
    cfg.B, cfg.Q, cfg.T, cfg.N, cfg.G, cfg.P, cfg.L = B, Q, T, 6, 4, 4, 4
    cfg.D, cfg.H, cfg.ffn, cfg.num_classes, cfg.code_size, cfg.attn_in_rows = 256, 8, 512, 10, 10, 776
    cfg.num_layers, cfg.out_points, cfg.gemm_mode = 6, 128, mode
    for l, (h, w) in enumerate([(64, 176), (32, 88), (16, 44), (8, 22)]):
        cfg.hw[l][0], cfg.hw[l][1] = h, w
    return cfg


def pad(n_bytes):
    return (n_bytes + 255) // 256 * 256


def test_cache_bytes(lib):
    for B, Q, T in ((1, 900, 8), (1, 36, 2), (2, 49, 2)):
        BQ, D = B * Q, 256
        pgN = 4 * (64 * 64 + T * 4 * 128)
        want = pad(4 * (4 + 64)) + pad(4 * BQ * 10) + 3 * pad(4 * BQ * D) + pad(4 * BQ * pgN)
        assert lib.sbev_prefix_cache_bytes(ctypes.byref(config(B, Q, T))) == want
    assert lib.sbev_prefix_cache_bytes(ctypes.byref(config(1, 900, 8))) > 900 * 32768 * 4          # 118 MB of parameters at config 2
    bad = config()
    bad.code_size = 11
    assert lib.sbev_prefix_cache_bytes(ctypes.byref(bad)) == -1 and lib.sbev_prefix_cache_bytes(None) == -1


def test_plan_rule(lib):
    w = DecoderWeights()
    w.chain_pack = 0x1000          # (never read: the plan touches no device)
    plan = lambda cfg, cache=1, mask=0, lazy=0, weights=w: lib.sbev_decoder_prefix_planned(ctypes.byref(cfg), ctypes.byref(weights), cache, mask, lazy)
    for mode in (GEMM_F16X3, GEMM_F16X4):
        for B, Q, T in ((1, 900, 8), (1, 36, 2), (2, 49, 2)):
            cfg = config(B, Q, T, mode)
            assert plan(cfg) == 1 and plan(cfg, lazy=1) == 1
            assert plan(cfg, cache=0) == 0 and plan(cfg, mask=1) == 0
    assert plan(config(mode=GEMM_F32)) == 0                       # no split-image generator
    assert plan(config(mode=GEMM_BF16X6)) == 0                    # three images: not the weight-stationary kernel
    assert plan(config(), weights=DecoderWeights()) == 0          # no packed weights: op-by-op launches
    assert plan(config(B=8, Q=900)) == 0                          # 7200 rows: beyond the row chains
    prev = lib.sbev_linear_gen_weight_stationary(0)
    try:
        assert plan(config()) == 0
    finally:
        lib.sbev_linear_gen_weight_stationary(prev)
    assert lib.sbev_decoder_row_chain(0) == 0
    try:
        assert plan(config()) == 0
    finally:
        lib.sbev_decoder_row_chain(1)
    lib.sbev_profile_sampler(1)                                   # launch profiling: every launch stays a full one
    try:
        assert plan(config()) == 0
    finally:
        lib.sbev_profile_sampler(0)
    assert plan(config()) == 1
    bad = config()
    bad.code_size = 11
    assert plan(bad) == -1 and lib.sbev_decoder_prefix_planned(ctypes.byref(config()), None, 1, 0, 0) == -1


def test_a_cache_changes_neither_struct(lib):
    assert DecoderConfig._fields_[-1][0] == 'slot_table'
    assert lib.sbev_decoder_switches(None, 0) == 11


def test_captured_step_and_key_defaults():
    from sparsebev_amd import runtime
    assert runtime.CapturedStep(None, False).prefix is None
    assert 'prefix' not in runtime.StepKey._fields and len(runtime.StepKey._fields) == 11
