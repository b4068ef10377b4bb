"""sbev_decoder_chain_fixed_plan: the unit tables COMPILED INTO the fixed-plan row-chain kernels (csrc/row_chain.hip, "fixed plans").
They come out of the same planner as the run-time tables (plan_units, constexpr), so for every key the build covers the words equal
sbev_decoder_chain_plan's, and for every other key the export says "none" (0) and the launch keeps the run-time-table kernel.  Pure host:
no GPU.  Covered keys of this build: config 2's launches -- the tail on pairs of 8 rows with and without the next front, the attention
chain and the front chain on 4-row blocks -- at 13 in-projection and 2 sampling column groups."""
import ctypes
import itertools
import os

import pytest

from sparsebev_amd import _lib

TAIL, FRONT, ATT = 0, 1, 2
D, FFN, CODE = 256, 512, 10
CLASSES = (1, 10, 64)
# (kind, with_front, pair_ok): the launches a covered config makes
LAUNCHES = ((TAIL, 1, 1), (TAIL, 0, 1), (FRONT, 0, 0), (ATT, 0, 0))


@pytest.fixture(scope='module')
def plans():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    from sparsebev_amd.runtime import DecoderConfig
    lib = _lib.load()
    a, b = (ctypes.c_int32 * 512)(), (ctypes.c_int32 * 512)()

    def call(B, Q, kind, with_front, pair_ok, cus=256, classes=10, qkv=776, G=4, P=4, L=4, capacity=512):
        """(the run-time plan's words, the fixed plan's words or 0 / -1)"""
        cfg = DecoderConfig()
        cfg.B, cfg.Q, cfg.G, cfg.P, cfg.L = B, Q, G, P, L
        cfg.T, cfg.N, cfg.H = 8, 6, 8
        cfg.D, cfg.ffn, cfg.code_size, cfg.num_classes, cfg.attn_in_rows = D, FFN, CODE, classes, qkv
        n = lib.sbev_decoder_chain_plan(ctypes.byref(cfg), kind, with_front, pair_ok, cus, a, 512)
        m = lib.sbev_decoder_chain_fixed_plan(ctypes.byref(cfg), kind, with_front, pair_ok, cus, b, capacity)
        return (list(a[:n]) if n > 0 else n), (list(b[:m]) if m > 0 else m)
    return call


@pytest.mark.parametrize('B,Q', [(1, 4), (1, 900), (2, 450), (1, 1024), (2, 512)])
def test_covered_keys_equal_the_run_time_plan_word_for_word(plans, B, Q):
    """4, 900 and 1024 rows (the largest pair launch); with and without front; both members (a pair plan carries both tables);
    1, 10 and 64 classes (one column group whatever the count); 769 .. 832 in-projection rows and 65 .. 128 sampling columns are the
    same 13 and 2 column groups."""
    for (kind, with_front, pair_ok), classes, qkv, (G, P, L) in itertools.product(LAUNCHES, CLASSES, (769, 776, 832), ((4, 4, 4), (4, 4, 5), (1, 13, 2))):
        run, fixed = plans(B, Q, kind, with_front, pair_ok, classes=classes, qkv=qkv, G=G, P=P, L=L)
        case = (B, Q, kind, with_front, classes, qkv, G, P, L)
        assert isinstance(run, list) and fixed == run, case
        pre, rg, pair, n_units = run[0], run[1], run[2], run[5]
        assert (pre, rg, pair) == ((TAIL, 2, 1) if kind == TAIL else (kind, 1, 0)), case
        assert len(run) == 12 + 18 * (2 if pair else 1) * n_units and n_units == {TAIL: 7 if with_front else 5, FRONT: 3, ATT: 2}[kind], case
    # the front and the attention chain do not depend on the tail's inputs
    assert plans(B, Q, FRONT, 1, 1)[1] == plans(B, Q, FRONT, 0, 0)[1] and plans(B, Q, ATT, 1, 1)[1] == plans(B, Q, ATT, 0, 0)[1]


def test_uncovered_keys_report_none(plans):
    for kind, with_front, pair_ok in LAUNCHES:
        case = (kind, with_front, pair_ok)
        assert isinstance(plans(1, 900, kind, with_front, pair_ok)[1], list), case                    # (the covered key itself)
        # other sampling column-group counts: 1, 3, 4 (config 6's 256 columns), and 5 groups' worth (320 columns: no row chain at all)
        for G, P, L in ((4, 2, 4), (4, 4, 9), (4, 8, 5), (4, 8, 7)):
            run, fixed = plans(1, 900, kind, with_front, pair_ok, G=G, P=P, L=L)
            assert fixed == 0 and (run == -1) == (G * P * (3 + L) > 256), (case, G, P, L)
        # another attn_in_rows: 12 column groups (768 rows, no gen_tau rows) and 11
        for qkv in (768, 704):
            run, fixed = plans(1, 900, kind, with_front, pair_ok, qkv=qkv)
            assert isinstance(run, list) and fixed == 0, (case, qkv)
    # 900 rows without pair mode (switch off / no fault word / no workspace / too few CUs): the single-workgroup tail on 4-row blocks
    for with_front in (0, 1):
        for pair_ok, cus in ((0, 256), (1, 64), (1, 0)):
            run, fixed = plans(1, 900, TAIL, with_front, pair_ok, cus=cus)
            assert run[:3] == [TAIL, 1, 0] and fixed == 0, (with_front, pair_ok, cus)
    # 8 and 16 rows per workgroup (1025, 2049 rows): no fixed instantiation in this build
    for rows, (kind, with_front, pair_ok) in itertools.product((1025, 2049, 4096), LAUNCHES):
        run, fixed = plans(1, rows, kind, with_front, pair_ok)
        assert isinstance(run, list) and run[2] == 0 and fixed == 0, (rows, kind)
    # not a row-chain config, not a chain
    assert plans(1, 4097, TAIL, 0, 0) == (-1, 0) and plans(1, 900, 3, 0, 0) == (-1, 0) and plans(1, 900, TAIL, 0, 0, classes=65) == (-1, 0)


def test_short_buffer_is_an_error_not_none(plans):
    run, fixed = plans(1, 900, ATT, 0, 0, capacity=47)
    assert len(run) == 48 and fixed == -1
    assert b'sbev_decoder_chain_fixed_plan: 48 words' in _lib.load().sbev_last_error()
    assert plans(1, 900, ATT, 0, 0, capacity=48)[1] == run


def test_switch_round_trip():
    from sparsebev_amd import runtime
    lib = _lib.load()
    prev = runtime.chain_fixed(False)
    try:
        assert lib.sbev_decoder_chain_fixed(1) == 0 and runtime.chain_fixed(True) is True and runtime.chain_fixed(False) is True
    finally:
        runtime.chain_fixed(prev)
    assert bool(lib.sbev_decoder_chain_fixed(int(prev))) == prev
