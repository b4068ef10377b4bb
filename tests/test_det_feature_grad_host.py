"""What the atomics-free feature gradient promises without a GPU: the tap count, the refusals and empty calls of its two entry points
(no row reaches a launch), the process-wide switch, and the host model of the sum against a hand-worked example."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import det_grad_cases as D
from conftest import ROOT
from sparsebev_amd import _lib, ops


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    return _lib.load()


def test_tap_count_table(lib):
    n = lib.sbev_msmv_bwd_tap_count
    assert n(3, 10, 6, 4) == 3 * 10 * 6 * 4 * 4 and n(1, 700, 4, 1) == 11200 and n(32, 900, 4, 4) == 1843200       # config 2: 1.84 M
    assert n(1, 1, 1, 1) == 4 and n(1, 1, 32, 5) == 640
    assert n(0, 10, 6, 4) == 0 and n(3, 0, 6, 4) == 0 and n(3, 10, 0, 4) == 0
    # refusals: negative sizes, P > SBEV_MAX_POINTS, L outside 1..SBEV_MAX_LEVELS, n > INT64_MAX / 4
    assert n(-1, 10, 6, 4) == -1 and n(3, -1, 6, 4) == -1 and n(3, 10, -1, 4) == -1
    assert n(3, 10, 33, 4) == -1 and n(3, 10, 6, 0) == -1 and n(3, 10, 6, 6) == -1 and n(0, 0, 0, 0) == -1
    limit = (2 ** 63 - 1) // 4
    assert n(limit // 4, 1, 1, 1) == (limit // 4) * 4 and n(limit // 4 + 1, 1, 1, 1) == -1
    assert n(2 ** 40, 2 ** 30, 1, 1) == -1 and n(2 ** 62, 1, 1, 1) == -1
    assert n(2 ** 29, 2 ** 30 - 1, 1, 1) == 2 ** 29 * (2 ** 30 - 1) * 4


def _entry_points(lib):
    """sbev_msmv_bwd_taps and sbev_msmv_bwd_sum_sorted as call(**overrides) over one good description (fake pointers: validation returns
    before any HIP call): 4 levels of 4 x 4 pixels, grouped channels-last with B, T, G, N, C, Q, P = 1, 2, 4, 6, 64, 3, 4, mixing layout."""
    M = 6
    base = dict(L=4, hw=[4, 4] * M, B=1, T=2, G=4, N=6, C=64, Q=3, P=4, gdiv=4, feats=[0x1000] * M, gfeats=[0x1000] * M,
                sbo=[6 * 16 * 256] * M, sg=64, sv=[16 * 256] * M, spx=256, ptr=0x1000, layout=1, n=None)

    def args(o):
        d = dict(base, **o)
        d.setdefault('Bp', d['B'] * d['T'] * d['G'])
        if d['n'] is None:
            d['n'] = max(lib.sbev_msmv_bwd_tap_count(d['Bp'], d['Q'], d['P'], d['L']), 0)
        arr = lambda ct, v: None if v is None else (ct * len(v))(*v)
        d.update(feats=arr(ctypes.c_void_p, d['feats']), gfeats=arr(ctypes.c_void_p, d['gfeats']), hw=arr(ctypes.c_int32, d['hw']),
                 sbo=arr(ctypes.c_int64, d['sbo']), sv=arr(ctypes.c_int64, d['sv']), ptr=ctypes.c_void_p(d['ptr']))
        return d

    def taps(**o):
        d = args(o)
        return lib.sbev_msmv_bwd_taps(d['feats'], d['hw'], d['L'], d['Bp'], d['N'], d['C'], d['Q'], d['P'], d['gdiv'], d['sbo'], d['sg'], d['sv'],
                                      d['spx'], d['ptr'], d['ptr'], d['ptr'], d['ptr'], None)

    def total(**o):
        d = args(o)
        return lib.sbev_msmv_bwd_sum_sorted(d['gfeats'], d['L'], d['ptr'], d['ptr'], d['ptr'], d['n'], d['ptr'], d['layout'], d['Bp'], d['C'],
                                            d['Q'], d['P'], d['T'], d['G'], None)

    return {'taps': taps, 'sum': total}


def test_entry_points_refusal_table(lib):
    """Status and message of the two entry points: a refusal names its entry point, an empty call returns 0 before a pointer is looked
    at, a null pointer or a bad layout is -1.  No row reaches a launch."""
    call = _entry_points(lib)
    OK = (0, b'')
    at = lambda l, v, rest: [rest] * l + [v] + [rest] * (5 - l)
    table = [
        (dict(B=0), {'taps': OK, 'sum': OK}),
        (dict(Q=0), {'taps': OK, 'sum': OK}),
        (dict(B=0, ptr=0, feats=at(1, 0, 0x1000), gfeats=at(1, 0, 0x1000)), {'taps': OK, 'sum': OK}),
        (dict(B=0, gfeats=None), {'sum': OK}),
        (dict(hw=None), {'taps': (-1, b'sbev_msmv_bwd_taps: null descriptor array')}),
        (dict(B=0, sbo=None), {'taps': (-1, b'sbev_msmv_bwd_taps: null descriptor array')}),
        (dict(B=0, feats=None), {'taps': (-1, b'sbev_msmv_bwd_taps: null descriptor array')}),
        (dict(L=0), {'taps': (-1, b'sbev_msmv_bwd_taps: L=0 not in 1..5'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: L=0 not in 1..5')}),
        (dict(L=6), {'taps': (-1, b'sbev_msmv_bwd_taps: L=6 not in 1..5'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: L=6 not in 1..5')}),
        (dict(P=33), {'taps': (-1, b'sbev_msmv_bwd_taps: num_point exceed limits (P=33 > 32)'),
                      'sum': (-1, b'sbev_msmv_bwd_sum_sorted: num_point exceed limits (P=33 > 32)')}),
        (dict(P=0), {'taps': (-1, b'sbev_msmv_bwd_taps: num_point exceed limits'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: num_point exceed limits')}),
        (dict(C=0), {'taps': (-1, b'sbev_msmv_bwd_taps: bad sizes'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: bad sizes')}),
        (dict(N=0), {'taps': (-1, b'sbev_msmv_bwd_taps: bad sizes')}),
        (dict(gdiv=0), {'taps': (-1, b'sbev_msmv_bwd_taps: bad sizes')}),
        (dict(Q=-1), {'taps': (-1, b'sbev_msmv_bwd_taps: bad sizes'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: bad sizes')}),
        (dict(Bp=2 ** 61), {'taps': (-1, b"sbev_msmv_bwd_taps: B'*Q*P*L*4 too large")}),
        (dict(ptr=0), {'taps': (-1, b'sbev_msmv_bwd_taps: null pointer'), 'sum': (-1, b'sbev_msmv_bwd_sum_sorted: null pointer')}),
        (dict(gfeats=None), {'sum': (-1, b'sbev_msmv_bwd_sum_sorted: null pointer')}),
        (dict(gfeats=at(2, 0, 0x1000)), {'sum': (-1, b'sbev_msmv_bwd_sum_sorted: level 2 pointer is null')}),
        (dict(feats=at(1, 0, 0x1000), B=0), {'taps': OK}),                # feature VALUES are not read: their pointers are not asked for
        (dict(layout=7), {'sum': (-1, b'sbev_msmv_bwd_sum_sorted: grad_out_layout 7')}),
        (dict(Bp=7), {'sum': (-1, b"sbev_msmv_bwd_sum_sorted: B'=7 is not B*T*G (T=2, G=4)")}),
        (dict(Bp=7, Q=0, layout=0), {'sum': OK}),                         # reference layout: T and G are not read
        (dict(Bp=8, T=0), {'sum': (-1, b"sbev_msmv_bwd_sum_sorted: B'=8 is not B*T*G")}),
        (dict(n=100), {'sum': (-1, b"sbev_msmv_bwd_sum_sorted: n=100 is not B'*Q*P*L*4 = 1536")}),
        (dict(B=0, n=4), {'sum': (-1, b"sbev_msmv_bwd_sum_sorted: n=4 is not B'*Q*P*L*4 = 0")}),
        # one writer per destination row: rows may not overlap, offsets are non-negative and fit the key's 56 bits
        (dict(spx=32), {'taps': (-1, b'sbev_msmv_bwd_taps: pixel / group strides must be >= C=64')}),
        (dict(sg=32), {'taps': (-1, b'sbev_msmv_bwd_taps: pixel / group strides must be >= C=64')}),
        (dict(sv=at(1, -4096, 4096)), {'taps': (-1, b'sbev_msmv_bwd_taps: level 1 has a negative stride')}),
        (dict(hw=[4, 4, 0, 4] + [4, 4] * 4), {'taps': (-1, b'sbev_msmv_bwd_taps: level 1 has empty map')}),
        (dict(sbo=at(3, 2 ** 56, 6 * 4096)), {'taps': (-1, b'sbev_msmv_bwd_taps: level 3: offsets do not fit 56 bits')}),
        (dict(B=1 << 30, Q=1 << 20, P=1, L=1), {'taps': (-1, b"sbev_msmv_bwd_taps: B'*Q too large"),
                                               'sum': (-1, b'sbev_msmv_bwd_sum_sorted: n=36028797018963968 too large for one launch')}),
    ]
    for overrides, expected in table:
        for name, (status, text) in expected.items():
            got = call[name](**overrides)
            err = lib.sbev_last_error() if got != 0 else b''
            assert got == status and text in err, (name, overrides, got, err)


def test_switch_returns_the_previous_setting_and_follows_torch():
    start = ops.deterministic_feature_grad()
    try:
        assert ops.deterministic_feature_grad(True) == start
        assert ops.deterministic_feature_grad() is True and ops.deterministic_feature_grad_active()
        assert ops.deterministic_feature_grad(False) is True
        assert ops.deterministic_feature_grad(None) is False and ops.deterministic_feature_grad() is False        # a query changes nothing
        before = torch.are_deterministic_algorithms_enabled()
        try:
            torch.use_deterministic_algorithms(False)
            assert not ops.deterministic_feature_grad_active()
            torch.use_deterministic_algorithms(True)
            assert ops.deterministic_feature_grad_active() and ops.deterministic_feature_grad() is False          # the mode, not the switch
        finally:
            torch.use_deterministic_algorithms(before)
    finally:
        ops.deterministic_feature_grad(start)


@pytest.mark.parametrize('value,expected', [(None, False), ('0', False), ('1', True)])
def test_switch_default_follows_the_environment(value, expected):
    env = {k: v for k, v in os.environ.items() if k != 'SBEV_DET_FEAT_GRAD'}
    if value is not None:
        env['SBEV_DET_FEAT_GRAD'] = value
    code = 'import sys; sys.path.insert(0, %r); from sparsebev_amd import ops; print(ops.deterministic_feature_grad())' % ROOT
    out = subprocess.check_output([sys.executable, '-c', code], env=env).decode().split()[-1]
    assert out == str(expected)


def test_host_model_on_a_hand_worked_three_tap_example():
    """L = 1, C = 2, two points (8 taps).  Destination A (offset 4) collects taps 0, 4, 5, destination B (offset 0) tap 2; the others are
    dead.  Channel 0 of A: ((+0 + 2^24) + 1) + (-1): 2^24 + 1 ties to even = 2^24, minus 1 = 16777215 -- back to front it would be
    (-1 + 1) + 2^24 = 2^24.  Channel 1: (1 + 2^-24) ties to 1, minus 2^-24 = 1 - 2^-24 -- back to front exactly 1.  Then ONE addition
    into the buffer: 0.5 + 16777215 = 16777215.5 ties to even = 16777216."""
    A, B_ = np.int64(4), np.int64(0)
    keys = np.array([A, D.KEY_DEAD, B_, D.KEY_DEAD, A, A, D.KEY_DEAD, D.KEY_DEAD], dtype=np.int64)
    coefs = np.array([1.0, 0.0, 0.25, 0.0, 1.0, -1.0, 0.0, 0.0], dtype=np.float32)
    rows = np.array([[2.0 ** 24, 1.0], [1.0, 2.0 ** -24]], dtype=np.float32)
    buf = np.array([10.0, 20.0, 7.0, 7.0, 0.5, 0.0, 7.0], dtype=np.float32)
    out, = D.host_feature_grad(keys, coefs, rows, [buf], L=1)
    want = np.array([10.0 + 2.0 ** 22, 20.25, 7.0, 7.0, 16777216.0, 1.0 - 2.0 ** -24, 7.0], dtype=np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, want), out
    assert buf[4] == 0.5                                              # the input buffers are left alone
    back, = D.host_feature_grad(keys, coefs, rows, [buf], L=1, descending=True)
    assert back[4] == np.float32(2.0 ** 24) and back[5] == np.float32(1.0)          # the other order is another result
    # a level above 0 lands in its own buffer
    keys2 = np.where(keys == D.KEY_DEAD, keys, keys | (np.int64(1) << D.LEVEL_SHIFT))
    o0, o1 = D.host_feature_grad(keys2, coefs, rows, [np.zeros(3, np.float32), buf], L=1)
    assert np.array_equal(o1, want) and not o0.any()


def test_restated_geometry_on_hand_worked_points():
    """ref_taps at the two exact points of the cases: (0, 1) is the bottom-left pixel with weight 1 on corner (0, 0) -- the corners
    beyond the last row are outside the map --, (0.5, 0.5) on a 3 x 4 level is h = 1, w = 1.5: all four corners are inside, the two of row 1 weigh 0.5 each."""
    loc = torch.tensor([[[[0.0, 1.0, 0.2]], [[0.5, 0.5, 1.0]], [[float('nan'), 0.5, 0.0]], [[0.5, 0.5, 1.1 / 5]]]])      # [1, 4, 1, 3]
    wts = torch.tensor([0.25, 1.0, 1.0, 1.0]).reshape(1, 4, 1, 1)
    H, W, C, Nv = 3, 4, 8, 6
    keys, coefs = D.ref_taps(loc, wts, [(H, W)], Nv, 1, [Nv * H * W * C], 0, [H * W * C], C)
    px = lambda view, h, w: (view * H * W + h * W + w) * C
    dead = int(D.KEY_DEAD)
    assert keys.tolist() == [px(1, 2, 0), px(1, 2, 1), dead, dead,                     # (0, 1): h = 2 exactly, w = 0; row 3 is outside
                             px(5, 1, 1), px(5, 1, 2), px(5, 2, 1), px(5, 2, 2),       # (0.5, 0.5), last view
                             dead, dead, dead, dead,                                   # NaN: no tap is live
                             px(1, 1, 1), px(1, 1, 2), px(1, 2, 1), px(1, 2, 2)]       # z = 0.22: round(1.1) = view 1
    assert coefs.tolist() == [0.25, 0.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0]
