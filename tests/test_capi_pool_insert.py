"""Refusal table of sbev_pool_insert without a GPU: fake aligned pointers, validation returns before any HIP call; an accepted row is an
empty call (B = 0)."""
import ctypes
import os

import pytest

from sparsebev_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    return _lib.load()


def caller(lib):
    """call(**overrides) over one description: 4 levels (the tiny pyramid's pixel counts), direct sources at fake 16-byte aligned
    addresses, fp32, 4 slots, 6 views, 256 channels, B = 0"""
    base = dict(table=None, index=None, src=[0x1000, 0x2000, 0x3000, 0x4000], out=[0x10000, 0x20000, 0x30000, 0x40000], L=4,
                hw=[176, 44, 12, 3], B=0, views=6, C=256, dtype=0, insert=0x5000, n_slots=4)

    def call(**o):
        d = dict(base, **o)
        arr = lambda ct, v: None if v is None else (ct * len(v))(*v)
        vp = lambda v: None if v is None else ctypes.c_void_p(v)
        return lib.sbev_pool_insert(vp(d['table']), arr(ctypes.c_int32, d['index']), arr(ctypes.c_void_p, d['src']), arr(ctypes.c_void_p, d['out']),
                                    d['L'], arr(ctypes.c_int32, d['hw']), d['B'], d['views'], d['C'], d['dtype'], vp(d['insert']), d['n_slots'], None)

    return call


def test_pool_insert_is_declared_last_and_the_abi_stays_1(lib):
    from conftest import ROOT
    text = open(os.path.join(ROOT, 'include', 'sbev_hip.h')).read()
    assert text.rindex('int sbev_pool_insert(') > max(text.rindex('int %s(' % n) for n in ('sbev_profile_read', 'sbev_graph_destroy', 'sbev_nchw_to_nhwc_lazy'))
    assert lib.sbev_abi_version() == 1 and '#define SBEV_ABI_VERSION 1' in text
    assert list(_lib.SIGNATURES)[-1] == 'sbev_pool_insert'


def test_pool_insert_refusal_table(lib):
    call = caller(lib)
    OK = (0, b'')
    indirect = dict(table=0x8000, index=[3, 4, 5, 6], src=None)
    table = [
        # accepted: empty calls, both source forms, every storage type, one level, the most levels, odd sizes
        (dict(), OK),
        (indirect, OK),
        (dict(dtype=1), OK), (dict(dtype=2), OK), (dict(indirect, dtype=2), OK),
        (dict(L=1), OK),
        (dict(L=5, src=[0x1000] * 5, out=[0x10000] * 5, hw=[704, 176, 44, 12, 3]), OK),
        (dict(C=7, hw=[5, 3, 2, 1]), OK),
        (dict(n_slots=1), OK),
        # null pointers
        (dict(out=None), (-1, b'sbev_pool_insert: null pointer')),
        (dict(hw=None), (-1, b'sbev_pool_insert: null pointer')),
        (dict(insert=None), (-1, b'sbev_pool_insert: null pointer')),
        (dict(table=0x8000, index=None, src=None), (-1, b'sbev_pool_insert: null pointer (table without index)')),
        (dict(src=[0x1000, 0, 0x3000, 0x4000]), (-1, b'sbev_pool_insert: level 1 ')),
        (dict(out=[0x10000, 0x20000, 0, 0x40000]), (-1, b'sbev_pool_insert: level 2 ')),
        # L outside 1 .. SBEV_MAX_LEVELS
        (dict(L=0), (-1, b'sbev_pool_insert: L=0 not in 1..5')),
        (dict(L=6), (-1, b'sbev_pool_insert: L=6 not in 1..5')),
        (dict(L=-1), (-1, b'sbev_pool_insert: L=-1 not in 1..5')),
        # n_slots < 1
        (dict(n_slots=0), (-1, b'sbev_pool_insert: n_slots must be at least 1 (got 0)')),
        (dict(n_slots=-3), (-1, b'sbev_pool_insert: n_slots must be at least 1 (got -3)')),
        # dtype code
        (dict(dtype=3), (-1, b'sbev_pool_insert: dtype 3')),
        (dict(dtype=-1), (-1, b'sbev_pool_insert: dtype -1')),
        # the source given both ways, or neither
        (dict(table=0x8000, index=[3, 4, 5, 6]), (-1, b'sbev_pool_insert: give the sources as table + index or as src, not both')),
        (dict(src=None), (-1, b'sbev_pool_insert: give the sources as table + index or as src, not neither')),
        (dict(src=None, index=[3, 4, 5, 6]), (-1, b'not neither')),
        # alignment and sizes
        (dict(indirect, table=0x8004), (-1, b'sbev_pool_insert: unaligned pointer table')),
        (dict(insert=0x5002), (-1, b'sbev_pool_insert: insert must be 4-byte aligned')),
        (dict(src=[0x1000, 0x2008, 0x3000, 0x4000]), (-1, b'sbev_pool_insert: level 1 ')),
        (dict(out=[0x10004, 0x20000, 0x30000, 0x40000]), (-1, b'sbev_pool_insert: level 0 ')),
        (dict(indirect, index=[3, 4, -1, 6]), (-1, b'sbev_pool_insert: level 2 ')),
        (dict(hw=[176, 44, 0, 3]), (-1, b'sbev_pool_insert: level 2 ')),
        (dict(B=-1), (-1, b'sbev_pool_insert: bad sizes')),
        (dict(C=0), (-1, b'sbev_pool_insert: bad sizes')),
        (dict(views=0), (-1, b'sbev_pool_insert: bad sizes')),
        (dict(hw=[1 << 30, 44, 12, 3]), (-1, b'sbev_pool_insert: level 0: plane too large')),
        # refused although the call is empty: validation does not depend on B
        (dict(B=0, n_slots=0), (-1, b'n_slots must be at least 1')),
    ]
    for overrides, (status, text) in table:
        got = call(**overrides)
        err = lib.sbev_last_error() if got != 0 else b''
        assert got == status and text in err, (overrides, got, err)
