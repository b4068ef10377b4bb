"""Several frames per step, host side, without a GPU: SlotBook.plan_frames against missing + assign + table over seeded random streams,
and the refusal table of sbev_pool_insert_frames (fake aligned pointers, validation returns before any HIP call; an accepted row is an
empty call, B = 0)."""
import ctypes
import os
import random

import pytest

from sparsebev_amd import _lib
from sparsebev_amd.cache import SlotBook

T = 4


def snapshot(book):
    return book.B, {b: list(m.items()) for b, m in book.slots.items()}, {b: list(k) for b, k in book.needed.items()}


class Streams:
    """B independent streams of windows [T] of keys, newest first: scene changes either start with a window padded by duplicates (the
    scene's first frame repeated) or with ``span`` distinct frames at once; a step may repeat the one before it.  A window holds at most
    ``span`` distinct keys (the oldest repeated), so that a pool of fewer than T slots is exercised too."""

    def __init__(self, rng, B, span):
        self.rng, self.B, self.span = rng, B, span
        self.state = [dict(scene=0, n=0, first=0) for _ in range(B)]

    def step(self):
        keys = []
        for b, s in enumerate(self.state):
            if self.rng.random() < 0.85 or s['n'] == 0:                             # else: the step before, repeated
                s['n'] += 1
            if self.rng.random() < 0.15:
                s['scene'] += 1
                s['first'] = s['n'] if self.rng.random() < 0.5 else s['n'] - T       # padded window, or T distinct frames at once
            keys.append([(b, s['scene'], max(s['n'] - t, s['first'], s['n'] - self.span + 1)) for t in range(T)])
        return keys


def lowest_positions(keys, missing):
    return {next(t for t in range(T) if keys[b][t] == k) for b, k in missing}


@pytest.mark.parametrize('n_slots', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('B', [1, 2, 3])
def test_plan_frames_equals_missing_assign_table(B, n_slots):
    rng = random.Random(100 * B + n_slots)
    ref, book = SlotBook(T, n_slots), SlotBook(T, n_slots)
    streams = Streams(rng, B, min(T, n_slots))
    planned = refused = multi = once = keyerrors = 0
    for step in range(120):
        keys = streams.step()
        before = snapshot(book)
        if n_slots < T and rng.random() < 0.2:                           # more distinct keys than slots: raises, the book unchanged
            wide = [list(row) for row in keys]
            wide[rng.randrange(B)] = [('wide', step, t) for t in range(T)]
            with pytest.raises(RuntimeError, match='distinct frames'):
                book.plan_frames(wide, range(T))
            assert snapshot(book) == before
            refused += 1
        miss = ref.missing(keys)
        need = lowest_positions(keys, miss)
        if need:                                                         # a missing key whose positions are not offered: KeyError, the book unchanged
            b0, k0 = miss[rng.randrange(len(miss))]
            short = [t for t in range(T) if keys[b0][t] != k0]
            with pytest.raises(KeyError if short else ValueError):       # (a key at every position leaves no other position to offer)
                book.plan_frames(keys, short)
            assert snapshot(book) == before
            keyerrors += bool(short)
            with pytest.raises(ValueError):
                book.plan_frames(keys, [])
            assert snapshot(book) == before
        # offered: what the step lacks, at the lowest or at EVERY position that carries it, plus positions nobody lacks
        offered = set(need)
        if rng.random() < 0.5:
            offered |= {t for b, k in miss for t in range(T) if keys[b][t] == k}
        offered |= {t for t in range(T) if rng.random() < 0.3}
        offered = sorted(offered or {0})
        want_slot = {(b, k): ref.assign(b, k)[0] for b, k in miss}
        want_rows = ref.table(keys)
        rows, insert = book.plan_frames(keys, rng.sample(offered, len(offered)))         # (any order in, ascending t out)
        assert rows == want_rows and snapshot(book)[:2] == snapshot(ref)[:2]
        assert len(insert) == len(offered) and all(len(r) == B for r in insert)
        got_slot = {}
        for i, t in enumerate(offered):
            for b in range(B):
                if insert[i][b] >= 0:
                    assert (b, keys[b][t]) not in got_slot               # a key at several offered positions is inserted once ...
                    assert t == min(u for u in offered if keys[b][u] == keys[b][t])      # ... at the lowest of them
                    got_slot[(b, keys[b][t])] = insert[i][b]
        assert got_slot == want_slot
        for b in range(B):
            live = [insert[i][b] for i in range(len(offered)) if insert[i][b] >= 0]
            assert len(live) == len(set(live)) and all(0 <= s < n_slots for s in live)   # no two live inserts of a sample share a slot
            assert all(k in book.slots[b] for k in keys[b])              # no needed key was evicted
            assert [book.slots[b][k] for k in keys[b]] == rows[b]
            multi += len(live) > 1
        once += sum(1 for b, k in miss if sum(1 for t in offered if keys[b][t] == k) > 1)
        planned += 1
    # the stream reached what it is here for
    assert planned == 120 and once > 0 and keyerrors > 5 and (multi > 0 or n_slots < 3) and (refused > 5 or n_slots >= T)


def test_plan_frames_against_plan_step():
    """with only the newest position offered it is plan_step"""
    a, b = SlotBook(T, 5), SlotBook(T, 5)
    for n in range(8):
        keys = [[('a', max(n - t, 0)) for t in range(T)], [('b', max(n - t, 0)) for t in range(T)]]
        rows, insert = a.plan_frames(keys, [0])
        assert (rows, insert[0]) == b.plan_step(keys) and len(insert) == 1
    with pytest.raises(ValueError):
        a.plan_frames(keys, [T])
    with pytest.raises(ValueError):
        a.plan_frames(keys, [-1, 0])


def test_step_key_holds_k_shapes_dtype_layout_and_the_rows_address_not_the_frames():
    """what a captured step of FramePool.stream is keyed on (StepGraphs._feat_key), on host tensors: fresh frames of one shape give one
    key; K, dtype, layout and the rows' address each give another; FramePool.step's form of the insert -- the insert row viewed as [1, B] --
    gives the key of stream()'s K = 1 form: the same address, one graph"""
    import torch
    from sparsebev_amd.runtime import StepGraphs
    from sparsebev_amd.utils import FrameInsert, frame_source

    class Pyr:
        pass

    level, table, rows = torch.zeros(2 * 4 * 6, 2, 3, 8), torch.zeros(2, T, dtype=torch.int32), torch.zeros(T, 2, dtype=torch.int32)
    other_rows = torch.zeros(T, 2, dtype=torch.int32)

    def key(K=1, nhwc=False, dtype=torch.float32, rows=rows, step=False):
        pyr = Pyr()
        pyr.levels, pyr.slot_table, pyr.n_slots = [level], table, 4
        frames = [torch.zeros(2, 6, 8, 2, 3, dtype=dtype) for _ in range(K)]          # new tensors every call
        pyr.insert = FrameInsert(frames, rows[0].view(1, -1) if step else rows[:K], nhwc)
        src = frame_source(pyr)
        assert src.kind == 'pool' and src.insert is pyr.insert
        part, ident, staged = StepGraphs._feat_key(None, pyr, src)
        assert ident == [] and staged is False
        return part

    assert key() == key() and key(K=3) == key(K=3)
    assert key(step=True) == key()
    distinct = [key(), key(K=3), key(nhwc=True), key(dtype=torch.float16), key(rows=other_rows)]
    assert len(set(distinct)) == len(distinct)
    assert FrameInsert([], rows[:3], True).K == 3


# ---- the C entry -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    return _lib.load()


def caller(lib):
    """call(**overrides) over one description: K = 2 frame sets of 4 levels (the tiny pyramid's pixel counts), direct sources at fake
    16-byte aligned addresses, NCHW, fp32 -> fp32, 4 slots, 6 views, 256 channels, B = 0"""
    base = dict(table=None, index=None, src=[0x1000 * (i + 1) for i in range(8)], out=[0x10000, 0x20000, 0x30000, 0x40000], K=2, L=4,
                hw=[176, 44, 12, 3], B=0, views=6, C=256, layout=0, sdt=0, ddt=0, insert=0x5000, n_slots=4)

    def call(**o):
        d = dict(base, **o)
        arr = lambda ct, v: None if v is None else (ct * len(v))(*v)
        vp = lambda v: None if v is None else ctypes.c_void_p(v)
        return lib.sbev_pool_insert_frames(vp(d['table']), arr(ctypes.c_int32, d['index']), arr(ctypes.c_void_p, d['src']), arr(ctypes.c_void_p, d['out']),
                                           d['K'], d['L'], arr(ctypes.c_int32, d['hw']), d['B'], d['views'], d['C'], d['layout'], d['sdt'], d['ddt'],
                                           vp(d['insert']), d['n_slots'], None)

    return call


def test_pool_insert_frames_is_declared_and_the_abi_stays_1(lib):
    from conftest import ROOT
    text = open(os.path.join(ROOT, 'include', 'sbev_hip.h')).read()
    assert 'int sbev_pool_insert_frames(' in text and 'enum sbev_frames_layout { SBEV_FRAMES_NCHW = 0, SBEV_FRAMES_NHWC = 1 }' in text
    assert lib.sbev_abi_version() == 1 and '#define SBEV_ABI_VERSION 1' in text
    res, args = _lib.SIGNATURES['sbev_pool_insert_frames']
    assert res is ctypes.c_int and len(args) == 16
    assert lib.sbev_pool_insert_frames.argtypes == args


def test_pool_insert_frames_refusal_table(lib):
    call = caller(lib)
    OK = (0, b'')
    P = b'sbev_pool_insert_frames: '
    indirect = dict(table=0x8000, index=list(range(3, 11)), src=None)
    many = dict(K=16, L=5, src=[0x1000] * 80, out=[0x10000] * 5, hw=[704, 176, 44, 12, 3])
    narrow = b'nothing is narrowed'
    table = [
        # accepted: empty calls, both source forms, both layouts, every type pair the kernel has, one set, the most sets and levels, odd sizes
        (dict(), OK), (indirect, OK), (dict(layout=1), OK), (dict(indirect, layout=1), OK),
        (dict(sdt=1, ddt=1), OK), (dict(sdt=2, ddt=2), OK), (dict(sdt=1, ddt=0), OK), (dict(sdt=2, ddt=0), OK), (dict(sdt=2, ddt=0, layout=1), OK),
        (dict(K=1, src=[0x1000] * 4), OK), (many, OK), (dict(many, src=None, table=0x8000, index=list(range(3, 83))), OK),
        (dict(C=7, hw=[5, 3, 2, 1]), OK), (dict(C=7, hw=[5, 3, 2, 1], layout=1, sdt=1, ddt=0), OK), (dict(n_slots=1), OK),
        # K outside 1 .. SBEV_MAX_FRAMES, L outside 1 .. SBEV_MAX_LEVELS
        (dict(K=0), (-1, P + b'K=0 not in 1..16')), (dict(K=17), (-1, P + b'K=17 not in 1..16')), (dict(K=-1), (-1, P + b'K=-1 not in 1..16')),
        (dict(L=0), (-1, P + b'L=0 not in 1..5')), (dict(L=6), (-1, P + b'L=6 not in 1..5')),
        # the source given both ways, or neither
        (dict(table=0x8000, index=list(range(3, 11))), (-1, P + b'give the sources as table + index or as src, not both')),
        (dict(src=None), (-1, P + b'give the sources as table + index or as src, not neither')),
        (dict(src=None, index=list(range(3, 11))), (-1, b'not neither')),
        (dict(table=0x8000, index=None, src=None), (-1, P + b'null pointer (table without index)')),
        # lossy type pairs: fp32 into 2-byte slots, one 2-byte type into the other
        (dict(sdt=0, ddt=1), (-1, narrow)), (dict(sdt=0, ddt=2), (-1, narrow)), (dict(sdt=0, ddt=2, layout=1), (-1, narrow)),
        (dict(sdt=1, ddt=2), (-1, narrow)), (dict(sdt=2, ddt=1), (-1, narrow)),
        (dict(sdt=3), (-1, P + b'src_dtype 3')), (dict(ddt=-1), (-1, P + b'dst_dtype -1')), (dict(layout=2), (-1, P + b'src_layout 2')),
        # null and misaligned pointers
        (dict(out=None), (-1, P + b'null pointer')), (dict(hw=None), (-1, P + b'null pointer')), (dict(insert=None), (-1, P + b'null pointer')),
        (dict(src=[0x1000] * 5 + [0] + [0x1000] * 2), (-1, P + b'frame set 1 level 1 ')),
        (dict(src=[0x1000] * 3 + [0x4008] + [0x1000] * 4), (-1, P + b'frame set 0 level 3 ')),
        (dict(src=[0x1000] * 7 + [0x8004]), (-1, P + b'frame set 1 level 3 ')),
        (dict(out=[0x10000, 0x20000, 0, 0x40000]), (-1, P + b'level 2 ')),
        (dict(out=[0x10004, 0x20000, 0x30000, 0x40000]), (-1, P + b'level 0 ')),
        (dict(indirect, table=0x8004), (-1, P + b'unaligned pointer table')),
        (dict(indirect, index=[3, 4, 5, 6, 7, -1, 9, 10]), (-1, P + b'frame set 1 level 1 ')),
        (dict(insert=0x5002), (-1, P + b'insert must be 4-byte aligned')),
        # sizes
        (dict(hw=[176, 44, 0, 3]), (-1, P + b'level 2 ')), (dict(B=-1), (-1, P + b'bad sizes')), (dict(C=0), (-1, P + b'bad sizes')),
        (dict(views=0), (-1, P + b'bad sizes')), (dict(hw=[1 << 30, 44, 12, 3]), (-1, P + b'level 0: frame too large')),
        (dict(n_slots=0), (-1, P + b'n_slots must be at least 1 (got 0)')),
    ]
    for overrides, (status, text) in table:
        got = call(**overrides)
        err = lib.sbev_last_error() if got != 0 else b''
        assert got == status and text in err, (overrides, got, err)
