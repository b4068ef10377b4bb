"""sbev_linear_gen_plan: what a generator GEMM call launches -- kernel, row split, grids, LDS bytes, column ranges -- is a pure host
function of the shape.  Checked here, without a GPU, against an independent restatement of the arithmetic the launcher carried inline
before the plan existed, against the properties every plan must have, and against three anchors worked out by hand."""
import ctypes
import itertools
import os

import pytest

from sparsebev_amd import _lib

MS = (1, 31, 32, 33, 97, 129, 257, 900, 1600, 3200, 3600, 65536)
NS = (256, 512, 1024, 4352, 32768, 77824)
KS = (32, 96, 256, 288)
NIMGS = (2, 3, 4, 5)
CUS = (256, 64)
LDS_BUDGET = 160 * 1024
WS_LDS = 4 * 16 * 2 * 1024          # 4 ring slots x one X fragment: 16 k-steps x 2 images x 1 KiB


@pytest.fixture(scope='module')
def plan():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    lib = _lib.load()
    buf = (ctypes.c_int32 * 4096)()

    def call(M, N, K, nimg, ws, cus, ldy=None, capacity=4096):
        n = lib.sbev_linear_gen_plan(M, N, K, N if ldy is None else ldy, nimg, int(ws), cus, buf, capacity)
        if n < 0:
            return n
        w = list(buf[:n])
        assert n == 7 + 4 * w[6]
        return dict(kernel=w[0], ntm=w[1], base=w[2], rem=w[3], a=w[4], tiles_per_wg=w[5],
                    launches=[tuple(w[7 + 4 * i:11 + 4 * i]) for i in range(w[6])])
    return call


def tiled_lds(images, rf):
    """ring + patch bytes of the tiled kernel, from its layout: 3 stages (4 with 128-row tiles) of (2 rf row + 8 column) fragments of
    1 KiB per image; two images with 256-row tiles: 8 per-wave transpose patches of 32 rows x 36 floats"""
    ring = (4 if rf == 2 else 3) * images * (2 * rf + 8) * 1024
    return ring + (8 * 32 * 36 * 4 if images == 2 and rf == 4 else 0)


def restated(M, N, K, ldy, nimg, ws_switch, cus):
    """The launcher's inline arithmetic of the commit before the plan was factored out, written again from its text."""
    nfrag = (M + 31) // 32
    nct = N // 256
    if ws_switch and K == 256 and nimg != 3 and M * ldy * 4 < 0x7fffffff:
        nrs, best = 1, 1e30
        for r in range(1, min(16, nfrag) + 1):
            tasks = nct * r
            cost = float((tasks + cus - 1) // cus) * ((nfrag + r - 1) // r + 4.0)
            if cost < best - 1e-9:
                best, nrs = cost, r
        ntask = nct * nrs
        return dict(kernel=0, ntm=nrs, base=nfrag // nrs, rem=nfrag % nrs, a=ntask, tiles_per_wg=0,
                    launches=[(0, nct, min(ntask, cus), WS_LDS)])
    forced = int(os.environ.get('SBEV_BF16S_GEN_RF', '0') or 0)
    rf = forced if forced in (2, 4) else (4 if nfrag > 4 else 2)
    tf = 2 * rf
    ntm = (nfrag + tf - 1) // tf
    nim = 3 if nimg == 3 else 2
    per = min(max(cus // ntm, 1), nct)
    nst = 4 if rf == 2 else 3
    ring_bytes = nst * nim * (tf + 8) * 1024 + (8 * 32 * 36 * 4 if nim == 2 and rf == 4 else 0)
    per_tile = 256 * 4 * (2 if nimg >= 4 else 1)
    tiles_per_wg = min((160 * 1024 - ring_bytes) // per_tile, 16)
    max_ct = per * tiles_per_wg
    launches = []
    for c0 in range(0, nct, max_ct):
        nc = min(nct - c0, max_ct)
        pc = min(per, nc)
        launches.append((c0, nc, pc * ntm, ring_bytes + (nc + pc - 1) // pc * per_tile))
    return dict(kernel=rf, ntm=ntm, base=nfrag // ntm, rem=nfrag % ntm, a=per, tiles_per_wg=tiles_per_wg, launches=launches)


def test_plan_equals_the_restated_arithmetic_and_covers_the_matrix(plan):
    """Over M x N x K x nimg x switch x CUs (4608 shapes): every field equals the restatement; the row split covers fragments
    0 .. ceil(M/32) - 1 exactly once; the column ranges cover the N / 256 tiles exactly once; a launch's LDS bytes are ring + patch +
    the slices of the column tiles a workgroup walks, within 160 KiB; every grid is >= 1 and <= the CUs.
    "<= the CUs" and "a multiple of ntm" (tiled) cannot both hold for ANY plan where ntm > cus: the tiled kernel keeps one row tile
    per workgroup for life, so it needs ntm workgroups at least (here M = 65536: 256 row tiles on 64 CUs; an MI355X has 256).  There
    the grid must be exactly ntm -- the smallest the kernel allows; everywhere else it is <= cus as stated."""
    n = 0
    for M, N, K, nimg, ws, cus in itertools.product(MS, NS, KS, NIMGS, (True, False), CUS):
        p = plan(M, N, K, nimg, ws, cus)
        case = (M, N, K, nimg, ws, cus)
        assert p == restated(M, N, K, N, nimg, ws, cus), (case, p)
        nfrag, nct = (M + 31) // 32, N // 256
        first = lambda i: i * p['base'] + min(i, p['rem'])
        count = lambda i: p['base'] + (1 if i < p['rem'] else 0)
        frags = [f for i in range(p['ntm']) for f in range(first(i), first(i) + count(i))]
        assert frags == list(range(nfrag)), case
        tiles = [c for c0, nc, _, _ in p['launches'] for c in range(c0, c0 + nc)]
        assert tiles == list(range(nct)), case
        f16 = nimg >= 4
        if p['kernel'] == 0:
            assert ws and K == 256 and nimg != 3, case
            assert p['a'] == nct * p['ntm'] and len(p['launches']) == 1, case
            (_, _, grid, lds), = p['launches']
            assert lds == WS_LDS <= LDS_BUDGET and 1 <= grid <= cus and grid <= p['a'], case
        else:
            assert p['kernel'] == (4 if nfrag > 4 else 2) and count(0) <= 2 * p['kernel'], case
            fixed = tiled_lds(3 if nimg == 3 else 2, p['kernel'])
            for c0, nc, grid, lds in p['launches']:
                assert grid >= 1 and grid % p['ntm'] == 0, case
                assert grid <= cus or grid == p['ntm'], case
                walked = -(-nc // (grid // p['ntm']))                 # column tiles of the busiest workgroup
                assert walked <= p['tiles_per_wg'] <= 16, case
                assert lds == fixed + walked * 256 * 4 * (2 if f16 else 1) <= LDS_BUDGET, case
        n += 1
    assert n == 12 * 6 * 4 * 4 * 2 * 2


def test_plan_anchors(plan):
    """Three plans derived by hand from the launcher's code, as literals."""
    # weight-stationary, c2: 29 fragments in 2 splits of 15 / 14, 128 column tiles x 2 = 256 tasks on 256 CUs, the 4-slot X ring
    assert plan(900, 32768, 256, 4, True, 256) == dict(kernel=0, ntm=2, base=14, rem=1, a=256, tiles_per_wg=0,
                                                       launches=[(0, 128, 256, 131072)])
    # tiled, 256-row tiles, three images: 4 row tiles of 8 / 7 / 7 / 7 fragments x 64 workgroups each, two bias slices of 1 KiB
    assert plan(900, 32768, 256, 3, True, 256) == dict(kernel=4, ntm=4, base=7, rem=1, a=64, tiles_per_wg=16,
                                                       launches=[(0, 128, 256, 147456 + 2048)])
    # 256 row tiles leave one workgroup per row tile, which holds the slices of 16 column tiles: 17 tiles take two launches.
    # (Planned only: launched, this shape writes 1.1 GB.)
    assert plan(65536, 4352, 256, 3, True, 256) == dict(kernel=4, ntm=256, base=8, rem=0, a=1, tiles_per_wg=16,
                                                        launches=[(0, 16, 256, 147456 + 16 * 1024), (16, 1, 256, 147456 + 1024)])


def test_plan_refuses_uncovered_shapes_and_short_buffers(plan):
    assert plan(900, 32768 + 128, 256, 4, True, 256) == -1          # N % 256
    assert plan(900, 32768, 250, 4, True, 256) == -1                # K % 32
    assert plan(0, 32768, 256, 4, True, 256) == -1 and plan(900, 32768, 256, 6, True, 256) == -1
    assert plan(900, 32768, 256, 4, True, 256, ldy=32764) == -1     # ldy < N
    assert plan(900, 32768, 256, 4, True, 256, capacity=10) == -1   # 11 words needed
    assert b'11 words' in _lib.load().sbev_last_error()
    assert plan(900, 32768, 256, 4, True, 256, capacity=11)['launches'] == [(0, 128, 256, 131072)]
    assert plan(900, 32768, 256, 4, True, 0)['kernel'] == 0         # cus = 0: the device's count, 256 where there is none to ask
