"""sbev_decoder_chain_plan: what a row-chain launch does -- instantiation, grid, LDS bytes, both pair members' unit tables, warm span,
small-vector range -- is a pure host function of the config.  Checked here, without a GPU, against an independent restatement of the
arithmetic launch_chain_front / launch_chain_attn / launch_chain_tail carried inline before the plan existed, against the properties
every plan must have, and against three anchors worked out by hand."""
import ctypes
import itertools
import os

import pytest

from sparsebev_amd import _lib

ROWS = (1, 4, 9, 900, 1024, 1025, 1600, 2048, 2049, 3600, 4096)
BQ = [(b, r // b) for r in ROWS for b in (1, 2) if r % b == 0]
CLASSES = (1, 10, 64)
QKV_ROWS = (768, 769, 832)
GPL = ((4, 2, 4), (4, 4, 4), (4, 8, 5))          # G P (3 + L) = 56, 112, 256
CUS = (256, 64, 0)
TAIL, FRONT, ATT = 0, 1, 2                       # kind = the kernels' Pre
D, FFN, CODE = 256, 512, 10
LDX, LDH = D + 8, FFN + 8
FFN0, FFN1, BR1, BR2, OUT, PE3, QKV, AOUT, SAMP = range(9)       # epilogues
NONE = (-1, 0, LDX, 1, 0, 8, 0, 1)
# float offsets of the LDS parameter block: tail | front, and the attention chain's own block
PV_TAIL_END, PV_FRONT_END, PV_ATTN_END = 4224, 4224 + 768 + 6 * 256 + 832, 1024
# the slots each epilogue reads (bias, LayerNorm weight / bias): the classification side's, then the regression side's
PV_READS = {FFN0: [(768, 1280)], FFN1: [(1280, 2048)], BR1: [(2048, 2816), (3648, 3904)], BR2: [(2816, 3584), (3904, 4160)],
            OUT: [(3584, 3648), (4160, 4224)], PE3: [(4224 + 1536, 4224 + 2304)], QKV: [(4224 + 2304, PV_FRONT_END)],
            AOUT: [(0, 768)], SAMP: [(768, 1024)]}
PV_PROLOGUE = {TAIL: [(0, 768)], FRONT: [(4224, 4224 + 1536)], ATT: []}      # out-projection bias + norm2 | position_encoder.0 / .1


def so_cols(c):
    return c['G'] * c['P'] * (3 + c['L'])


def matrices(c):
    """(N, K) of the 12 matrices in image order, from the decoder layer's shapes"""
    return [(FFN, D), (D, FFN), (D, D), (D, D), (D, D), (D, D), (c['classes'], D), (CODE, D), (D, D), (c['qkv'], D), (D, D), (so_cols(c), D)]


def offsets(c):
    at = [0]
    for N, K in matrices(c):
        at.append(at[-1] + (N + 63) // 64 * 64 * K)
    return at


def lds_offsets(rg):
    R = 4 * rg
    return dict(x2=0, x3=R * LDX, h=2 * R * LDX, c=2 * R * LDX, r=3 * R * LDX)


def lds_bytes(rg):
    R = 4 * rg
    floats = 4 * R * LDX + (16 if rg == 1 else 12) * R * 64 + (8 * 3 * 1024 if rg == 1 else 0) + 8 * 64 + PV_FRONT_END
    return 4 * floats


@pytest.fixture(scope='module')
def plan():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    from sparsebev_amd.runtime import DecoderConfig
    lib = _lib.load()
    buf = (ctypes.c_int32 * 512)()

    def call(c, kind, with_front=0, pair_ok=0, cus=256, capacity=512):
        cfg = DecoderConfig()
        cfg.B, cfg.Q, cfg.G, cfg.P, cfg.L = c['B'], c['Q'], c['G'], c['P'], c['L']
        cfg.T, cfg.N, cfg.H = 8, 6, 8
        cfg.D, cfg.ffn, cfg.code_size, cfg.num_classes, cfg.attn_in_rows = D, FFN, CODE, c['classes'], c['qkv']
        n = lib.sbev_decoder_chain_plan(ctypes.byref(cfg), kind, with_front, pair_ok, cus, buf, capacity)
        if n < 0:
            return n
        w = list(buf[:n])
        p = dict(zip(('pre', 'rg', 'pair', 'grid', 'lds', 'n_units', 'n_pairs', 'warm', 'warm_lines', 'vec', 'vec_off', 'vec_n'), w[:12]))
        members = 2 if p['pair'] else 1
        assert n == 12 + 18 * members * p['n_units']
        units = [dict(epi=w[i], col0=w[i + 1], a=tuple(w[i + 2:i + 10]), b=tuple(w[i + 10:i + 18])) for i in range(12, n, 18)]
        p['units'] = [units[m * p['n_units']:(m + 1) * p['n_units']] for m in range(members)]
        return p
    return call


def config(B, Q, classes=10, qkv=776, G=4, P=4, L=4):
    return dict(B=B, Q=Q, classes=classes, qkv=qkv, G=G, P=P, L=L)


# ---- the launchers' inline arithmetic of the commit before the plan was factored out, written again from its text ----------------
def pieces(rg, cgs, K):
    if rg == 1:
        return 0
    tie_large = os.environ.get('SBEV_CHAIN_TIE_SMALL') is None
    best, best_cost = 1, 1e30
    kh = 1
    while kh <= 4 and cgs * kh <= 12 and K // kh >= 64:
        items = cgs * kh
        full, rest = items // 8, items % 8
        cost = (K / (16.0 * kh)) * (full + (0.0 if rest == 0 else 0.5 if rest <= 4 else 1.0))
        if (cost < best_cost + 1e-9) if tie_large else (cost < best_cost - 1e-9):
            best_cost, best = cost, kh
        kh *= 2
    return best


def row_groups(rows):
    forced = int(os.environ.get('SBEV_CHAIN_RG', '0') or 0)
    if (forced == 1 and rows <= 1024) or (forced == 2 and rows <= 2048) or forced == 4:
        return forced
    return 1 if rows <= 1024 else 2 if rows <= 2048 else 4


def pair_blocks(rows, rg):
    pairs = (rows + 4 * rg - 1) // (4 * rg)
    return 16 * ((pairs + 7) // 8)


def pair_row_groups(rows, pair_ok, cus):
    if not pair_ok or rows > 4096:
        return 0
    rg = 2
    while rg <= (4 if os.environ.get('SBEV_CHAIN_PAIR16') is not None else 2):
        if pair_blocks(rows, rg) <= cus:
            return rg
        rg *= 2
    return 0


def lin(wp, in_off, ld, N, K, kh=0, cg0=0, ncg=-1):
    KH = kh if kh > 0 else K // 128
    if ncg < 0:
        ncg = (N + 63) // 64 - cg0
    return (wp + cg0 * K * 64, in_off, ld, KH, ncg * KH, K // (16 * KH), 0, KH)


def lin_khalf(wp, in_off, ld, N, K, kh, half):
    return (wp, in_off, ld, kh, (N + 63) // 64 * kh, K // (32 * kh), half * kh, 2 * kh)


def unit(a, b, epi, col0=0):
    return dict(epi=epi, col0=col0, a=a, b=b)


def add_front(units, c, at, rg):
    o = lds_offsets(rg)
    units.append(unit(lin(at[8], o['c'], LDX, D, D, pieces(rg, D // 64, D)), NONE, PE3))
    ncg = (c['qkv'] + 63) // 64
    for cg0 in range(0, ncg, 8):
        n_here = min(ncg - cg0, 8)
        units.append(unit(lin(at[9], o['x2'], LDX, c['qkv'], D, pieces(rg, n_here, D), cg0, n_here), NONE, QKV, cg0 * 64))


def restated(c, kind, with_front, pair_ok, cus):
    rows = c['B'] * c['Q']
    at = offsets(c)
    vec = at[12]
    if kind == FRONT:
        rg = row_groups(rows)
        units = []
        add_front(units, c, at, rg)
        return dict(pre=FRONT, rg=rg, pair=0, grid=(rows + 4 * rg - 1) // (4 * rg), lds=lds_bytes(rg), n_units=len(units), n_pairs=0,
                    warm=at[8], warm_lines=(at[10] - at[8]) // 32, vec=vec + PV_TAIL_END, vec_off=PV_TAIL_END,
                    vec_n=PV_FRONT_END - PV_TAIL_END, units=[units])
    if kind == ATT:
        rg = row_groups(rows)
        o = lds_offsets(rg)
        soN = so_cols(c)
        units = [unit(lin(at[10], o['x2'], LDX, D, D, pieces(rg, D // 64, D)), NONE, AOUT),
                 unit(lin(at[11], o['x3'], LDX, soN, D, pieces(rg, (soN + 63) // 64, D)), NONE, SAMP)]
        return dict(pre=ATT, rg=rg, pair=0, grid=(rows + 4 * rg - 1) // (4 * rg), lds=lds_bytes(rg), n_units=2, n_pairs=0,
                    warm=at[10], warm_lines=(vec - at[10]) // 32, vec=vec + PV_FRONT_END, vec_off=0, vec_n=PV_ATTN_END, units=[units])
    common = dict(pre=TAIL, warm=at[0], warm_lines=((at[10] if with_front else at[8]) - at[0]) // 32, vec=vec, vec_off=0,
                  vec_n=PV_FRONT_END if with_front else PV_TAIL_END)
    dcg = D // 64
    prg = pair_row_groups(rows, pair_ok, cus)
    if prg:
        rg = prg
        o = lds_offsets(rg)
        half_cg = FFN // 128
        kh1 = pieces(rg, dcg, FFN // 2)
        q0_forced = int(os.environ.get('SBEV_CHAIN_PAIR_Q0', '-1') or -1)
        qcg = (c['qkv'] + 63) // 64
        q0 = q0_forced if 0 <= q0_forced <= qcg else (qcg - 8 if qcg > 8 else qcg // 2)
        tables = []
        for mem in (0, 1):
            u = [unit(lin(at[0], o['x2'], LDX, FFN, D, pieces(rg, half_cg, D), mem * half_cg, half_cg), NONE, FFN0),
                 unit(lin_khalf(at[1], o['h'], LDH, D, FFN, kh1, mem), NONE, FFN1)]
            br1 = lin(at[3] if mem else at[2], o['x3'], LDX, D, D, pieces(rg, dcg, D))
            br2 = lin(at[5] if mem else at[4], o['r'] if mem else o['c'], LDX, D, D, pieces(rg, dcg, D))
            out = lin(at[7], o['r'], LDX, CODE, D, pieces(rg, 1, D)) if mem else lin(at[6], o['c'], LDX, c['classes'], D, pieces(rg, 1, D))
            for l, epi in ((br1, BR1), (br2, BR2), (out, OUT)):
                u.append(unit(NONE, l, epi) if mem else unit(l, NONE, epi))
            if with_front:
                u.append(unit(lin(at[8], o['c'], LDX, D, D, pieces(rg, dcg, D)) if mem else NONE, NONE, PE3))
                cg0, ncg = (q0, qcg - q0) if mem else (0, q0)
                u.append(unit(lin(at[9], o['x2'], LDX, c['qkv'], D, pieces(rg, ncg, D), cg0, ncg) if ncg > 0 else NONE, NONE, QKV, cg0 * 64))
            tables.append(u)
        return dict(common, rg=rg, pair=1, grid=pair_blocks(rows, rg), lds=lds_bytes(rg), n_units=len(tables[0]),
                    n_pairs=(rows + 4 * rg - 1) // (4 * rg), units=tables)
    rg = row_groups(rows)
    o = lds_offsets(rg)
    u = [unit(lin(at[0], o['x2'], LDX, FFN, D, pieces(rg, FFN // 64, D)), NONE, FFN0),
         unit(lin(at[1], o['h'], LDH, D, FFN, pieces(rg, dcg, FFN)), NONE, FFN1),
         unit(lin(at[2], o['x3'], LDX, D, D, pieces(rg, 2 * dcg, D)), lin(at[3], o['x3'], LDX, D, D, pieces(rg, 2 * dcg, D)), BR1),
         unit(lin(at[4], o['c'], LDX, D, D, pieces(rg, 2 * dcg, D)), lin(at[5], o['r'], LDX, D, D, pieces(rg, 2 * dcg, D)), BR2),
         unit(lin(at[6], o['c'], LDX, c['classes'], D, pieces(rg, 2, D)), lin(at[7], o['r'], LDX, CODE, D, pieces(rg, 2, D)), OUT)]
    if with_front:
        add_front(u, c, at, rg)
    return dict(common, rg=rg, pair=0, grid=(rows + 4 * rg - 1) // (4 * rg), lds=lds_bytes(rg), n_units=len(u), n_pairs=0, units=[u])


# ---- properties every plan must have, independent of the restatement ----------------------------------------------------------------
def check_properties(p, c, kind, with_front, cus, case):
    rows = c['B'] * c['Q']
    at, mats = offsets(c), matrices(c)
    rg = p['rg']
    assert rg in (1, 2, 4) and p['lds'] == lds_bytes(rg) <= 160 * 1024, case
    if p['pair']:
        pairs = (rows + 4 * rg - 1) // (4 * rg)
        assert kind == TAIL and rg > 1 and p['n_pairs'] == pairs and p['grid'] == 16 * ((pairs + 7) // 8) <= cus, case
        assert len(p['units']) == 2 and len(p['units'][0]) == len(p['units'][1]) == p['n_units'], case
        assert [(u['epi'], ) for u in p['units'][0]] == [(u['epi'], ) for u in p['units'][1]], case
    else:
        assert p['grid'] == (rows + 4 * rg - 1) // (4 * rg) and p['n_pairs'] == 0 and len(p['units']) == 1, case
    assert 1 <= p['n_units'] <= 8, case
    warm0, warm1 = p['warm'], p['warm'] + 32 * p['warm_lines']
    assert 0 <= warm0 and warm1 <= at[12], case
    covered = {}                   # matrix -> 16-k chunks (column group, chunk) some item multiplies
    reads = PV_PROLOGUE[kind] + (PV_PROLOGUE[FRONT] if kind == TAIL and with_front else [])
    for table in p['units']:
        for u in table:
            assert u['a'][4] + u['b'][4] <= (16 if rg == 1 else 12), case
            if u['a'][4] + u['b'][4] > 0:
                reads = reads + PV_READS[u['epi']]
            for w, in_off, ld, KH, items, chunks, kh0, KHT in (u['a'], u['b']):
                assert chunks % 4 == 0 and chunks > 0, case
                if items == 0:
                    continue
                mat = max(i for i in range(12) if at[i] <= w)
                N, K = mats[mat]
                assert (w - at[mat]) % (K * 64) == 0 and items % KH == 0 and chunks * 16 * KHT == K and kh0 + KH <= KHT, case
                cg0, cgs = (w - at[mat]) // (K * 64), items // KH
                assert items == cgs * KH and cg0 + cgs <= (N + 63) // 64, case
                assert warm0 <= w and w + cgs * K * 64 <= warm1, case               # inside the warmed span (hence inside the image)
                assert (in_off, ld) in {(o, LDH if mat == 1 else LDX) for o in lds_offsets(rg).values()}, case
                seen = covered.setdefault(mat, set())
                for j in range(items):
                    piece = kh0 + j % KH
                    cells = {(cg0 + j // KH, k) for k in range(piece * chunks, (piece + 1) * chunks)}
                    assert not (cells & seen), case                                 # nothing is multiplied twice ...
                    seen |= cells
    streamed = {FRONT: (8, 9), ATT: (10, 11), TAIL: tuple(range(8)) + ((8, 9) if with_front else ())}[kind]
    assert sorted(covered) == [m for m in streamed if mats[m][0] > 0], case
    for mat, seen in covered.items():                                               # ... and nothing is left out: the members' ffn.0 and
        N, K = mats[mat]                                                            # in-projection column groups, their ffn.1 k-pieces
        assert len(seen) == (N + 63) // 64 * (K // 16), (case, mat)                 # and branch sides PARTITION each weight
    for lo, hi in reads:
        assert p['vec_off'] <= lo and hi <= p['vec_off'] + p['vec_n'], case
    block = at[12] + {TAIL: 0, FRONT: 0, ATT: PV_FRONT_END}[kind]
    assert p['vec'] == block + p['vec_off'] and p['vec'] + p['vec_n'] <= at[12] + PV_FRONT_END + PV_ATTN_END, case


def test_plan_equals_the_restated_arithmetic_and_has_the_properties(plan):
    n = 0
    for (B, Q), classes, qkv, (G, P, L) in itertools.product(BQ, CLASSES, QKV_ROWS, GPL):
        c = config(B, Q, classes, qkv, G, P, L)
        for kind in (FRONT, ATT):
            p = plan(c, kind)
            assert p == restated(c, kind, 0, 0, 256), (c, kind, p)
            check_properties(p, c, kind, 0, 256, (c, kind))
            n += 1
        assert plan(c, FRONT, 1, 1, 64) == plan(c, FRONT) and plan(c, ATT, 1, 1, 64) == plan(c, ATT)      # the tail's inputs only
        for with_front, pair_ok, cus in itertools.product((0, 1), (0, 1), CUS):
            case = (c, with_front, pair_ok, cus)
            p = plan(c, TAIL, with_front, pair_ok, cus)
            assert p == restated(c, TAIL, with_front, pair_ok, cus), (case, p)
            check_properties(p, c, TAIL, with_front, cus, case)
            n += 1
    assert n == len(BQ) * 27 * (2 + 12) and len(BQ) == 18


def test_plan_anchors(plan):
    """Three plans derived by hand from the launchers' code, as literals (config 2's layer: 10 classes, 776 in-projection rows = 13
    column groups, 4 x 4 points on 4 levels = 112 sampling columns; image offsets in floats)."""
    ffn1, cls6, reg4, pe3, qkv, attn_out, samp, vec = 131072, 524288, 540672, 557056, 622592, 835584, 901120, 933888
    # 900 rows on 256 CUs with pairs: 113 pairs of 8 rows -> 16 x 15 workgroups; every member unit has 8 items of 8 chunks but: the
    # output unit (1 column group in 4 k-pieces), and the in-projection cut at q0 = 13 - 8 = 5 (member 0: 5 groups x 2, member 1: 8 x 1)
    p = plan(config(1, 900), TAIL, 1, 1, 256)
    assert {k: v for k, v in p.items() if k != 'units'} == dict(pre=0, rg=2, pair=1, grid=240, lds=89856, n_units=7, n_pairs=113, warm=0,
                                                                warm_lines=26112, vec=vec, vec_off=0, vec_n=7360)
    m0, m1 = p['units']
    assert [u['epi'] for u in m0] == [u['epi'] for u in m1] == [FFN0, FFN1, BR1, BR2, OUT, PE3, QKV]
    assert m0[0] == unit((0, 0, 264, 2, 8, 8, 0, 2), NONE, FFN0) and m1[0] == unit((4 * 256 * 64, 0, 264, 2, 8, 8, 0, 2), NONE, FFN0)
    assert m0[1] == unit((ffn1, 4224, 520, 2, 8, 8, 0, 4), NONE, FFN1) and m1[1] == unit((ffn1, 4224, 520, 2, 8, 8, 2, 4), NONE, FFN1)
    assert m0[4] == unit((cls6, 4224, 264, 4, 4, 4, 0, 4), NONE, OUT) and m1[4] == unit(NONE, (reg4, 6336, 264, 4, 4, 4, 0, 4), OUT)
    assert m0[5] == unit(NONE, NONE, PE3) and m1[5] == unit((pe3, 4224, 264, 2, 8, 8, 0, 2), NONE, PE3)
    assert m0[6] == unit((qkv, 0, 264, 2, 10, 8, 0, 2), NONE, QKV, 0)
    assert m1[6] == unit((qkv + 5 * 256 * 64, 0, 264, 1, 8, 16, 0, 1), NONE, QKV, 320)
    # 1600 rows: pairs would take 16 x 25 = 400 workgroups -> one workgroup per 8 rows, the in-projection in units of 8 + 5 column groups
    p = plan(config(1, 1600), TAIL, 1, 1, 256)
    assert {k: v for k, v in p.items() if k != 'units'} == dict(pre=0, rg=2, pair=0, grid=200, lds=89856, n_units=8, n_pairs=0, warm=0,
                                                                warm_lines=26112, vec=vec, vec_off=0, vec_n=7360)
    u, = p['units']
    assert u[0] == unit((0, 0, 264, 1, 8, 16, 0, 1), NONE, FFN0) and u[1] == unit((ffn1, 4224, 520, 2, 8, 16, 0, 2), NONE, FFN1)
    assert u[4] == unit((cls6, 4224, 264, 4, 4, 4, 0, 4), (reg4, 6336, 264, 4, 4, 4, 0, 4), OUT)
    assert u[6] == unit((qkv, 0, 264, 1, 8, 16, 0, 1), NONE, QKV, 0) and u[7] == unit((qkv + 8 * 256 * 64, 0, 264, 2, 10, 8, 0, 2), NONE, QKV, 512)
    # 3600 rows: 16 rows per workgroup; the attention chain streams attn_out + the sampling Linear (2 column groups in 4 k-pieces)
    p = plan(config(4, 900), ATT)
    assert p == dict(pre=2, rg=4, pair=0, grid=225, lds=148224, n_units=2, n_pairs=0, warm=attn_out, warm_lines=3072, vec=vec + 7360,
                     vec_off=0, vec_n=1024, units=[[unit((attn_out, 0, 264, 2, 8, 8, 0, 2), NONE, AOUT),
                                                    unit((samp, 16 * 264, 264, 4, 8, 4, 0, 4), NONE, SAMP)]])
    assert plan(config(4, 900), TAIL, 0, 1, 256)['grid'] == 225 and plan(config(4, 900), TAIL, 0, 1, 256)['warm_lines'] == pe3 // 32


def test_plan_refuses_uncovered_configs_and_short_buffers(plan):
    assert plan(config(1, 4097), TAIL) == -1 and plan(config(1, 0), TAIL) == -1         # more than one round of 16-row workgroups; no rows
    assert plan(config(1, 900, qkv=833), FRONT) == -1 and plan(config(1, 900, classes=65), TAIL) == -1
    assert plan(config(1, 900, G=4, P=8, L=6), ATT) == -1                               # 288 sampling columns
    assert plan(config(1, 900), 3) == -1 and plan(config(1, 900), TAIL, cus=-1) == -1
    assert plan(config(1, 900), ATT, capacity=47) == -1                                 # 12 + 2 x 18 words needed
    assert b'48 words' in _lib.load().sbev_last_error()
    assert plan(config(1, 900), ATT, capacity=48)['n_units'] == 2
