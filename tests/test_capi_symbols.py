"""CPU-side checks of the C-ABI boundary: the library loads, exports every symbol include/sbev_hip.h
declares (and nothing it does not), the ctypes table matches, and argument validation returns the
documented status codes without ever touching a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from sparsebev_amd import _lib

HEADER = os.path.join(ROOT, 'include', 'sbev_hip.h')


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(sbev_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from sparsebev_amd.csrc import build
        build.build()
    return _lib.load()


def test_header_symbols_all_exported(lib):
    syms = declared_symbols()
    assert 'sbev_msmv_fwd' in syms and 'sbev_project_select' in syms
    for s in syms:
        assert hasattr(lib, s), 'libsbev_hip.so does not export %s' % s
    assert sorted(_lib.SIGNATURES) == syms, 'ctypes table and include/sbev_hip.h disagree'


def test_exports_are_plain_c(lib):
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and l.split()[-1].startswith('sbev_'))
    assert exported == declared_symbols()          # extern "C": unmangled, exactly the header's set


def test_abi_version_and_device_query(lib):
    assert lib.sbev_abi_version() == 1
    assert lib.sbev_device_count() >= 0


def test_argument_validation_without_gpu(lib):
    L = 4
    feats = (ctypes.c_void_p * L)(1, 1, 1, 1)
    hw = (ctypes.c_int32 * (2 * L))(*([4, 4] * L))
    s = (ctypes.c_int64 * L)(*([16] * L))
    one = ctypes.c_void_p(16)

    def call(L_=L, P=4, C=8, layout=0, Bp=2):
        return lib.sbev_msmv_fwd(feats, hw, L_, 0, Bp, 6, C, 3, P, 1, s, 0, s, C, one, one, one, layout, 1, 1, None)

    assert call(P=33) == -1 and b'num_point exceed limits' in lib.sbev_last_error()   # msmv_sampling.cpp:125
    assert call(L_=6) == -1
    assert call(C=6) == -1
    assert call(layout=7) == -1
    assert call(Bp=0) == 0                                                             # empty input: no launch, OK
    assert lib.sbev_project_select(None, None, 1, 4, 1, 6, 4, 4, 1.0, 1.0, 1e-5, None, None, None, None, None) == -1
    assert lib.sbev_project_select(None, None, 0, 4, 1, 6, 4, 4, 1.0, 1.0, 1e-5, None, None, None, None, None) == 0


def _sampler_entry_points(lib):
    """The eight entry points that take a feature pyramid + sample points, each as call(**overrides) over ONE shared description
    (fake pointers: validation returns before any HIP call).  Base: 4 levels of 4 x 4 pixels, grouped channels-last [B*T*N, H, W, G*C]
    with B, T, G, N, C, Q, P = 1, 2, 4, 6, 64, 3, 4, mixing layout, a 2-slot ring."""
    M = 6                                                  # array capacity: one more than SBEV_MAX_LEVELS, for the L = 6 row
    base = dict(L=4, hw=[4, 4] * M, dtype=0, B=1, T=2, G=4, N=6, C=64, Q=3, P=4, gdiv=4, feats=[0x1000] * M, gfeats=[0x1000] * M,
                sbo=[6 * 16 * 256] * M, sg=64, sv=[16 * 256] * M, spx=256, ptr=0x1000, layout=1, slots=[0, 1], n_slots=2,
                Pout=128, up=9, order=None)

    def args(o):
        d = dict(base, **o)
        d.setdefault('Bp', d['B'] * d['T'] * d['G'])
        arr = lambda ct, v: None if v is None else (ct * len(v))(*v)
        d.update(feats=arr(ctypes.c_void_p, d['feats']), gfeats=arr(ctypes.c_void_p, d['gfeats']), hw=arr(ctypes.c_int32, d['hw']),
                 sbo=arr(ctypes.c_int64, d['sbo']), sv=arr(ctypes.c_int64, d['sv']), slots=arr(ctypes.c_int32, d['slots']),
                 ptr=ctypes.c_void_p(d['ptr']), order=None if d['order'] is None else ctypes.c_void_p(d['order']))
        d['pyr'] = (d['gdiv'], d['sbo'], d['sg'], d['sv'], d['spx'], d['ptr'], d['ptr'])      # ... gdiv, strides, loc, weights
        return d

    def fwd(d, ring):
        tail = (d['slots'], d['n_slots'], None) if ring else (None,)
        return (lib.sbev_msmv_fwd_ring if ring else lib.sbev_msmv_fwd)(
            d['feats'], d['hw'], d['L'], d['dtype'], d['Bp'], d['N'], d['C'], d['Q'], d['P'], *d['pyr'], d['ptr'], d['layout'], d['T'], d['G'], *tail)

    def bwd(d, ex):
        mid = (d['layout'], d['T'], d['G']) if ex else ()
        return (lib.sbev_msmv_bwd_ex if ex else lib.sbev_msmv_bwd)(
            d['feats'], d['gfeats'], d['hw'], d['L'], d['Bp'], d['N'], d['C'], d['Q'], d['P'], *d['pyr'], d['ptr'], *mid, d['ptr'], d['ptr'], None)

    def mix(d, pairs, ordered):
        fn = getattr(lib, 'sbev_sample_mix_' + ('pairs_f16' if pairs else 'f32') + ('_ordered' if ordered else ''))
        tail = ((d['up'],) if pairs else ()) + ((d['order'],) if ordered else ()) + (None,)
        return fn(d['feats'], d['hw'], d['L'], d['dtype'], d['B'], d['N'], d['Q'], d['T'], d['G'], d['P'], d['C'], *d['pyr'][1:],
                  d['slots'], d['n_slots'], d['ptr'], d['ptr'], d['Pout'], 1e-5, *tail)

    return {'fwd': lambda **o: fwd(args(o), False), 'fwd_ring': lambda **o: fwd(args(o), True),
            'bwd': lambda **o: bwd(args(o), False), 'bwd_ex': lambda **o: bwd(args(o), True),
            'mix': lambda **o: mix(args(o), False, False), 'mix_ordered': lambda **o: mix(args(o), False, True),
            'mix_pairs': lambda **o: mix(args(o), True, False), 'mix_pairs_ordered': lambda **o: mix(args(o), True, True)}


def test_sampler_entry_points_refusal_table(lib):
    """What each of the eight pyramid-taking entry points answers to a table of good and bad descriptions, status and message.  The three
    implementations behind them do NOT check the same things (the backward accepts any C >= 1 and checks neither strides nor maps; the
    fused launch needs every slab below the buffer limit; only the forward validates the levels of an empty call): those differences
    are behaviour and are pinned here.  No row reaches a launch: a refusal returns first, an accepted row is an empty call (B = 0 or
    Q = 0)."""
    call = _sampler_entry_points(lib)
    FWD, BWD = ('fwd', 'fwd_ring'), ('bwd', 'bwd_ex')
    MIX = ('mix', 'mix_ordered', 'mix_pairs', 'mix_pairs_ordered')
    OK = (0, b'')
    hw_at = lambda l, h, w: [4, 4] * l + [h, w] + [4, 4] * (5 - l)          # level l is h x w, the others 4 x 4
    at = lambda l, v, rest: [rest] * l + [v] + [rest] * (5 - l)
    big, mid = 8192, 2048            # with N = 1: 8192^2 pixels of 256 elements = 2^34 elements; 2048^2 of them = 2^30 (4 GiB of fp32)
    unsupported = (-1, b'sbev_sample_mix_f32: needs L in {4,5}')
    table = [
        # (overrides, {entry points: (status, substring of sbev_last_error())})
        (dict(B=0), {FWD + BWD + MIX: OK}),
        (dict(Q=0), {FWD + BWD + MIX: OK}),
        (dict(B=0, hw=hw_at(1, 0, 4)), {FWD: (-1, b'sbev_msmv_fwd: level 1 has empty map'), BWD + MIX: OK}),
        (dict(B=0, feats=at(1, 0, 0x1000)), {FWD + BWD + MIX: OK}),
        (dict(hw=None), {FWD: (-1, b'sbev_msmv_fwd: null descriptor array'), BWD: (-1, b'sbev_msmv_bwd: null descriptor array'),
                         MIX: (-1, b'sbev_sample_mix_f32: null descriptor array')}),
        (dict(B=0, sbo=None), {FWD: (-1, b'sbev_msmv_fwd: null descriptor array'), BWD: (-1, b'sbev_msmv_bwd: null descriptor array'),
                               MIX: (-1, b'sbev_sample_mix_f32: null descriptor array')}),
        (dict(B=0, feats=None), {FWD + BWD + MIX: (-1, b'null descriptor array')}),
        (dict(B=0, sv=None), {FWD + BWD + MIX: (-1, b'null descriptor array')}),
        (dict(B=0, gfeats=None), {('bwd',): (-1, b'sbev_msmv_bwd: null descriptor array'), ('bwd_ex',): OK}),      # frozen features: _ex only
        (dict(L=0), {FWD: (-1, b'sbev_msmv_fwd: L=0 not in 1..5'), BWD: (-1, b'sbev_msmv_bwd: L=0'), MIX: unsupported}),
        (dict(L=6), {FWD: (-1, b'sbev_msmv_fwd: L=6 not in 1..5'), BWD: (-1, b'sbev_msmv_bwd: L=6'), MIX: unsupported}),
        (dict(B=0, L=3), {FWD + BWD: OK, MIX: unsupported}),
        (dict(P=33), {FWD: (-1, b'sbev_msmv_fwd: num_point exceed limits (P=33 > 32)'), BWD: (-1, b'sbev_msmv_bwd: num_point exceed limits (P=33'),
                      MIX: unsupported}),
        (dict(P=0), {FWD + BWD: (-1, b'num_point exceed limits'), MIX: unsupported}),
        (dict(B=0, C=6), {FWD: (-1, b'sbev_msmv_fwd: C=6 must be a positive multiple of 4'), BWD: OK, MIX: unsupported}),
        (dict(C=0), {FWD: (-1, b'sbev_msmv_fwd: C=0 must be'), BWD: (-1, b'sbev_msmv_bwd: bad sizes'), MIX: unsupported}),
        (dict(N=0), {FWD: (-1, b'sbev_msmv_fwd: bad sizes'), BWD: (-1, b'sbev_msmv_bwd: bad sizes'), MIX: (-1, b'sbev_sample_mix_f32: bad sizes')}),
        (dict(gdiv=0), {FWD: (-1, b'sbev_msmv_fwd: bad sizes'), BWD: (-1, b'sbev_msmv_bwd: bad sizes')}),
        (dict(dtype=3), {FWD: (-1, b'sbev_msmv_fwd: feat_dtype 3'), MIX: (-1, b'sbev_sample_mix_f32: feat_dtype 3')}),
        (dict(hw=hw_at(1, 0, 4)), {FWD: (-1, b'sbev_msmv_fwd: level 1 has empty map'), MIX: (-1, b'sbev_sample_mix_f32: level 1')}),
        (dict(feats=at(1, 0, 0x1000)), {FWD: (-1, b'sbev_msmv_fwd: feats[1] is null'), BWD: (-1, b'sbev_msmv_bwd: level 1 pointer is null'),
                                        MIX: (-1, b'sbev_sample_mix_f32: ')}),
        (dict(gfeats=at(2, 0, 0x1000)), {BWD: (-1, b'sbev_msmv_bwd: level 2 pointer is null')}),
        (dict(ptr=0), {FWD: (-1, b'sbev_msmv_fwd: null loc/weights/out'), BWD: (-1, b'sbev_msmv_bwd: null pointer'),
                       MIX: (-1, b'sbev_sample_mix_f32: null pointer')}),
        # strides: multiples of 4 elements for the forward and the fused launch (16-byte taps); the backward does not ask
        (dict(B=0, spx=258), {FWD: (-1, b'sbev_msmv_fwd: pixel/group strides must be multiples of 4'), BWD: OK,
                              MIX: (-1, b'sbev_sample_mix_f32: pixel/group strides must be multiples of 4')}),
        (dict(B=0, sg=66), {FWD: (-1, b'sbev_msmv_fwd: pixel/group strides'), BWD: OK, MIX: (-1, b'sbev_sample_mix_f32: pixel/group strides')}),
        (dict(B=0, sv=at(1, 4098, 4096)), {FWD: (-1, b'sbev_msmv_fwd: level 1 strides must be multiples of 4 elements'), BWD + MIX: OK}),
        (dict(sv=at(1, 4098, 4096)), {FWD: (-1, b'sbev_msmv_fwd: level 1 strides'), MIX: (-1, b'sbev_sample_mix_f32: level 1 strides')}),
        (dict(sbo=at(3, 6 * 4096 + 2, 6 * 4096)), {FWD: (-1, b'sbev_msmv_fwd: level 3 strides'), MIX: (-1, b'sbev_sample_mix_f32: level 3 strides')}),
        (dict(sv=at(0, -4096, 4096)), {FWD: (-1, b'sbev_msmv_fwd: level 0: one (sample-batch) slab spans'), MIX: (-1, b'one (sample-batch) slab must stay below 2 GiB')}),
        # one slab beyond the 32-bit in-slab offset: refused by the forward also when the call is empty
        (dict(N=1, hw=hw_at(0, big, big), sv=at(0, big * big * 256, 4096)),
         {FWD: (-1, b'the in-slab tap offset is 32-bit (limit 2^31 - 1)'), MIX: (-1, b'one (sample-batch) slab must stay below 2 GiB')}),
        (dict(B=0, N=1, hw=hw_at(0, big, big), sv=at(0, big * big * 256, 4096)), {FWD: (-1, b'sbev_msmv_fwd: level 0: one (sample-batch) slab spans'), BWD + MIX: OK}),
        # one slab between the buffer limit (2^31 - 1 BYTES) and 2^31 elements: the forward has its global-load path, the fused launch refuses
        (dict(B=0, N=1, hw=hw_at(2, mid, mid), sv=at(2, mid * mid * 256, 4096)), {FWD + BWD + MIX: OK}),
        (dict(N=1, hw=hw_at(2, mid, mid), sv=at(2, mid * mid * 256, 4096)), {MIX: (-1, b'one (sample-batch) slab must stay below 2 GiB')}),
        (dict(layout=7), {FWD: (-1, b'sbev_msmv_fwd: out_layout 7'), ('bwd_ex',): (-1, b'sbev_msmv_bwd: grad_out_layout 7')}),
        (dict(Bp=7), {FWD: (-1, b"sbev_msmv_fwd: B'=7 is not B*T*G (T=2, G=4)"), ('bwd_ex',): (-1, b"sbev_msmv_bwd: B'=7 is not B*T*G (T=2, G=4)")}),
        (dict(Bp=7, Q=0, layout=0), {FWD + BWD: OK}),                        # reference layout: T and G are not read
        (dict(Bp=8, T=0), {FWD: (-1, b"sbev_msmv_fwd: B'=8 is not B*T*G (T=0, G=4)"), ('bwd_ex',): (-1, b"sbev_msmv_bwd: B'=8 is not B*T*G")}),
        (dict(Bp=1 << 31), {FWD: (-1, b"sbev_msmv_fwd: B'*Q = 6442450944 too large for one launch")}),
        (dict(Bp=1 << 32), {BWD: (-1, b"sbev_msmv_bwd: B'*Q too large")}),
        (dict(B=1 << 29), {MIX: (-1, b'sbev_sample_mix_f32: too many items')}),
        (dict(Pout=64), {MIX: (-1, b'sbev_sample_mix_f32: built for 128 out points')}),
        # the ring
        (dict(B=0, slots=None), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: frame_slots is null'), MIX: OK}),
        (dict(slots=[0, 2]), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: frame_slots[1] = 2 out of range'), MIX: (-1, b'sbev_sample_mix_f32: frame_slots[1]')}),
        (dict(slots=[-1, 1]), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: frame_slots[0] = -1 out of range'), MIX: (-1, b'sbev_sample_mix_f32: frame_slots[0]')}),
        (dict(B=0, slots=[0, 2]), {('fwd_ring',) + MIX: OK}),                # the slot table of an empty call is not read
        (dict(n_slots=1), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: need 1 <= T <= 16, n_slots >= T, gdiv == G'), MIX: (-1, b'T <= 16, n_slots >= T')}),
        (dict(T=17, slots=list(range(17)), n_slots=17), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: need 1 <= T <= 16'), MIX: unsupported}),
        (dict(gdiv=1), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: need 1 <= T <= 16, n_slots >= T, gdiv == G')}),
        (dict(layout=0, T=2, G=2), {('fwd_ring',): (-1, b'sbev_msmv_fwd_ring: need')}),                                     # gdiv = 4 != G
        # the fused launch's own arguments
        (dict(B=0, up=101), {('mix_pairs', 'mix_pairs_ordered'): (-1, b'sbev_sample_mix_pairs_f16: up_log2=101'), ('mix', 'mix_ordered'): OK}),
        (dict(up=-101), {('mix_pairs', 'mix_pairs_ordered'): (-1, b'sbev_sample_mix_pairs_f16: up_log2=-101')}),
        (dict(order=0x1002), {('mix_ordered', 'mix_pairs_ordered'): (-1, b'sbev_sample_mix_f32: order must be 4-byte aligned')}),
        (dict(B=0, order=0x1002), {MIX: OK}),
    ]
    for overrides, expected in table:
        for names, (status, text) in expected.items():
            for name in names:
                got = call[name](**overrides)
                err = lib.sbev_last_error() if got != 0 else b''
                assert got == status and text in err, (name, overrides, got, err)
    # the shape / slab predicates the decoder plans with agree with the launch's refusals
    i32, i64 = lambda v: (ctypes.c_int32 * len(v))(*v), lambda v: (ctypes.c_int64 * len(v))(*v)
    assert lib.sbev_sample_mix_slabs_ok(i32([4, 4] * 4), 4, 0, 6, 64, i64([4096] * 4), 256) == 1
    assert lib.sbev_sample_mix_slabs_ok(i32(hw_at(2, mid, mid)), 4, 0, 1, 64, i64(at(2, mid * mid * 256, 4096)), 256) == 0
    assert lib.sbev_sample_mix_slabs_ok(i32(hw_at(2, mid, mid)), 4, 1, 1, 64, i64(at(2, mid * mid * 256, 4096)), 256) == 1      # bf16: 2^31 - 376 bytes
    assert lib.sbev_sample_mix_slabs_ok(None, 4, 0, 6, 64, i64([4096] * 4), 256) == 0
    assert lib.sbev_sample_mix_slabs_ok(i32([4, 4] * 4), 6, 0, 6, 64, i64([4096] * 4), 256) == 0


def _split_image_entry_points(lib):
    """The three split-K out-projection entry points and the two generator entry points, each as call(**overrides) over one good call
    (fake, aligned pointers; M = 64, N = 256, K = 512): validation returns before any HIP call."""
    base = dict(X=0x1000, Wp=0x2000, Y=0x3000, ws=0x4000, scale=0x5000, xscale=0x6000, bias=None, M=64, N=256, K=512, ld=None, relu=0,
                mode=None, pairs=0, up=0)
    vp = lambda v: None if v is None else ctypes.c_void_p(v)

    def args(o, gen=False):      # mode: nimg / nprod (3 is valid for all five); ld: ldx = K, the generators' ldy = N
        d = dict(base, **o)
        d['mode'] = 3 if d['mode'] is None else d['mode']
        d['ld'] = (d['N'] if gen else d['K']) if d['ld'] is None else d['ld']
        return d

    def out(d, head):      # ..., bias, residual, ln_w, ln_b, ln_eps, Y, M, N, K, ldx, relu, nimg / nprod, workspace, stream
        return head + (vp(d['bias']), None, None, None, 1e-5, vp(d['Y']), d['M'], d['N'], d['K'], d['ld'], d['relu'], d['mode'], vp(d['ws']), None)

    def bf16s(**o):
        d = args(o)
        return lib.sbev_linear_splitk_bf16s(*out(d, (vp(d['X']), vp(d['Wp']))))

    def f16s(**o):
        d = args(o)
        return lib.sbev_linear_splitk_f16s(*out(d, (vp(d['X']), d['pairs'], d['up'], vp(d['Wp']), vp(d['scale']))))

    def xdev(**o):
        d = args(o)
        return lib.sbev_linear_splitk_f16s_xdev(*out(d, (vp(d['X']), vp(d['xscale']), vp(d['Wp']), vp(d['scale']))))

    def gen(**o):          # Xs, Ws, bias, Y, M, N, K, ldy, relu, nimg, stream
        d = args(o, gen=True)
        return lib.sbev_linear_bf16s_gen(vp(d['X']), vp(d['Wp']), vp(d['bias']), vp(d['Y']), d['M'], d['N'], d['K'], d['ld'], d['relu'], d['mode'], None)

    def f16gen(**o):       # Xs, xscale, Ws, wdown, bias, Y, M, N, K, ldy, relu, nprod, stream
        d = args(o, gen=True)
        return lib.sbev_linear_f16s_gen(vp(d['X']), vp(d['xscale']), vp(d['Wp']), vp(d['scale']), vp(d['bias']), vp(d['Y']), d['M'], d['N'], d['K'],
                                        d['ld'], d['relu'], d['mode'], None)

    return {'bf16s': bf16s, 'f16s': f16s, 'xdev': xdev, 'gen': gen, 'f16gen': f16gen}


def test_split_image_gemm_entry_points_refusal_table(lib):
    """Status and FULL message of sbev_linear_splitk_bf16s / _f16s / _f16s_xdev and sbev_linear_bf16s_gen / sbev_linear_f16s_gen, one
    provoking call per check in the order the checks run: mode (nimg / nprod), x_up_log2 range where the entry point has one, shape, the
    empty call (M == 0 returns 0 before any pointer is looked at), pointers, alignment.  A row that breaks several checks at once pins
    the order.  No row reaches a launch."""
    call = _split_image_entry_points(lib)
    nothing = dict(X=None, Wp=None, Y=None, ws=None, scale=None, xscale=None)
    shape = 'needs N == 256, K % 32 == 0, K >= 256'
    gshape = 'sbev_linear_bf16s_gen: needs N % 256 == 0, K % 32 == 0, K <= 4096'
    table = [
        # ---- sbev_linear_splitk_bf16s
        ('bf16s', dict(mode=4), -1, 'sbev_linear_splitk_bf16s: nimg=4 (2 = bf16x3, 3 = bf16x6)'),
        ('bf16s', dict(mode=1, N=128, **nothing), -1, 'sbev_linear_splitk_bf16s: nimg=1 (2 = bf16x3, 3 = bf16x6)'),
        ('bf16s', dict(N=128), -1, 'sbev_linear_splitk_bf16s: %s (N=128 K=512)' % shape),
        ('bf16s', dict(K=250, **nothing), -1, 'sbev_linear_splitk_bf16s: %s (N=256 K=250)' % shape),
        ('bf16s', dict(K=224), -1, 'sbev_linear_splitk_bf16s: %s (N=256 K=224)' % shape),
        ('bf16s', dict(M=-1), -1, 'sbev_linear_splitk_bf16s: %s (N=256 K=512)' % shape),
        ('bf16s', dict(M=1 << 22), -1, 'sbev_linear_splitk_bf16s: %s (N=256 K=512)' % shape),
        ('bf16s', dict(M=0, **nothing), 0, ''),
        ('bf16s', dict(M=0, mode=2, **nothing), 0, ''),
        ('bf16s', dict(M=0, N=128, **nothing), -1, 'sbev_linear_splitk_bf16s: %s (N=128 K=512)' % shape),
        ('bf16s', nothing, -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(X=None), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(Wp=None), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(Y=None), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(ws=None, X=0x1004), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(ld=510), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(ld=508), -1, 'sbev_linear_splitk_bf16s: bad pointers'),
        ('bf16s', dict(X=0x1004), -1, 'sbev_linear_splitk_bf16s: 16-byte alignment'),
        ('bf16s', dict(Wp=0x2008), -1, 'sbev_linear_splitk_bf16s: 16-byte alignment'),
        ('bf16s', dict(ws=0x4004), -1, 'sbev_linear_splitk_bf16s: 16-byte alignment'),
        # ---- sbev_linear_splitk_f16s
        ('f16s', dict(mode=5), -1, 'sbev_linear_splitk_f16s: nprod=5 (3 or 4 image products)'),
        ('f16s', dict(mode=2, up=101, N=128, **nothing), -1, 'sbev_linear_splitk_f16s: nprod=2 (3 or 4 image products)'),
        ('f16s', dict(up=101), -1, 'sbev_linear_splitk_f16s: x_up_log2=101'),
        ('f16s', dict(up=-101, N=128, M=0, **nothing), -1, 'sbev_linear_splitk_f16s: x_up_log2=-101'),
        ('f16s', dict(N=128), -1, 'sbev_linear_splitk_f16s: %s (N=128 K=512)' % shape),
        ('f16s', dict(K=250, pairs=1, **nothing), -1, 'sbev_linear_splitk_f16s: %s (N=256 K=250)' % shape),
        ('f16s', dict(M=-1), -1, 'sbev_linear_splitk_f16s: %s (N=256 K=512)' % shape),
        ('f16s', dict(M=0, **nothing), 0, ''),
        ('f16s', dict(M=0, mode=4, pairs=1, up=100, **nothing), 0, ''),
        ('f16s', nothing, -1, 'sbev_linear_splitk_f16s: bad pointers'),
        ('f16s', dict(scale=None), -1, 'sbev_linear_splitk_f16s: bad pointers'),
        ('f16s', dict(scale=None, pairs=1), -1, 'sbev_linear_splitk_f16s: bad pointers'),
        ('f16s', dict(ws=None, scale=0x5004), -1, 'sbev_linear_splitk_f16s: bad pointers'),
        ('f16s', dict(ld=508), -1, 'sbev_linear_splitk_f16s: bad pointers'),
        ('f16s', dict(X=0x1004), -1, 'sbev_linear_splitk_f16s: 16-byte alignment'),
        ('f16s', dict(scale=0x5004, pairs=1), -1, 'sbev_linear_splitk_f16s: 16-byte alignment'),
        ('f16s', dict(ws=0x4008, mode=4), -1, 'sbev_linear_splitk_f16s: 16-byte alignment'),
        # ---- sbev_linear_splitk_f16s_xdev (no host exponent: no range check; x_scale is required but only 4-byte aligned)
        ('xdev', dict(mode=5), -1, 'sbev_linear_splitk_f16s_xdev: nprod=5 (3 or 4 image products)'),
        ('xdev', dict(mode=0, N=128, **nothing), -1, 'sbev_linear_splitk_f16s_xdev: nprod=0 (3 or 4 image products)'),
        ('xdev', dict(N=128), -1, 'sbev_linear_splitk_f16s_xdev: %s (N=128 K=512)' % shape),
        ('xdev', dict(K=250, **nothing), -1, 'sbev_linear_splitk_f16s_xdev: %s (N=256 K=250)' % shape),
        ('xdev', dict(M=0, **nothing), 0, ''),
        ('xdev', nothing, -1, 'sbev_linear_splitk_f16s_xdev: bad pointers'),
        ('xdev', dict(xscale=None), -1, 'sbev_linear_splitk_f16s_xdev: bad pointers'),
        ('xdev', dict(scale=None), -1, 'sbev_linear_splitk_f16s_xdev: bad pointers'),
        ('xdev', dict(Y=None, Wp=0x2004), -1, 'sbev_linear_splitk_f16s_xdev: bad pointers'),
        ('xdev', dict(ld=256), -1, 'sbev_linear_splitk_f16s_xdev: bad pointers'),
        ('xdev', dict(Wp=0x2004), -1, 'sbev_linear_splitk_f16s_xdev: 16-byte alignment'),
        ('xdev', dict(scale=0x5008), -1, 'sbev_linear_splitk_f16s_xdev: 16-byte alignment'),
        # ---- sbev_linear_bf16s_gen (K = 512 here: the weight-stationary kernel's K = 256 is not what is tested)
        ('gen', dict(mode=4), -1, 'sbev_linear_bf16s_gen: nimg=4 (2 = bf16x3, 3 = bf16x6)'),
        ('gen', dict(mode=5, N=128, **nothing), -1, 'sbev_linear_bf16s_gen: nimg=5 (2 = bf16x3, 3 = bf16x6)'),
        ('gen', dict(N=128), -1, '%s (M=64 N=128 K=512)' % gshape),
        ('gen', dict(K=4128, **nothing), -1, '%s (M=64 N=256 K=4128)' % gshape),
        ('gen', dict(K=48), -1, '%s (M=64 N=256 K=48)' % gshape),
        ('gen', dict(M=-1), -1, '%s (M=-1 N=256 K=512)' % gshape),
        ('gen', dict(M=0, **nothing), 0, ''),
        ('gen', dict(M=0, N=128, **nothing), -1, '%s (M=0 N=128 K=512)' % gshape),
        ('gen', nothing, -1, 'sbev_linear_bf16s_gen: bad pointers / leading dimension'),
        ('gen', dict(Y=None, X=0x1004), -1, 'sbev_linear_bf16s_gen: bad pointers / leading dimension'),
        ('gen', dict(ld=128), -1, 'sbev_linear_bf16s_gen: bad pointers / leading dimension'),
        ('gen', dict(ld=258), -1, 'sbev_linear_bf16s_gen: bad pointers / leading dimension'),
        ('gen', dict(X=0x1004), -1, 'sbev_linear_bf16s_gen: 16-byte alignment'),
        ('gen', dict(bias=0x7004), -1, 'sbev_linear_bf16s_gen: 16-byte alignment'),
        # ---- sbev_linear_f16s_gen: its own two checks, then the shared generator's under the shared prefix
        ('f16gen', dict(mode=5), -1, 'sbev_linear_f16s_gen: nprod=5 (3 or 4 image products)'),
        ('f16gen', dict(mode=2, **nothing), -1, 'sbev_linear_f16s_gen: nprod=2 (3 or 4 image products)'),
        ('f16gen', dict(xscale=None, N=128), -1, 'sbev_linear_f16s_gen: null scale pointer'),
        ('f16gen', dict(scale=None), -1, 'sbev_linear_f16s_gen: null scale pointer'),
        ('f16gen', dict(N=128), -1, '%s (M=64 N=128 K=512)' % gshape),
        ('f16gen', dict(M=0, **nothing), 0, ''),
        ('f16gen', dict(X=None), -1, 'sbev_linear_bf16s_gen: bad pointers / leading dimension'),
        ('f16gen', dict(Wp=0x2008, mode=4), -1, 'sbev_linear_bf16s_gen: 16-byte alignment'),
    ]
    for name, overrides, status, text in table:
        got = call[name](**overrides)
        err = lib.sbev_last_error().decode() if got != 0 else ''
        assert (got, err) == (status, text), (name, overrides, got, err)


def test_bf16s_out_plan_table(lib):
    """sbev_linear_bf16s_out_plan(M, 256, K) -- the slabs a caller provides: the largest of the three out-projection kernels' chunk
    counts -- as a literal table, recorded from the library before the three chunk searches became one; 0 for shapes not covered."""
    plan = lib.sbev_linear_bf16s_out_plan
    Ks = (256, 512, 2048, 4096, 32768, 32800)
    table = {
        1: [2, 4, 16, 32, 64, 64],
        31: [2, 4, 16, 32, 64, 64],
        32: [2, 4, 16, 32, 64, 64],
        33: [2, 4, 16, 32, 64, 64],
        64: [2, 4, 16, 32, 64, 64],
        65: [2, 4, 16, 32, 64, 64],
        96: [2, 4, 16, 32, 64, 64],
        128: [2, 4, 16, 32, 64, 64],
        129: [2, 4, 16, 32, 64, 64],
        256: [2, 4, 16, 32, 64, 64],
        257: [2, 4, 16, 32, 64, 64],
        512: [2, 4, 16, 32, 64, 64],
        900: [2, 4, 16, 32, 32, 32],
        1023: [2, 4, 16, 32, 32, 32],
        1024: [2, 4, 16, 32, 64, 64],
        1025: [2, 4, 16, 32, 51, 51],
        1600: [2, 4, 16, 32, 59, 59],
        2048: [2, 4, 16, 32, 32, 32],
        2112: [2, 4, 16, 28, 31, 31],
        3200: [2, 4, 16, 19, 51, 51],
        3600: [2, 4, 16, 26, 58, 58],
        4096: [2, 4, 16, 16, 16, 16],
        4097: [2, 4, 15, 31, 63, 63],
        8192: [2, 4, 8, 8, 8, 8],
        16384: [2, 4, 4, 4, 4, 4],
        65536: [1, 1, 1, 1, 1, 1],
        100000: [2, 4, 16, 18, 47, 47],
        4194303: [1, 1, 1, 1, 1, 1],
    }
    for M, row in table.items():
        assert [plan(M, 256, K) for K in Ks] == row, (M, [plan(M, 256, K) for K in Ks])
    assert {1, 31, 32, 33, 64, 65, 128, 129, 900, 1023, 1024, 1600, 2112, 3200, 3600, 4096, 4097} <= set(table)
    for M in (1, 900, 4097):
        assert plan(M, 512, 32768) == 0 and plan(M, 128, 32768) == 0 and plan(M, 256, 250) == 0 and plan(M, 256, 224) == 0
        assert plan(M, 256, 32776) == 0          # K % 32
    for K in Ks:
        assert plan(0, 256, K) == 0 and plan(-1, 256, K) == 0 and plan((0x7fffffff >> 9) + 1, 256, K) == 0


def test_product_has_no_cpu_fallback():
    import torch
    from sparsebev_amd import ops
    f = [torch.zeros(1, 6, 2, 2, 4)]
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.msmv_sampling(f, torch.zeros(1, 1, 1, 3), torch.zeros(1, 1, 1, 1))
    # and the product package never imports (or even mentions) the oracle
    for root, _, files in os.walk(os.path.join(ROOT, 'sparsebev_amd')):
        for fn in files:
            if fn.endswith('.py'):
                text = open(os.path.join(root, fn)).read()
                assert 'import oracle' not in text and 'from oracle' not in text and 'oracle.' not in text, fn


def test_splitk_plan_is_a_pure_host_function(lib):
    """sbev_linear_splitk_plan: K splits that fill the GPU once.  Config 2's out-projection (900 x 256 x 32768) runs as
    19 row groups x 2 column groups x 26 splits = 988 wave tasks on the 1024 one-wave-per-SIMD slots."""
    plan = lib.sbev_linear_splitk_plan
    assert plan(900, 256, 32768) == 26
    assert plan(3600, 256, 32768) == 6 and plan(3200, 256, 32768) == 7          # configs 4 and 3 (75 / 67 row groups)
    assert plan(36, 256, 32768) == 64                                           # capped: at least 512 of K per split
    assert plan(900, 250, 32768) >= 1 and plan(900, 256, 1000) == 1             # shapes of the generic tile kernel / tiny K
    assert plan(0, 256, 32768) == 1 and plan(900, 0, 32768) == 1
    assert lib.sbev_linear_splitk_workspace(900, 256, 26) == 900 * 256 * 26 * 4


def test_sampler_refuses_a_slab_beyond_the_32bit_in_slab_offset():
    """Argument validation only (returns before any HIP call, so it runs without a GPU): the forward sampler keeps a
    tap's offset inside one sample-batch slab in 32 bits; a level whose slab does not fit must be refused, not mis-read."""
    import ctypes
    from sparsebev_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    feats = (ctypes.c_void_p * 1)(fake)
    for H, W, ok_expected in ((1024, 1024, True), (8192, 8192, False)):
        C = 64
        hw = (ctypes.c_int32 * 2)(H, W)
        sbo = (ctypes.c_int64 * 1)(6 * H * W * C)
        sv = (ctypes.c_int64 * 1)(H * W * C)
        # Bp = 0: a valid call returns OK before touching the device; an invalid one must fail in validation first
        st = lib.sbev_msmv_fwd(feats, hw, 1, 0, 0, 6, C, 4, 4, 1, sbo, 0, sv, C, fake, fake, fake, 0, 1, 1, None)
        if ok_expected:
            assert st == 0, lib.sbev_last_error()
        else:
            assert st != 0 and b'32-bit' in lib.sbev_last_error()


def test_transformer_refuses_other_code_sizes():
    import pytest
    from sparsebev_amd.transformer import SparseBEVTransformer
    from sparsebev_amd import synthetic as S
    with pytest.raises(ValueError):
        SparseBEVTransformer(256, num_frames=2, num_levels=4, code_size=11, pc_range=S.PC_RANGE)


def test_round2_entry_points_validate_without_gpu(lib):
    """Argument validation of the training / fused entry points returns the documented status before any HIP call."""
    one = ctypes.c_void_p(16)
    pc = (ctypes.c_double * 6)(-51.2, -51.2, -5, 51.2, 51.2, 3)
    # shape coverage table of the fused gather + mixing launch
    assert lib.sbev_sample_mix_supported(4, 64, 4, 8, 4, 4) == 1 and lib.sbev_sample_mix_supported(5, 64, 4, 16, 4, 4) == 1
    assert lib.sbev_sample_mix_supported(4, 64, 4, 2, 4, 4) == 1          # T*P = 8: padded row tile (round 3)
    assert lib.sbev_sample_mix_supported(4, 64, 8, 8, 4, 4) == 1 and lib.sbev_sample_mix_supported(5, 64, 8, 15, 4, 4) == 1     # P = 8; the 15 x 8 shape
    assert lib.sbev_sample_mix_supported(4, 64, 8, 12, 4, 4) == 0 and lib.sbev_sample_mix_supported(4, 64, 6, 4, 4, 4) == 0    # 96 in_points; P = 6
    assert lib.sbev_sample_mix_supported(4, 32, 4, 8, 4, 4) == 0          # C = 32
    assert lib.sbev_sample_mix_supported(4, 64, 4, 8, 1, 4) == 0          # reference layout (gdiv != G)
    # generic GEMM: empty problems are fine, bad leading dimensions are refused
    assert lib.sbev_gemm_f32(None, 0, 8, None, 1, 8, None, 8, 0, 8, 8, 0, None, None) == 0
    assert lib.sbev_gemm_f32(one, 0, 4, one, 1, 8, one, 8, 4, 8, 8, 0, None, None) == -1 and b'leading dimension' in lib.sbev_last_error()
    assert lib.sbev_gemm_f32_workspace(900, 256, 32768) > 0 and lib.sbev_gemm_f32_workspace(900, 32768, 256) == 0
    assert lib.sbev_gemm_f32_workspace(-1, 4, 4) == -1
    # workspaces
    assert lib.sbev_colsum_workspace(900, 256) == 29 * 256 * 4 and lib.sbev_layer_norm_bwd_workspace(900, 256) == (1800 + 2 * 29 * 256) * 4
    # mixing backward: same shape contract as the forward
    assert lib.sbev_adaptive_mixing_bwd_f32(one, one, one, one, one, 4, 4, 32, 32, 128, 1e-5, None) == -1      # C != 64
    assert lib.sbev_adaptive_mixing_bwd_f32(one, one, one, one, one, 4, 4, 30, 64, 128, 1e-5, None) == -1      # Pin % 4
    assert lib.sbev_adaptive_mixing_bwd_f32(None, None, None, None, None, 0, 4, 32, 64, 128, 1e-5, None) == 0  # empty
    # attention backward: head_dim and dropout range
    assert lib.sbev_sasa_bwd_f32(one, 776, one, pc, None, one, one, one, one, 1, 8, 8, 64, 0.0, 0, None) == -1
    assert lib.sbev_sasa_bwd_f32(one, 776, one, pc, None, one, one, one, one, 1, 8, 8, 32, 1.0, 0, None) == -1
    assert lib.sbev_sasa_bwd_f32(None, 776, None, pc, None, None, None, None, None, 0, 8, 8, 32, 0.1, 0, None) == 0
    # LayerNorm backward: width contract
    assert lib.sbev_layer_norm_bwd(one, one, one, one, 1e-5, 0, one, one, one, one, 4, 6, None) == -1
    # sampler backward: mixing-layout gradient needs B' = B*T*G
    feats = (ctypes.c_void_p * 1)(16)
    hw = (ctypes.c_int32 * 2)(4, 4)
    s64 = (ctypes.c_int64 * 1)(6 * 16 * 64)
    sv = (ctypes.c_int64 * 1)(16 * 64)
    assert lib.sbev_msmv_bwd_ex(feats, None, hw, 1, 6, 6, 64, 3, 4, 1, s64, 0, sv, 64, one, one, one, 1, 4, 4, one, one, None) == -1
    assert lib.sbev_dropout_f32(one, one, 16, 1, 1.0, None) == -1 and lib.sbev_dropout_f32(None, None, 0, 1, 0.5, None) == 0
    assert lib.sbev_copy_widen_f32(one, 3, one, 4, None) == -1


def test_query_order_entry_points_validate_without_gpu(lib):
    """round 4: the launch-order sort and switch (sbev_query_order, sbev_decoder_query_order) check their arguments before any HIP call"""
    one = ctypes.c_void_p(16)
    pc = (ctypes.c_double * 6)(-51.2, -51.2, -5, 51.2, 51.2, 3)
    assert lib.sbev_query_order_max() == 4096
    assert lib.sbev_query_order(None, 10, pc, 0, 900, None, None) == 0 and lib.sbev_query_order(None, 10, pc, 2, 0, None, None) == 0      # empty
    assert lib.sbev_query_order(one, 10, pc, 1, 4097, one, None) == -1 and b'at most 4096' in lib.sbev_last_error()
    assert lib.sbev_query_order(one, 1, pc, 1, 8, one, None) == -1          # a row holds at least the two centre columns
    assert lib.sbev_query_order(None, 10, pc, 1, 8, one, None) == -1 and lib.sbev_query_order(one, 10, None, 1, 8, one, None) == -1
    prev = lib.sbev_decoder_query_order(1)
    assert lib.sbev_decoder_query_order(prev) == 1                           # returns the previous setting
    assert lib.sbev_decoder_query_order(prev) == prev


def test_two_byte_relayout_validates_without_gpu(lib):
    """round 4: sbev_nchw_to_nhwc_b16 / _indirect (bf16 / fp16 storage) check their arguments before any HIP call"""
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    assert lib.sbev_nchw_to_nhwc_b16(None, None, 0, 256, 64, None) == 0                       # empty
    assert lib.sbev_nchw_to_nhwc_b16(None, two, 1, 256, 64, None) == -1 and lib.sbev_nchw_to_nhwc_b16(one, None, 1, 256, 64, None) == -1
    assert lib.sbev_nchw_to_nhwc_b16(one, one, 1, 256, 64, None) == -1                        # aliased
    assert lib.sbev_nchw_to_nhwc_b16(one, two, 1, 0, 64, None) == -1 and lib.sbev_nchw_to_nhwc_b16(one, two, 70000, 8, 4, None) == -1
    assert lib.sbev_nchw_to_nhwc_b16_indirect(None, 0, two, 1, 256, 64, None) == -1
    assert lib.sbev_nchw_to_nhwc_b16_indirect(ctypes.c_void_p(12), 0, two, 1, 256, 64, None) == -1      # table not 8-byte aligned
    assert lib.sbev_nchw_to_nhwc_b16_indirect(one, -1, two, 1, 256, 64, None) == -1


def test_round3_training_entry_points_validate_without_gpu(lib):
    """The grouped parameter-gradient launches and the fp16 hi + lo training GEMMs refuse what they do not cover before any HIP call."""
    one = ctypes.c_void_p(16)
    VP = ctypes.c_void_p
    # grad_W on the fp16 kernel: shape coverage (>= 256 tiles of 128 x 128, K >= 32, multiples of 4), 32-bit buffer offsets
    assert lib.sbev_gemm_tn_f16s_ok(256, 32768, 900) == 1 and lib.sbev_gemm_tn_f16s_ok(32768, 256, 900) == 1
    assert lib.sbev_gemm_tn_f16s_ok(256, 256, 900) == 0 and lib.sbev_gemm_tn_f16s_ok(256, 32768, 16) == 0 and lib.sbev_gemm_tn_f16s_ok(258, 32768, 900) == 0
    # contiguous operands past the 32-bit buffer offsets (K * M or K * N >= 2^29) are refused here, so that callers fall back to the
    # exact kernels instead of meeting the launch's refusal: grad_W_pg at Pin 120 (NP = 77824) from B*Q = 6899, grad_W_op (N = 32768) from 16384
    assert lib.sbev_gemm_tn_f16s_ok(77824, 256, 6898) == 1 and lib.sbev_gemm_tn_f16s_ok(77824, 256, 6899) == 0
    assert lib.sbev_gemm_tn_f16s_ok(77824, 256, 7200) == 0 and lib.sbev_gemm_tn_f16s_ok(256, 77824, 7200) == 0
    assert lib.sbev_gemm_tn_f16s_ok(256, 32768, 16383) == 1 and lib.sbev_gemm_tn_f16s_ok(256, 32768, 16384) == 0
    assert lib.sbev_gemm_tn_f16s_ok(32768, 256, 16384) == 0 and lib.sbev_gemm_tn_f16s_ok(256, 32768, 7200) == 1
    assert lib.sbev_gemm_tn_f16s(one, 256, one, one, 32768, one, one, 32768, 256, 256, 900, 0, None) == -1               # too few tiles
    assert lib.sbev_gemm_tn_f16s(one, 256, None, one, 32768, one, one, 32768, 256, 32768, 900, 0, None) == -1            # null scale
    assert lib.sbev_gemm_tn_f16s(one, 128, one, one, 32768, one, one, 32768, 256, 32768, 900, 0, None) == -1             # lda < M
    assert lib.sbev_gemm_tn_f16s(one, 256, one, one, 1 << 22, one, one, 32768, 256, 32768, 900, 0, None) == -1 and b'2 GiB' in lib.sbev_last_error()
    assert lib.sbev_f16s_tensor_scale(one, 6, 4, 6, one, None) == -1                                                    # K % 4
    # split-K Linear with the operand scale in device memory: same shape contract as sbev_linear_splitk_f16s, fp32 X only
    assert lib.sbev_linear_splitk_f16s_xdev(one, one, one, one, None, None, None, None, 1e-5, one, 4, 128, 256, 256, 0, 3, one, None) == -1   # N != 256
    assert lib.sbev_linear_splitk_f16s_xdev(one, None, one, one, None, None, None, None, 1e-5, one, 4, 256, 256, 256, 0, 3, one, None) == -1  # null scale
    assert lib.sbev_linear_splitk_f16s_xdev(None, None, None, None, None, None, None, None, 1e-5, None, 0, 256, 256, 256, 0, 3, None, None) == 0
    # mixing backward that also writes the partial maxima
    assert lib.sbev_adaptive_mixing_bwd_max_f32(one, one, one, one, one, None, 4, 4, 32, 64, 128, 1e-5, None) == -1     # null item_max
    assert lib.sbev_adaptive_mixing_bwd_max_f32(None, None, None, None, None, None, 0, 4, 32, 64, 128, 1e-5, None) == 0  # empty
    # grouped reductions: group / segment limits
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    ptrs = lambda n: (VP * n)(*([16] * n))
    assert lib.sbev_colsum_group(ptrs(17 * 8), ptrs(17), i32(*[4] * 17), i32(*[1] * 17), i32(*[0] * 17), 17, 8, None) == -1      # > 16 groups
    assert lib.sbev_colsum_group(ptrs(8), ptrs(1), i32(4), i32(9), i32(0), 1, 8, None) == -1                                      # > 8 segments
    assert lib.sbev_layer_norm_param_group(ptrs(72), ptrs(72), ptrs(72), ptrs(9), ptrs(9), ptrs(9), ptrs(9), i32(*[4] * 9), i32(*[1] * 9),
                                           i32(*[0] * 9), i32(*[0] * 9), 9, 8, None) == -1                                        # > 8 groups
    assert lib.sbev_layer_norm_bwd_rows(one, one, one, one, 1e-5, 0, one, one, 4, 6, None) == -1                                  # N % 4
    assert lib.sbev_gemm_f32_multi_workspace(256, 256, 900, 6) > 0 and lib.sbev_gemm_f32_multi_workspace(256, 256, 900, 9) == -1


def test_chain_pack_size_is_a_pure_host_function(lib):
    """sbev_decoder_chain_pack_floats: the size of the lane-ordered weight image of the row-chain kernels for the
    reference's layer shape, 0 for shapes the kernels do not cover; the pack call validates its arguments on the host."""
    from sparsebev_amd.runtime import DecoderConfig, DecoderWeights
    cfg = DecoderConfig()
    cfg.B = cfg.Q = 1
    cfg.T, cfg.N, cfg.G, cfg.P, cfg.L = 8, 6, 4, 4, 4
    cfg.D, cfg.H, cfg.ffn, cfg.num_classes, cfg.code_size, cfg.attn_in_rows = 256, 8, 512, 10, 10, 776
    n = lib.sbev_decoder_chain_pack_floats(ctypes.byref(cfg))
    mats = (512 * 256 + 256 * 512 + 5 * 256 * 256 + 2 * 64 * 256      # ffn, cls0 / reg0 / cls3 / reg2 / pe3, cls6 / reg4 (64-column groups)
            + 832 * 256 + 256 * 256 + 128 * 256)                        # attn_in (776 -> 13 groups), attn_out, sampling (112 -> 2 groups)
    assert n > mats and (n - mats) % 64 == 0 and n - mats < 16384         # + the small vectors
    cfg.ffn = 1024
    assert lib.sbev_decoder_chain_pack_floats(ctypes.byref(cfg)) == 0
    cfg.ffn, cfg.code_size = 512, 8
    assert lib.sbev_decoder_chain_pack_floats(ctypes.byref(cfg)) == 0
    w = DecoderWeights()
    assert lib.sbev_decoder_chain_pack(ctypes.byref(cfg), ctypes.byref(w), None, None) == -1                  # SBEV_EINVAL
    assert b'sbev_decoder_chain_pack' in lib.sbev_last_error()
    assert lib.sbev_decoder_row_chain(1) == 0


def test_build_tracks_textual_include_fragments(monkeypatch):
    """msmv_chunk.inc is #included by msmv_sampling.hip AND mixing.hip (the fused gather + mixing kernel): editing it must make
    both objects stale -- the .so ships prebuilt to the GPU box, so a stale object would go unnoticed.  Also
    every #include "..." of every translation unit has to be in the dependency list at all."""
    from sparsebev_amd.csrc import build
    deps = {os.path.basename(d) for d in build.header_deps()}
    assert 'msmv_chunk.inc' in deps and 'sbev_common.hpp' in deps and 'sbev_hip.h' in deps
    for src in build.UNITS:
        text = open(os.path.join(build.HERE, src)).read()
        for inc in re.findall(r'#include\s+"([^"]+)"', text):
            assert os.path.basename(inc) in deps, '%s includes %s, which the build does not track' % (src, inc)
    for hdr in [d for d in build.header_deps() if d.endswith(('.hpp', '.inc'))]:       # headers including headers
        for inc in re.findall(r'#include\s+"([^"]+)"', open(hdr).read()):
            assert os.path.basename(inc) in deps, '%s includes %s, which the build does not track' % (hdr, inc)
    # touch msmv_chunk.inc (virtually: a patched mtime) -> every unit that can include it is stale, so in particular its two users
    real = os.path.getmtime
    chunk = os.path.join(build.HERE, 'msmv_chunk.inc')
    newest = max(real(build.object_path(s)) for s in build.UNITS if os.path.exists(build.object_path(s)))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda f: newest + 10.0 if os.path.abspath(f) == chunk else real(f))
    stale = build.stale_units()
    assert 'msmv_sampling.hip' in stale and 'mixing.hip' in stale
    monkeypatch.undo()
    users = [s for s in build.UNITS if re.search(r'#include\s+"msmv_chunk\.inc"', open(os.path.join(build.HERE, s)).read())]
    assert sorted(users) == ['mixing.hip', 'msmv_sampling.hip']
