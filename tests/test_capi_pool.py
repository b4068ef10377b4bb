"""Refusal tables of the keyed frame pool's entry points (sbev_msmv_fwd_pool, sbev_sample_mix_pool) and of the decoder config's
slot_table, without a GPU: fake pointers, validation returns before any HIP call; an accepted row is an empty call (B = 0 or Q = 0)."""
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


def _pool_entry_points(lib):
    """sbev_msmv_fwd_pool and sbev_sample_mix_pool (fp32 and pair output, with and without a launch order), each as call(**overrides) over
    ONE shared description.  Base: 4 levels of 4 x 4 pixels, grouped channels-last [B*n_slots*N, H, W, G*C] with B, T, G, N, C, Q, P =
    1, 2, 4, 6, 64, 3, 4, mixing layout, a 2-slot pool whose device table sits at a fake, aligned address."""
    M = 6
    base = dict(L=4, hw=[4, 4] * M, dtype=0, B=1, T=2, G=4, N=6, C=64, Q=3, P=4, gdiv=4, feats=[0x1000] * M,
                sbo=[6 * 16 * 256] * M, sg=64, sv=[16 * 256] * M, spx=256, ptr=0x1000, layout=1, table=0x2000, slots=None, n_slots=2,
                Pout=128, up=9, order=None)

    def args(o):
        d = dict(base, **o)
        d.setdefault('Bp', d['B'] * d['T'] * d['G'])
        arr = lambda ct, v: None if v is None else (ct * len(v))(*v)
        vp = lambda v: None if v is None else ctypes.c_void_p(v)
        d.update(feats=arr(ctypes.c_void_p, d['feats']), hw=arr(ctypes.c_int32, d['hw']), sbo=arr(ctypes.c_int64, d['sbo']),
                 sv=arr(ctypes.c_int64, d['sv']), slots=arr(ctypes.c_int32, d['slots']), ptr=vp(d['ptr']), table=vp(d['table']),
                 order=vp(d['order']))
        d['pyr'] = (d['gdiv'], d['sbo'], d['sg'], d['sv'], d['spx'], d['ptr'], d['ptr'])      # ... gdiv, strides, loc, weights
        return d

    def fwd(d):
        return lib.sbev_msmv_fwd_pool(d['feats'], d['hw'], d['L'], d['dtype'], d['Bp'], d['N'], d['C'], d['Q'], d['P'], *d['pyr'], d['ptr'],
                                      d['layout'], d['T'], d['G'], d['table'], d['n_slots'], None)

    def mix(d, pairs):
        return lib.sbev_sample_mix_pool(d['feats'], d['hw'], d['L'], d['dtype'], d['B'], d['N'], d['Q'], d['T'], d['G'], d['P'], d['C'], *d['pyr'][1:],
                                        d['slots'], d['table'], d['n_slots'], d['ptr'], d['ptr'], d['Pout'], 1e-5, pairs, d['up'], d['order'], None)

    return {'fwd_pool': lambda **o: fwd(args(o)), 'mix_pool': lambda **o: mix(args(o), 0), 'mix_pool_pairs': lambda **o: mix(args(o), 1)}


def test_pool_entry_points_refusal_table(lib):
    """Status and message per entry point.  The cases the pool adds to the samplers' shared checks (pinned for the other entry points in
    test_capi_symbols.py): null table, T outside 1 .. SBEV_MAX_FRAMES, n_slots < 1, gdiv != G, both slot forms given (expressible only
    where an entry point takes both: the fused launch) -- and NOT n_slots < T, which is the ring's rule: with duplicates in a window a
    pool of fewer slots than frames is meaningful.  The table itself is device memory and is never read here."""
    call = _pool_entry_points(lib)
    FWD, MIX = ('fwd_pool',), ('mix_pool', 'mix_pool_pairs')
    OK = (0, b'')
    unsupported = (-1, b'sbev_sample_mix_f32: needs L in {4,5}')
    need = b'need 1 <= T <= 16, n_slots >= 1, gdiv == G'
    table = [
        (dict(B=0), {FWD + MIX: OK}),
        (dict(Q=0), {FWD + MIX: OK}),
        # null table: the stand-alone sampler refuses (also an empty call); the fused launch without any slot form is the dense pyramid
        (dict(table=None), {FWD: (-1, b'sbev_msmv_fwd_pool: slot_table is null')}),
        (dict(B=0, table=None), {FWD: (-1, b'sbev_msmv_fwd_pool: slot_table is null'), MIX: OK}),
        (dict(table=0x2002), {FWD: (-1, b'sbev_msmv_fwd_pool: slot_table must be 4-byte aligned'), MIX: (-1, b'sbev_sample_mix_f32: slot_table must be 4-byte aligned')}),
        # T outside 1 .. 16
        (dict(T=17), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need), MIX: unsupported}),
        (dict(T=0, Bp=8), {FWD: (-1, b"sbev_msmv_fwd: B'=8 is not B*T*G (T=0, G=4)"), MIX: unsupported}),
        (dict(T=17, layout=0), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need)}),
        (dict(T=0, Bp=8, layout=0), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need)}),
        # n_slots < 1 -- and n_slots < T is fine (the ring's entry point refuses n_slots = 1 at T = 2)
        (dict(n_slots=0), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need), MIX: (-1, b'sbev_sample_mix_f32: ' + need)}),
        (dict(n_slots=-1), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need), MIX: (-1, b'sbev_sample_mix_f32: ' + need)}),
        (dict(n_slots=1, ptr=0), {FWD: (-1, b'sbev_msmv_fwd: null loc/weights/out'), MIX: (-1, b'sbev_sample_mix_f32: null pointer')}),
        (dict(n_slots=1, Q=0), {FWD + MIX: OK}),
        # gdiv != G (the fused launch has no gdiv argument: its pyramid is grouped by G by construction)
        (dict(gdiv=1), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need)}),
        (dict(layout=0, T=2, G=2), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need)}),
        # B' is not B*T*G
        (dict(Bp=12, layout=0), {FWD: (-1, b'sbev_msmv_fwd_pool: ' + need)}),
        # both slot forms
        (dict(slots=[0, 1]), {MIX: (-1, b'sbev_sample_mix_f32: give frame_slots (host, by value) or slot_table (device), not both')}),
        (dict(slots=[0, 1], table=None, n_slots=1), {MIX: (-1, b'T <= 16, n_slots >= T')}),      # the by-value ring through the general form: its rule
        (dict(slots=[0, 2], table=None), {MIX: (-1, b'sbev_sample_mix_f32: frame_slots[1] = 2 out of range')}),
        # the checks every sampler entry point shares still come first
        (dict(hw=None), {FWD: (-1, b'sbev_msmv_fwd: null descriptor array'), MIX: (-1, b'sbev_sample_mix_f32: null descriptor array')}),
        (dict(L=6), {FWD: (-1, b'sbev_msmv_fwd: L=6 not in 1..5'), MIX: unsupported}),
        (dict(C=6, B=0), {FWD: (-1, b'sbev_msmv_fwd: C=6 must be a positive multiple of 4'), MIX: unsupported}),
        (dict(dtype=3), {FWD: (-1, b'sbev_msmv_fwd: feat_dtype 3'), MIX: (-1, b'sbev_sample_mix_f32: feat_dtype 3')}),
        (dict(ptr=0), {FWD: (-1, b'sbev_msmv_fwd: null loc/weights/out'), MIX: (-1, b'sbev_sample_mix_f32: null pointer')}),
        (dict(Pout=64), {MIX: (-1, b'sbev_sample_mix_f32: built for 128 out points')}),
        # the fused launch's own arguments
        (dict(B=0, up=101), {('mix_pool_pairs',): (-1, b'sbev_sample_mix_pool: up_log2=101'), ('mix_pool',): OK}),
        (dict(order=0x1002), {MIX: (-1, b'sbev_sample_mix_f32: order must be 4-byte aligned')}),
    ]
    for overrides, expected in table:
        for names, (status, text) in expected.items():
            for name in names:
                got = call[name](**overrides)
                err = lib.sbev_last_error() if got != 0 else b''
                assert got == status and text in err, (name, overrides, got, err)


def test_decoder_config_slot_table_is_mirrored_and_validated(lib):
    """sbev_decoder_config.slot_table: appended at the end of the struct and mirrored by the ctypes struct; non-null needs n_slots > 0;
    the planner treats the pool as it treats the ring (no on-demand relayout)."""
    from sparsebev_amd.runtime import DecoderConfig
    assert DecoderConfig._fields_[-1][0] == 'slot_table' and DecoderConfig._fields_[-2][0] == 'pc_range'
    assert DecoderConfig.slot_table.offset == DecoderConfig.pc_range.offset + 48 and ctypes.sizeof(DecoderConfig) == DecoderConfig.slot_table.offset + 8
    cfg = DecoderConfig()
    cfg.B, cfg.Q = 1, 16
    cfg.T, cfg.N, cfg.G, cfg.P, cfg.L = 8, 6, 4, 4, 4
    cfg.D, cfg.H, cfg.ffn, cfg.num_classes, cfg.code_size, cfg.attn_in_rows = 256, 8, 512, 10, 10, 776
    cfg.num_layers, cfg.out_points = 6, 128
    for l in range(4):
        cfg.hw[l][0], cfg.hw[l][1] = 16, 16
    assert lib.sbev_decoder_lazy_supported(ctypes.byref(cfg)) == 1
    cfg.slot_table = 0x2000
    cfg.n_slots = 0
    from sparsebev_amd.runtime import DecoderWeights
    w = DecoderWeights()
    assert lib.sbev_decoder_launches_per_layer(ctypes.byref(cfg), ctypes.byref(w)) == -1
    assert b'slot_table (keyed frame pool) needs n_slots > 0' in lib.sbev_last_error()
    cfg.n_slots = 3                                   # below T: legal for the pool
    assert lib.sbev_decoder_launches_per_layer(ctypes.byref(cfg), ctypes.byref(w)) > 0
    assert lib.sbev_decoder_lazy_supported(ctypes.byref(cfg)) == 0          # like the ring: resident slots are never relayouted on demand
    cfg.slot_table = None
    assert lib.sbev_decoder_lazy_supported(ctypes.byref(cfg)) == 0          # (the by-value ring)


def test_pool_pyramid_is_not_mistaken_for_the_ring():
    """PoolPyramid carries slot_table and no frame_slots (that attribute marks the by-value ring); utils.slot_resident knows both."""
    from sparsebev_amd import cache, utils

    class Ring:
        frame_slots = [0, 1]

    class Pool:
        slot_table = object()

    assert utils.slot_resident(Ring()) and utils.slot_resident(Pool()) and not utils.slot_resident([]) and not utils.slot_resident(object())
    assert not hasattr(cache.PoolPyramid, 'frame_slots')
    import inspect
    assert 'frame_slots' not in inspect.getsource(cache.PoolPyramid.__init__)
    with pytest.raises(ValueError):
        cache.FramePool(4, n_slots=17)
    pool = cache.FramePool(4)
    assert pool.n_slots == 16 and pool.T == 4 and pool.slot_table is None
    assert pool.missing([['a', 'a', 'a', 'a']]) == [(0, 'a')] and pool.B == 1
