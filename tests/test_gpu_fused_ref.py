"""The fused gather + adaptive-mixing launch (sbev_sample_mix_f32 / _pairs_f16 and their _ordered forms) against a yardstick that shares
no code with it: the whole launch restated in fp64 on the CPU -- the oracle's sampler on the CUDA kernel's semantics followed by
relu(LN(x @ M)), relu(LN(S @ .)) -- at the smallest shape that reaches each instantiation family (row tiles 1 .. 4 tuned, padded tiles,
the 8-tile k-split path with 4 and 8 points per frame, 4 / 5 levels, fp32 / bf16 / fp16 storage, the frame ring, an ordered walk).
tests/test_gpu_fused.py and tests/test_gpu_order.py hold the launch bit-identical to the two launches it replaces; all three kernels
share the sampler's chunk code and the LayerNorm / MFMA body, so an error there moves both sides together.  Here it cannot.

The pair-format entry points (the operand format of the fp16 out-projection, what the decoder runs in its default GEMM mode) are
checked twice: bit for bit against dense.f16s_pairs of the fp32 launch, and decoded on the host against hi = RNE_fp16(y 2^u),
|hi + lo - y 2^u| <= max(|y 2^u| 2^-23, 2^-25) -- the bound tests/test_gpu_bf16s.py holds the stand-alone split to.

The reference helpers themselves are tested on the CPU (the tests here without the gpu mark)."""
import functools
import math

import pytest
import torch

from oracle import sparsebev_oracle as O
from sparsebev_amd import synthetic as S

gpu = pytest.mark.gpu
DEV = 'cuda:0'
N_VIEWS, G, C, POUT, EPS = 6, 4, 64, 128, 1e-5
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


# ---- the reference: plain torch on the CPU ----------------------------------------------------------------------------------------
def gather_ref(levels, B, T, loc, weights, dtype=torch.float64, frame_slots=None, n_slots=0):
    """ops.msmv_sampling_nhwc / msmv_sampling_ring with OUT_MIX, evaluated in `dtype`: levels[l] [B*T*6 (ring: B*n_slots*6), H, W, G*C]
    in any storage type (widened exactly), loc [B*T*G, Q, P, 3] fp32, weights [B*T*G, Q, P, L] -> [B, Q, G, T*P, C], in-point t*P + p.
    The sampler is the oracle's restatement of the CUDA kernel; with an fp32 loc it forms y (H-1), x (W-1), z (N-1) in fp32 like the
    kernel and does everything behind them -- view rounding, floor, range test, interpolation and level weights, sums -- in `dtype`."""
    Q, P = loc.shape[1:3]
    cl = []
    for f in levels:
        H, W = f.shape[1:3]
        f = f.to(dtype).reshape(B, -1, N_VIEWS, H, W, G, C)                    # [B, T or n_slots, view, H, W, g, c]
        if frame_slots is not None:
            assert f.shape[1] == n_slots
            f = f[:, list(frame_slots)]                                        # logical frame t <- physical slot frame_slots[t]
        assert f.shape[1] == T
        cl.append(f.permute(0, 1, 5, 2, 3, 4, 6).reshape(B * T * G, N_VIEWS, H, W, C))      # sample batch b' = (b*T + t)*G + g
    x = O.msmv_sampling_kernel_semantics(cl, loc, weights.to(dtype))           # [B', Q, C, P]
    return x.reshape(B, T, G, Q, C, P).permute(0, 3, 2, 1, 5, 4).reshape(B, Q, G, T * P, C)


def mix_ref(x, params):
    """x [B, Q, G, Pin, C], params [B, Q, G*(C*C + POUT*Pin)] -> (y [B, Q, G*POUT*C], variance of every item's first LayerNorm
    [B, Q, G]), in x's dtype: relu(LN_[Pin,C](x @ M)), relu(LN_[POUT,C](S @ .)), eps 1e-5 (the formula of
    tests/test_gpu_dense.py::test_adaptive_mixing_core_vs_fp64)."""
    B, Q, _, Pin, _ = x.shape
    prm = params.reshape(B, Q, G, C * C + POUT * Pin).to(x.dtype)
    M = prm[..., :C * C].reshape(B, Q, G, C, C)
    Sm = prm[..., C * C:].reshape(B, Q, G, POUT, Pin)
    z = x @ M
    y = torch.relu(torch.nn.functional.layer_norm(z, [Pin, C], eps=EPS))
    y = torch.relu(torch.nn.functional.layer_norm(Sm @ y, [POUT, C], eps=EPS))
    return y.reshape(B, Q, G * POUT * C), z.var((-2, -1), unbiased=False)


def sample_mix_ref(inp, dtype=torch.float64):
    x = gather_ref(inp['levels'], inp['B'], inp['T'], inp['loc'], inp['w'], dtype, inp['slots'], inp['n_slots'])
    return mix_ref(x, inp['params'])


def decode_pairs(words):
    """int32 pair words -> (hi, lo) as fp16 tensors on the host: hi in the low half of the word, lo in the high half"""
    halves = words.cpu().contiguous().view(torch.int16).reshape(*words.shape, 2)      # little endian: [..., 0] = low half
    return halves[..., 0].view(torch.float16), halves[..., 1].view(torch.float16)


def pair_bound(v):
    """the bound of the split on v = y 2^u (float64): 11 + 11 significand bits and lo's sign cover an fp32 to 2^-23 relative; a lo
    below fp16's normal range is rounded to the subnormal spacing 2^-24, half of it absolute"""
    return torch.maximum(v.abs() * 2.0 ** -23, torch.full_like(v, 2.0 ** -25))


# ---- cases: (B, Q, T, pyramid, storage, P[, 'ring' | 'order']), each the smallest that reaches its instantiation ----------------------
RING_SLOTS, RING_N = [4, 0, 5, 2], 6
CASES = {
    'pin4_idle_waves': (2, 9, 1, 'tiny', F32, 4),            # one frame: waves 1..3 of the gather have none
    'pin8_p8': (1, 9, 1, 'tiny5', BF16, 8),
    'two_frames': (1, 9, 2, 'tiny', F16, 4),                 # no second frame round
    'pin16_rt1': (1, 12, 4, 'tiny5', F32, 4),                # tuned, 1 row tile
    'pin12_pad': (1, 12, 3, 'tiny', F32, 4),                 # padded row tile
    'pin32_bench': (1, 10, 8, 'tiny', F32, 4),               # the benchmark's instantiation
    'pin64_rt4': (1, 8, 16, 'tiny', BF16, 4),                # tuned, 4 row tiles
    'pin64_p8': (1, 8, 8, 'tiny5', F32, 8),
    'pin116_ksplit': (1, 6, 29, 'tiny', F32, 4),
    'pin120_p4': (1, 6, 30, 'tiny5', F16, 4),
    'pin120_p8': (1, 6, 15, 'tiny', BF16, 8),
    'ring': (2, 7, 4, 'tiny', F32, 4, 'ring'),               # 6 slots, logical frames in slots [4, 0, 5, 2]
    'ordered': (2, 9, 8, 'tiny5', BF16, 4, 'order'),         # walked in a shuffled permutation of the B*Q rows
}
NAMES = list(CASES)


def make_inputs(B, Q, T, pyr, dtype, P, kind=None, seed=0):
    """the distributions of tests/test_gpu_fused.py, drawn on the CPU: loc in [-0.15, 1.15] (a border band and outside points), view k/5,
    softmax level weights, params ~ 0.3 N(0, 1)"""
    _, _, sizes = S.PYRAMIDS[pyr]
    L = len(sizes)
    g = torch.Generator().manual_seed(1000 * seed + B * 100 + Q + T)
    frames = RING_N if kind == 'ring' else T
    levels = [torch.randn(B * frames * N_VIEWS, h, w, G * C, generator=g).to(dtype) for h, w in sizes]
    loc = torch.rand(B * T * G, Q, P, 3, generator=g) * 1.3 - 0.15
    loc[..., 2] = torch.randint(0, 6, (B * T * G, Q, P), generator=g).float() / 5
    w = torch.softmax(torch.randn(B * T * G, Q, P, L, generator=g), -1)
    params = torch.randn(B, Q, G * (C * C + POUT * T * P), generator=g) * 0.3
    order = torch.randperm(B * Q, generator=g).int() if kind == 'order' else None
    return dict(B=B, Q=Q, T=T, P=P, L=L, levels=levels, loc=loc, w=w, params=params, order=order,
                slots=RING_SLOTS if kind == 'ring' else None, n_slots=RING_N if kind == 'ring' else 0)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return make_inputs(*CASES[name])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(fp64 result, first-LayerNorm variances, the same formula evaluated in plain fp32 on the CPU) -- computed once, never written to"""
    inp = case_inputs(name)
    y64, var1 = sample_mix_ref(inp, torch.float64)
    y32, _ = sample_mix_ref(inp, torch.float32)
    return y64, var1, y32


def launch(inp, up_log2=None, order='own', loc=None):
    """ops.sample_mix on the device copies of a case's inputs -> host tensor; order 'own': the case's (None unless it is the ordered one)"""
    from sparsebev_amd import ops
    order = inp['order'] if isinstance(order, str) else order
    y = ops.sample_mix([f.to(DEV) for f in inp['levels']], inp['B'], inp['T'], G, (inp['loc'] if loc is None else loc).to(DEV),
                       inp['w'].to(DEV), inp['params'].to(DEV), POUT, frame_slots=inp['slots'], n_slots=inp['n_slots'],
                       order=None if order is None else order.to(DEV), up_log2=up_log2)
    assert y.shape == (inp['B'], inp['Q'], G * POUT * C) and y.dtype == (torch.float32 if up_log2 is None else torch.int32)
    return y


# ---- the helpers themselves, on the CPU -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'ring'])
def test_reference_equals_the_oracle_sampler_then_mixing(kind):
    """in fp32 the helper is the oracle's own regroup + sampler and the mixing formula, item by item: same numbers, bit for bit"""
    B, Q, T, P = 2, 3, 4 if kind else 3, 4
    inp = make_inputs(B, Q, T, 'tiny', F32, P, kind, seed=1)
    got, _ = sample_mix_ref(inp, torch.float32)
    levels = inp['levels']
    if kind:                                                                   # ops.msmv_sampling_ring: logical frame t is physical slot frame_slots[t]
        levels = [torch.stack([f.reshape(B, RING_N, N_VIEWS, *f.shape[1:])[:, s] for s in RING_SLOTS], 1).flatten(0, 2) for f in levels]
    nchw = [f.permute(0, 3, 1, 2).reshape(B, T * N_VIEWS, G * C, *f.shape[1:3]) for f in levels]      # the reference's [B, T*N, G*C, H, W]
    x = O.msmv_sampling_kernel_semantics(O.regroup_features(nchw, channel_last=True), inp['loc'], inp['w'])      # [B*T*G, Q, C, P]
    prm = inp['params'].reshape(B, Q, G, -1)
    for b in range(B):
        for q in range(Q):
            for g in range(G):
                xi = torch.cat([x[(b * T + t) * G + g, q].t() for t in range(T)])                      # [T*P, C], row t*P + p
                M, Sm = prm[b, q, g, :C * C].reshape(C, C), prm[b, q, g, C * C:].reshape(POUT, T * P)
                y = torch.relu(torch.nn.functional.layer_norm(xi @ M, [T * P, C], eps=EPS))
                y = torch.relu(torch.nn.functional.layer_norm(Sm @ y, [POUT, C], eps=EPS))
                assert torch.equal(got[b, q].reshape(G, POUT * C)[g], y.reshape(-1)), (b, q, g)


@pytest.mark.parametrize('kind,P,dtype', [(None, 4, torch.float64), (None, 8, torch.float32), ('ring', 4, torch.float64)])
def test_reference_gather_reads_the_slab_and_row_it_should(kind, P, dtype):
    """features that hold their own (image, group) index in every pixel and channel, interior points (all four corners of every level in
    the map, level weights summing to 1): row t*P + p of item (b, q, g) must read exactly image (b*T + t)*6 + view (ring: slot
    frame_slots[t] of sample b) and group g, with the view of ITS point (b, t, g, q, p)"""
    B, Q, T = 2, 3, 4
    inp = make_inputs(B, Q, T, 'tiny', F32, P, kind, seed=2)
    frames = RING_N if kind else T
    code = (torch.arange(B * frames * N_VIEWS)[:, None] * G + torch.arange(G)[None]).float()           # [image, group]
    levels = [code[:, None, None, :, None].expand(-1, h, w, G, C).reshape(-1, h, w, G * C).contiguous() for h, w in S.PYRAMIDS['tiny'][2]]
    loc = inp['loc'].clone()
    loc[..., :2] = loc[..., :2].clamp(0.05, 0.95)
    x = gather_ref(levels, B, T, loc, inp['w'], dtype, inp['slots'], inp['n_slots'])
    assert x.shape == (B, Q, G, T * P, C) and x.dtype == dtype
    view = (loc[..., 2] * 5).round().long().reshape(B, T, G, Q, P)
    for b in range(B):
        for t in range(T):
            frame = b * frames + (RING_SLOTS[t] if kind else t)
            for g in range(G):
                want = ((frame * N_VIEWS + view[b, t, g]) * G + g).to(dtype)                           # [Q, P]
                got = x[b, :, g, t * P:(t + 1) * P]                                                     # [Q, P, C]
                assert (got - want[..., None]).abs().max() < 0.01, (b, t, g)                            # (codes are integers: 1 apart)


def test_reference_forms_the_coordinate_products_in_fp32():
    """the tap a point lands on is decided by fp32(y (H-1)), as in the kernel: a coordinate whose fp32 product rounds up to an integer
    row reads that row alone in the fp64 evaluation too (in all-fp64 arithmetic it would sit a hair below, between two rows)"""
    H, W = 8, 22
    y = torch.tensor(3.0 / 7.0)                                                                         # fp32(3/7) * 7 rounds to 3.0 exactly
    assert float(y * 7) == 3.0 and float(y.double() * 7) != 3.0
    f = torch.arange(H, dtype=torch.float64)[None, None, :, None, None].expand(1, N_VIEWS, H, W, C).contiguous()      # pixel value = its row
    loc = torch.tensor([0.5, float(y), 0.0]).reshape(1, 1, 1, 3)
    out = O.msmv_sampling_kernel_semantics([f], loc, torch.ones(1, 1, 1, 1, dtype=torch.float64))
    assert out.dtype == torch.float64 and torch.equal(out, torch.full_like(out, 3.0))


def test_pair_decoder_and_the_bound_of_the_split():
    """the host-side decoder and the bound (d) holds the kernel to, on the split written out in torch: hi = RNE_fp16(v), lo = RNE_fp16(v - hi)
    over the whole range a LayerNorm output can take (|y| <= sqrt(n - 1) = sqrt(8191)), down through fp16's subnormals, and zeros"""
    ymax = math.sqrt(8191.0)
    assert ymax * 2 ** 9 < 65504                                                                        # 46338: the decoder's 2^9 keeps hi finite
    g = torch.Generator().manual_seed(3)
    y = torch.cat([torch.rand(20000, generator=g) * ymax, torch.tensor([ymax, 0.0, -0.0, 1.0, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25]),
                   torch.rand(20000, generator=g) * torch.exp2(-torch.rand(20000, generator=g) * 40),  # 2^-40 .. 1: through the subnormals
                   -torch.rand(1000, generator=g) * ymax, torch.zeros(16)])
    reached = False
    for u in (0, 4, 9):
        v = y * 2.0 ** u                                                                                # exact
        assert float(v.abs().max()) < 65504
        hi = v.half()
        lo = (v - hi.float()).half()                                                                    # (the subtraction is exact)
        words = torch.stack([hi, lo], -1).view(torch.int32).squeeze(-1)
        dhi, dlo = decode_pairs(words)
        assert torch.equal(dhi.view(torch.int16), hi.view(torch.int16)) and torch.equal(dlo.view(torch.int16), lo.view(torch.int16))
        assert bool(((words[v == 0] & 0x7fff7fff) == 0).all())                                          # zeros: no bit but hi's sign
        assert torch.isfinite(dhi).all()
        err = (dhi.double() + dlo.double() - v.double()).abs()
        assert bool((err <= pair_bound(v.double())).all()), float((err / pair_bound(v.double())).max())
        reached = reached or bool((err == pair_bound(v.double())).any())
    assert reached                                                                                      # the bound is tight: 2^-25 is lost at v = 2^-25
    # the layout: hi in the LOW half
    one = torch.tensor([1.0]).half()
    w1 = torch.stack([one, torch.zeros(1).half()], -1).view(torch.int32)
    assert int(w1) == 0x3c00


# ---- (a) fp32 output against the fp64 reference ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', NAMES)
def test_fused_launch_vs_fp64(name):
    """max |got - ref| < 2e-5, the project's bound for this operation at these parameter magnitudes (test_adaptive_mixing_core_vs_fp64);
    the gather adds input rounding of order 1e-7 below the first LayerNorm.  Printed per case: max / rms error of the kernel beside the
    error of the same formula evaluated in plain fp32 on the CPU."""
    inp = case_inputs(name)
    ref, var1, y32 = case_reference(name)
    # what keeps the comparison honest, asserted on the REFERENCE: no near-constant item (it would amplify input rounding by up to
    # 1 / sqrt(eps)) -- the coarsest level, 1 x 3, is hit by every point of these distributions -- so that no element is left out
    assert var1.shape == (inp['B'], inp['Q'], G) and float(var1.min()) >= 1e-2, float(var1.min())
    got = launch(inp).cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d, d32 = got - ref, y32.double() - ref
    print('fused vs fp64 %-14s Pin %3d  kernel max %.2e rms %.2e | fp32 on the CPU max %.2e rms %.2e | min LN-1 variance %.2e'
          % (name, inp['T'] * inp['P'], d.abs().max(), d.pow(2).mean().sqrt(), d32.abs().max(), d32.pow(2).mean().sqrt(), var1.min()))
    assert got.abs().max() > 1 and d.abs().max().item() < 2e-5


# ---- (b) items that sample nothing ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', ['pin32_bench', 'pin12_pad', 'pin120_p4'])
def test_items_that_sample_nothing_are_exact_zeros(name):
    """every point of one query far outside every map: both LayerNorms see exact zeros, so its four items are exactly 0.0 (pair words
    0x00000000); every other item is untouched, bit for bit"""
    inp = case_inputs(name)
    B, Q, T, P = inp['B'], inp['Q'], inp['T'], inp['P']
    q0 = Q // 2
    loc = inp['loc'].clone()
    loc[:, q0, :, :2] = 5.0
    ref, _ = mix_ref(gather_ref(inp['levels'], B, T, loc, inp['w']), inp['params'])
    assert bool((ref[:, q0] == 0).all())                                                                # the reference agrees on what "nothing" gives
    base, got, pairs = launch(inp).cpu(), launch(inp, loc=loc).cpu(), launch(inp, up_log2=9, loc=loc).cpu()
    others = [q for q in range(Q) if q != q0]
    assert torch.equal(got[:, q0].contiguous().view(torch.int32), torch.zeros_like(pairs[:, q0]))                    # +0.0, not -0.0
    assert torch.equal(pairs[:, q0], torch.zeros_like(pairs[:, q0]))
    assert torch.equal(got[:, others], base[:, others]) and bool((base[:, q0].reshape(B, G, -1).abs().amax(-1) > 0).all())
    assert (got.double() - ref).abs().max().item() < 2e-5


# ---- (c) pair format, bit for bit -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('u', [9, 0])
@pytest.mark.parametrize('name', NAMES)
def test_pair_launch_equals_the_split_of_the_fp32_launch(name, u):
    from sparsebev_amd import dense, ops
    inp = case_inputs(name)
    y = launch(inp)
    assert torch.equal(launch(inp, up_log2=u), dense.f16s_pairs(y, u))
    if u == 9:                                                                                          # sbev_sample_mix_pairs_f16_ordered: any order, same words
        g = torch.Generator().manual_seed(11)
        bbox = torch.rand(inp['B'], inp['Q'], 10, generator=g).to(DEV)
        for order in (ops.query_order(bbox, S.PC_RANGE), torch.randperm(inp['B'] * inp['Q'], generator=g).int()):
            assert torch.equal(launch(inp, up_log2=u, order=order), dense.f16s_pairs(y, u))


@gpu
def test_pair_launch_with_nonfinite_border_pixels():
    """test_fused_launch_with_nonfinite_border_pixels (Inf in every border pixel of the finest level) in pair mode: the same items are
    dead -- all words 0 -- and every word equals the split of the fp32 launch"""
    from sparsebev_amd import dense, ops
    B, Q, T, P = 1, 200, 4, 4
    _, _, sizes = S.PYRAMIDS['tiny5']
    L = len(sizes)
    g = torch.Generator().manual_seed(77)
    levels = [torch.randn(B * T * N_VIEWS, h, w, G * C, generator=g) for h, w in sizes]
    f = levels[0]
    f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = float('inf'), float('inf'), float('inf'), float('inf')
    levels = [f.to(BF16).to(DEV) for f in levels]
    loc = torch.rand(B * T * G, Q, P, 3, generator=g) * 0.4 + 0.3                                       # interior ...
    loc[:, ::3] = loc[:, ::3] * 4 - 1.5                                                                 # ... every third query: from far outside to the border
    loc[..., 2] = torch.randint(0, 6, (B * T * G, Q, P), generator=g).float() / 5
    w = torch.softmax(torch.randn(B * T * G, Q, P, L, generator=g), -1)
    params = torch.randn(B, Q, G * (C * C + POUT * T * P), generator=g) * 0.3
    args = (levels, B, T, G, loc.to(DEV), w.to(DEV), params.to(DEV), POUT)
    y = ops.sample_mix(*args)
    pairs = ops.sample_mix(*args, up_log2=9)
    dead = (y.reshape(B, Q, G, -1) == 0).all(-1)
    assert 0.01 < dead.float().mean() < 0.9 and not dead[:, 1::3].any() and not dead[:, 2::3].any()
    assert torch.equal((pairs.reshape(B, Q, G, -1) == 0).all(-1), dead)
    assert torch.isfinite(y).all() and torch.equal(pairs, dense.f16s_pairs(y, 9))


# ---- (d) pair format, independent of f16s_pairs ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('u', [9, 0])
@pytest.mark.parametrize('name', NAMES)
def test_pair_words_decode_to_the_fp32_result(name, u):
    inp = case_inputs(name)
    v = launch(inp).cpu() * 2.0 ** u                                                                    # exact
    hi, lo = decode_pairs(launch(inp, up_log2=u))
    assert float(v.max()) < 65504 and float(v.max()) > 2.0 ** u                                         # (a ReLU output: v >= 0)
    assert bool(torch.isfinite(hi).all())
    assert torch.equal(hi.view(torch.int16), v.half().view(torch.int16))                                # hi = RNE_fp16(v), signed zeros included
    err = (hi.double() + lo.double() - v.double()).abs()
    assert bool((err <= pair_bound(v.double())).all()), float((err / pair_bound(v.double())).max())


@gpu
def test_sample_mix_up_log2_argument_checks():
    from sparsebev_amd import ops
    inp = case_inputs('pin4_idle_waves')
    for bad in (9.0, True, '9'):
        with pytest.raises(RuntimeError):
            launch(inp, up_log2=bad)
    with pytest.raises(RuntimeError):
        launch(inp, up_log2=101)                                                                        # the C ABI's own range check
    with pytest.raises(RuntimeError):                                                                   # the fp32 path's checks are the pair path's
        ops.sample_mix([f.to(DEV) for f in inp['levels']], inp['B'], inp['T'], G, inp['loc'].to(DEV), inp['w'].to(DEV),
                       inp['params'].to(DEV)[..., :-1], POUT, up_log2=9)
