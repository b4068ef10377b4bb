"""Shapes, inputs and fp64 references of the exact-fp32 Linear family's forward sweep (tests/test_gpu_linear_fwd.py on the device,
tests/test_linear_fwd_host.py for what can be checked without one): sbev_linear_f32 on each of its six kernels, sbev_linear_splitk_f32
with a chosen `splits` on each of its four, the slab reducer sbev_splitk_reduce_f32, sbev_layer_norm_f32, sbev_ln_linear_f32,
sbev_linear_group_f32 and sbev_linear3_ln_relu(_ex)_f32 (csrc/gemm.hip, csrc/gemm_regtile.hip, csrc/small_ops.hpp).

Which kernel a case runs is not restated here: every list below sits under the name of the path it was chosen for, and the host test asks
the library (sbev_linear_f32_path, sbev_linear_splitk_path) whether the case takes it.

Every case has two kinds of input.  The INTEGER leg draws X and W from [-3, 3] and the bias and the residual from [-8, 8]: every partial
sum in any order is an integer of at most 9 K + 16 < 2^24, so the kernel must be BIT-EQUAL to the reference through every tile shape,
split plan, fold and slab sum.  LayerNorm outputs are no integers: where a call has a LayerNorm the integer leg runs the same call
without it.  The REAL leg draws X ~ randn, W ~ randn / sqrt(K), bias and residual ~ randn and is held to the project's own measure,
max |err| / max |ref| against fp64:

    TOL    = 2e-5   a Linear                    (backward_rows_cases.TOL, test_gpu_dense.py::test_linear_shapes)
    TOL_LN = 1e-4   where a LayerNorm follows   (test_splitk_register_tiled_kernel_ragged, test_layer_norm_as_linear_prologue)

Measured worst on an MI355X, per path (MEASURED_WORST below has every line the device tests print, next to its bound):
    held to 2e-5: sbev_linear_f32 strip 9.5e-7, ragged 64 x 64 5.2e-7, 128 x 128 7.0e-7, small 256 / 512 2.3e-7 / 2.8e-7, 64 x 64 1.3e-6;
                  sbev_linear_splitk_f32 register tiles fold 1 / 2 2.3e-6 / 1.2e-6, 128 x 128 split-K 1.9e-6, ragged 1.4e-6;
                  sbev_splitk_reduce_f32 1.2e-7; sbev_linear_group_f32 2.6e-7; `pre` of sbev_linear3_ln_relu_ex_f32 9.5e-8
    held to 1e-4: the split-K paths + LayerNorm 3.2e-6; the reducer + LayerNorm 2.1e-7; sbev_layer_norm_f32 (mean 100) 3.1e-6;
                  sbev_ln_linear_f32 Xn 1.5e-7, Y 3.0e-7; sbev_linear3_ln_relu(_ex)_f32 1.8e-7

Everything here is torch on the CPU; the references are plain fp64 restatements of the contracts in include/sbev_hip.h."""
import collections
import functools
import zlib

import torch

TOL = 2e-5
TOL_LN = 1e-4
EXACT_LIMIT = 2 ** 24           # integers below it are exact in fp32
EPS = 1e-5                      # LayerNorm epsilon
MIN_LN_VARIANCE = 1e-3          # no LayerNorm row of a real leg has less: rstd never amplifies fp32 noise past the bound

# the values of enum sbev_linear_path / sbev_linear_splitk_path_id (include/sbev_hip.h), by position
LINEAR_PATHS = ['STRIP', 'RAGGED64', 'BIG128', 'SMALL256', 'SMALL512', 'TILE64']
SPLITK_PATHS = ['REGTILE_FOLD2', 'REGTILE_FOLD1', 'SPLIT128', 'SPLIT128_RAGGED']

# worst real-leg max |err| / max |ref| per path as printed by tests/test_gpu_linear_fwd.py on an MI355X  (bound it is held to)
MEASURED_WORST = {
    'sbev_linear_f32 STRIP': (9.54e-07, TOL),
    'sbev_linear_f32 RAGGED64': (5.22e-07, TOL),
    'sbev_linear_f32 BIG128': (7.03e-07, TOL),
    'sbev_linear_f32 SMALL256': (2.34e-07, TOL),
    'sbev_linear_f32 SMALL512': (2.83e-07, TOL),
    'sbev_linear_f32 TILE64': (1.28e-06, TOL),
    'sbev_linear_f32 strip leavers': (7.72e-07, TOL),
    'sbev_linear_splitk_f32 REGTILE_FOLD1': (2.25e-06, TOL),
    'sbev_linear_splitk_f32 REGTILE_FOLD1 + LayerNorm': (2.25e-06, TOL_LN),
    'sbev_linear_splitk_f32 REGTILE_FOLD2': (1.24e-06, TOL),
    'sbev_linear_splitk_f32 REGTILE_FOLD2 + LayerNorm': (5.23e-07, TOL_LN),
    'sbev_linear_splitk_f32 SPLIT128': (1.91e-06, TOL),
    'sbev_linear_splitk_f32 SPLIT128 + LayerNorm': (3.19e-06, TOL_LN),
    'sbev_linear_splitk_f32 SPLIT128_RAGGED': (1.40e-06, TOL),
    'sbev_linear_splitk_f32 SPLIT128_RAGGED + LayerNorm': (1.90e-06, TOL_LN),
    'sbev_splitk_reduce_f32': (1.17e-07, TOL),
    'sbev_splitk_reduce_f32 + LayerNorm': (2.09e-07, TOL_LN),
    'sbev_layer_norm_f32': (3.12e-06, TOL_LN),
    'sbev_ln_linear_f32 one launch, Xn': (1.34e-07, TOL_LN),
    'sbev_ln_linear_f32 one launch, Y': (2.67e-07, TOL_LN),
    'sbev_ln_linear_f32 two launches, Xn': (1.46e-07, TOL_LN),
    'sbev_ln_linear_f32 two launches, Y': (3.02e-07, TOL_LN),
    'sbev_linear_group_f32 K=256': (1.47e-07, TOL),
    'sbev_linear_group_f32 K=512': (2.60e-07, TOL),
    'sbev_linear3_ln_relu(_ex)_f32 y': (1.82e-07, TOL_LN),
    'sbev_linear3_ln_relu_ex_f32 pre': (9.53e-08, TOL),
}


# ---- measures and generators --------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """the project's measure: max |got - ref| / max |ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if ref.numel() == 0:
        return 0.0
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))     # the same stream in every process


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def assert_exact(bound, what):
    """the integer leg's premise: `bound` >= the sum of the absolute values of everything one output adds up, so every partial sum in
    every order is an integer of at most that size"""
    assert bound < EXACT_LIMIT, '%s: integer sums up to %d are not exact in fp32' % (what, bound)


def int_bound(K):
    """|x|, |w| <= 3, |bias|, |residual| <= 8"""
    return 9 * K + 16


@functools.lru_cache(maxsize=6)
def rows(M, K, leg):
    """X [M, K] -- read-only"""
    g = _gen('x', M, K, leg)
    if leg == 'int':
        assert_exact(int_bound(K), 'K=%d' % K)
        return _ints(g, -3, 3, M, K)
    return torch.randn(M, K, generator=g)


@functools.lru_cache(maxsize=6)
def weights(N, K, leg):
    """W [N, K] -- read-only"""
    g = _gen('w', N, K, leg)
    return _ints(g, -3, 3, N, K) if leg == 'int' else torch.randn(N, K, generator=g) * K ** -0.5


@functools.lru_cache(maxsize=16)
def vector(N, leg, tag='bias'):
    """bias [N] -- read-only"""
    g = _gen(tag, N, leg)
    return _ints(g, -8, 8, N) if leg == 'int' else torch.randn(N, generator=g)


@functools.lru_cache(maxsize=6)
def matrix(M, N, leg, tag='res'):
    """residual / add_after [M, N] -- read-only"""
    g = _gen(tag, M, N, leg)
    return _ints(g, -8, 8, M, N) if leg == 'int' else torch.randn(M, N, generator=g)


@functools.lru_cache(maxsize=16)
def ln_params(N):
    """(gamma in [0.5, 1.5], beta ~ 0.2 randn) -- read-only"""
    g = _gen('ln', N)
    return torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2


@functools.lru_cache(maxsize=4)
def product(M, N, K, leg):
    """X W^T in fp64 -- read-only, shared by every case of the shape"""
    return rows(M, K, leg).double() @ weights(N, K, leg).double().t()


# ---- fp64 references: the header's contracts ------------------------------------------------------------------------------------------------
def _ln(v, gamma, beta, eps=EPS):
    mean = v.mean(-1, keepdim=True)
    var = (v - mean).pow(2).mean(-1, keepdim=True)
    return (v - mean) * (var + eps).rsqrt() * gamma.double() + beta.double()


def row_variance(v):
    v = v.double()
    return (v - v.mean(-1, keepdim=True)).pow(2).mean(-1)


def linear_ref(X, W, b=None, res=None, relu=False, xw=None):
    """sbev_linear_f32: act(X W^T + b) + res"""
    y = X.double() @ W.double().t() if xw is None else xw.clone()
    if b is not None:
        y = y + b.double()
    if relu:
        y = y.clamp_min(0.0)
    if res is not None:
        y = y + res.double()
    return y


def splitk_pre_ln(X, W, b=None, res=None, relu=False, xw=None):
    """what sbev_linear_splitk_f32 normalises: relu?(X W^T + b) + res"""
    return linear_ref(X, W, b, res, relu, xw)


def splitk_ref(X, W, b=None, res=None, ln=None, relu=False, xw=None):
    """sbev_linear_splitk_f32: LN?(relu?(X W^T + b) + res) -- the ReLU is the Linear's activation, before the residual, LayerNorm or not"""
    y = splitk_pre_ln(X, W, b, res, relu, xw)
    return _ln(y, ln[0], ln[1]) if ln is not None else y


def reduce_ref(slabs, b=None, res=None, ln=None, relu=False):
    """sbev_splitk_reduce_f32: LN?(relu?(sum_z slabs[z] + b) + res), slabs [splits, M, N]"""
    y = slabs.double().sum(0)
    if b is not None:
        y = y + b.double()
    if relu:
        y = y.clamp_min(0.0)
    if res is not None:
        y = y + res.double()
    return _ln(y, ln[0], ln[1]) if ln is not None else y


def layer_norm_ref(x, gamma, beta, relu=False, add_after=None):
    """sbev_layer_norm_f32: relu?(LN(x)) + add_after -- here the ReLU is the LayerNorm's"""
    y = _ln(x.double(), gamma, beta)
    if relu:
        y = y.clamp_min(0.0)
    if add_after is not None:
        y = y + add_after.double()
    return y


def ln_linear_ref(X, gamma, beta, ln_relu, ln_add, W, b=None, res=None, relu=False):
    """sbev_ln_linear_f32: Xn = relu?(LN(X)) + ln_add;  Y = act(Xn W^T + b) + res.  Returns (Xn, Y)."""
    xn = layer_norm_ref(X, gamma, beta, ln_relu, ln_add)
    return xn, linear_ref(xn, W, b, res, relu)


def lin3_ref(x, w, b, gamma, beta):
    """sbev_linear3_ln_relu(_ex)_f32: pre = x[:, 0:3] w^T + b;  y = relu(LN(pre)).  Returns (y, pre)."""
    pre = x[:, :3].double() @ w.double().t() + b.double()
    return _ln(pre, gamma, beta).clamp_min(0.0), pre


# ---- case lists ---------------------------------------------------------------------------------------------------------------------------
def _unique(seq):
    seen, out = set(), []
    for p in seq:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def cross_edges(As, Bs, two_b, two_a):
    """every a with the two b of `two_b` and every b with the two a of `two_a`, not the full product"""
    return _unique([(a, b) for b in two_b for a in As] + [(a, b) for a in two_a for b in Bs])


# The sweeps pair every M with two N of at least 5 and every N with two M of at least 33, so the smallest output has 5 elements: the
# real leg's measure divides by max |ref|, which stands for the size of the terms an output sums only while SOME output is that large.
# A 1 x 1 output is a single draw of x.w + b and can cancel to a few per cent of its terms (K = 260: -0.022 from terms of order 1), where
# the fp32 round-off of a correct K-step chain (about sqrt(K) 2^-25 of the terms) reads as 2e-5 of the result.  MIN_REAL_REF holds the
# lists to it (tests/test_linear_fwd_host.py).
MIN_REAL_REF = 0.5


def r4(k):
    return (k + 3) // 4 * 4


# path: the kernel the case was chosen for;  res: None, 'aligned' or 'offset' (residual base one float past a 16-byte boundary);
# yoff: floats between a 16-byte boundary and Y;  bias: present or NULL
LinCase = collections.namedtuple('LinCase', 'path M N K ldx ldw ldy yoff relu res bias')
EPILOGUES = [(relu, res) for relu in (0, 1) for res in (None, 'aligned', 'offset')]       # the relu x residual sub-grid, cycled over a path's shapes
LAYOUTS = [(pad, yoff) for pad in (0, 1, 3, 4) for yoff in (0, 1)]                        # (ldy - N, Y offset): both epilogues of a kernel


def _lin(path, M, N, K, i=0, dk=0, **kw):
    relu, res = EPILOGUES[i % len(EPILOGUES)]
    d = dict(path=path, M=M, N=N, K=K, ldx=r4(K) + dk, ldw=r4(K) + dk, ldy=N, yoff=0, relu=relu, res=res, bias=(i % 5 != 4))
    d.update(kw)
    return LinCase(**d)


def _layouts(path, M, N, K):
    """ldy in {N, N + 1, N + 3, N + 4} x Y offset by 0 / 1 float, with an aligned residual: vector and scalar epilogue"""
    return [_lin(path, M, N, K, ldy=N + pad, yoff=yoff, relu=i % 2, res='aligned', bias=True) for i, (pad, yoff) in enumerate(LAYOUTS)]


SMALL_M, SMALL_N = [1, 31, 32, 33, 65], [1, 3, 4, 5, 31, 32, 33, 36, 776]            # 32 x 32 tiles; float4 epilogue slots full / partial
TILE_M, TILE_N = [1, 63, 64, 65, 129], [1, 5, 63, 64, 65, 130]                        # 64 x 64 tiles
TILE_K = [32, 64, 96, 1024]                                                             # one, two, three K steps of the double buffer; a long K
RAGGED_K = [1, 3, 5, 31, 33, 37, 100, 260]                                              # K % 32 != 0 with K % 4 != 0 and == 0, below and above one K step
BIG_SHAPES = [(1, 32768 + 5), (129, 16384 + 2), (257, 11008 + 3), (4100, 1100)]         # >= 256 tiles of 128 x 128: one row and a ragged last column tile;
#                                                                                         2 x 129; 3 x 87 = 261 tiles (no multiple of 8); 33 x 9 with tiles_n < tiles_m
STRIP_M, STRIP_N = [1, 15, 16, 17, 31, 32, 33, 49], [24576, 24704]                      # 16-row fragments alternating between two waves; N / 128 = 192, 193
NOT_STRIP_N = 24448                                                                     # N / 128 = 191: one below the strip kernel's threshold


@functools.lru_cache(maxsize=None)
def linear_cases(path):
    """the cases of one path of sbev_linear_f32"""
    out = []
    if path in ('SMALL256', 'SMALL512'):
        K = 256 if path == 'SMALL256' else 512
        shapes = cross_edges(SMALL_M, SMALL_N, two_b=(5, 776), two_a=(33, 65))
        out += [_lin(path, M, N, K, i, dk=4 * (i % 2)) for i, (M, N) in enumerate(shapes)]
        out += _layouts(path, 33, 36, K)
    elif path == 'TILE64':
        shapes = cross_edges(TILE_M, TILE_N, two_b=(5, 130), two_a=(65, 129))
        for K in TILE_K:
            out += [_lin(path, M, N, K, i + K // 32, dk=4 * (i % 2)) for i, (M, N) in enumerate(shapes)]
        out += _layouts(path, 65, 130, 96)
    elif path == 'RAGGED64':
        shapes = cross_edges(TILE_M, TILE_N, two_b=(5, 130), two_a=(65, 129))
        for K in RAGGED_K:                       # ldx = ldw = K rounded up to 4, and the same plus 4
            out += [_lin(path, M, N, K, i + K, dk=4 * (i % 2)) for i, (M, N) in enumerate(shapes)]
        out += _layouts(path, 65, 130, 37)
    elif path == 'BIG128':
        for i, (M, N) in enumerate(BIG_SHAPES):
            out += [_lin(path, M, N, 32, 2 * i, dk=4 * (i % 2)), _lin(path, M, N, 64, 2 * i + 1)]
        out += [_lin(path, 257, 11008 + 3, 256, relu=1, res='aligned'), _lin(path, 129, 16384 + 2, 512, relu=0, res=None)]
        out += _layouts(path, 257, 11008 + 3, 32)
    elif path == 'STRIP':                        # K = 256, no residual, ldy % 4 == 0, aligned
        shapes = cross_edges(STRIP_M, STRIP_N, two_b=tuple(STRIP_N), two_a=(1, 17))
        for i, (M, N) in enumerate(shapes):
            out.append(_lin(path, M, N, 256, relu=i % 2, res=None, bias=(i // 2) % 2 == 0, ldy=N + 4 * ((i // 4) % 2), ldx=256 + 4 * ((i // 8) % 2)))
        out += [_lin(path, 33, 24576, 256, relu=r, res=None, bias=bool(b), ldy=24576 + ly, ldx=256 + lx)
                for r in (0, 1) for b in (0, 1) for ly in (0, 4) for lx in (0, 4)]
    else:
        raise KeyError(path)
    return out


@functools.lru_cache(maxsize=None)
def strip_leavers():
    """the strip kernel's shapes with what it does not take -- a residual, ldy = N + 1, Y offset by one float -- and N = 24448, one tile
    short of it: (case, where the library must send it).  Fewer than 256 tiles of 128 x 128 go to the small-tile kernel, more to the
    128 x 128 one."""
    out = []
    for M, path in ((17, 'SMALL256'), (129, 'BIG128')):
        N = 24576
        out += [_lin(path, M, N, 256, relu=1, res='aligned', bias=True),
                _lin(path, M, N, 256, relu=0, res=None, bias=True, ldy=N + 1),
                _lin(path, M, N, 256, relu=1, res=None, bias=False, yoff=1)]
    out += [_lin('SMALL256', 17, NOT_STRIP_N, 256, relu=1, res=None, bias=True),           # 191 tiles
            _lin('BIG128', 129, NOT_STRIP_N, 256, relu=0, res=None, bias=True)]            # 2 x 191 tiles
    return out


# sbev_linear_splitk_f32 with `splits` given.  bias / relu / res / ln: the reducer's epilogue
SplitCase = collections.namedtuple('SplitCase', 'path M N K splits ldx ldw bias relu res ln')
EPILOGUE_GRID = [(b, r, s, l) for b in (0, 1) for r in (0, 1) for s in (0, 1) for l in (0, 1)]     # bias x relu x residual x LayerNorm

REG_M, REG_N, REG_K = [1, 47, 48, 49, 97], [128, 384], [2048, 2080, 4096]             # 48-row wave tasks; K / 32 = 64, 65 (odd), 128
S128_M, S128_N, S128_K = [1, 127, 128, 129], [4, 132, 1020], [64, 96, 1024, 2080]
S128_SPLITS = [1, 2, 3, 4, 5]
SRAG_K = [36, 100, 2050]


def reg_splits(K):
    return [1, 2, 3, 7, 8, K // 32]           # fold == 1 (odd), fold == 2 (even), one K step per split


def _keep_ln_rows_apart(N, relu, res, ln):
    """a ReLU'd row of 4 or 8 columns is all zeros once in 16 or 256 rows, and a LayerNorm of a constant row measures nothing: where the
    cycled epilogue puts ReLU + LayerNorm on so narrow a row without a residual, it gets the residual (the full grids run at N >= 132)"""
    return 1 if (ln and relu and not res and N <= 8) else res


def _split(path, M, N, K, splits, i=0, **kw):
    b, r, s, l = EPILOGUE_GRID[(5 * i + 3) % 16]
    d = dict(path=path, M=M, N=N, K=K, splits=splits, ldx=r4(K) + 4 * (i % 2), ldw=r4(K) + 4 * ((i // 2) % 2), bias=b, relu=r, res=s, ln=l)
    d.update(kw)
    d['res'] = _keep_ln_rows_apart(d['N'], d['relu'], d['res'], d['ln'])
    return SplitCase(**d)


def _fold_path(splits):
    return 'REGTILE_FOLD2' if splits % 2 == 0 else 'REGTILE_FOLD1'


@functools.lru_cache(maxsize=None)
def splitk_cases(kernel):
    """kernel: 'REGTILE' (both folds), 'SPLIT128' or 'SPLIT128_RAGGED'"""
    out = []
    if kernel == 'REGTILE':
        i = 0
        for K in REG_K:
            for N in REG_N:
                for M, s in cross_edges(REG_M, reg_splits(K), two_b=(3, 8), two_a=(1, 49)):
                    out.append(_split(_fold_path(s), M, N, K, s, i))
                    i += 1
        # (1, 128, 3) and (49, 128, 3): 3 and 6 wave tasks, no multiple of 4 -- a spare wave repeats the last task
        out += [_split('REGTILE_FOLD1', M, 128, 2048, 3, j) for j, M in enumerate((1, 49))]
        out += [_split('REGTILE_FOLD2', 1, 128, 2048, 6, 0)]                               # 6 tasks: a spare PAIR of waves under fold == 2
        for fold_splits in (3, 8):                                                         # the epilogue grid on one shape per fold
            out += [_split(_fold_path(fold_splits), 49, 384, 2080, fold_splits, bias=b, relu=r, res=s, ln=l) for b, r, s, l in EPILOGUE_GRID]
    elif kernel == 'SPLIT128':
        i = 0
        for K in S128_K:
            for N in S128_N:
                for M, s in cross_edges(S128_M, S128_SPLITS, two_b=(1, 3), two_a=(1, 129)):
                    out.append(_split('SPLIT128', M, N, K, s, i))
                    i += 1
        out += [_split('SPLIT128', M, 132, 96, 4, j) for j, M in enumerate((1, 129))]      # fewer slabs written than asked for (3 K steps)
        out += [_split('SPLIT128', M, 128, 2048, 65, j) for j, M in enumerate((1, 129))]   # splits > K / 32 leaves the register-tiled kernel
        out += [_split('SPLIT128', 129, 132, 2080, 3, bias=b, relu=r, res=s, ln=l) for b, r, s, l in EPILOGUE_GRID]
    elif kernel == 'SPLIT128_RAGGED':
        i = 0
        for K in SRAG_K:
            for N in (4, 132):
                for M in (1, 129):
                    for s in (1, 3):
                        out.append(_split('SPLIT128_RAGGED', M, N, K, s, i))
                        i += 1
        out += [_split('SPLIT128_RAGGED', 129, 132, 100, 3, bias=b, relu=r, res=s, ln=l) for b, r, s, l in EPILOGUE_GRID]
    else:
        raise KeyError(kernel)
    return out


def _ceil_div(a, b):
    return (a + b - 1) // b


def expected_slabs_split128(K, splits):
    """slabs the 128 x 128 split-K tiles write, from the header: ceil(K / (32 ceil(K / splits / 32)))"""
    kps = _ceil_div(_ceil_div(K, splits), 32) * 32
    return _ceil_div(K, kps)


# sbev_splitk_reduce_f32 / sbev_layer_norm_f32: one wave per row, 4 rows per block, 1 .. 4 float4 slots per lane (the last one full / partial)
RED_M = [1, 3, 4, 5, 9]
RED_N = [4, 8, 252, 256, 260, 512, 1020, 1024]
RED_SPLITS = [1, 2, 5]
ReduceCase = collections.namedtuple('ReduceCase', 'M N splits bias relu res ln')


@functools.lru_cache(maxsize=None)
def reduce_cases():
    out = []
    for i, (M, N) in enumerate((M, N) for M in RED_M for N in RED_N):
        for j, s in enumerate(RED_SPLITS):
            b, r, rs, l = EPILOGUE_GRID[(7 * i + 5 * j) % 16]
            out.append(ReduceCase(M, N, s, b, r, _keep_ln_rows_apart(N, r, rs, l), l))
    out += [ReduceCase(5, 260, 5, b, r, rs, l) for b, r, rs, l in EPILOGUE_GRID]
    return out


@functools.lru_cache(maxsize=8)
def slabs(M, N, splits, leg):
    """[splits, M, N] -- read-only.  Integer leg: |slab| <= 1000, so sums stay below 5016"""
    g = _gen('slabs', M, N, splits, leg)
    if leg == 'int':
        assert_exact(1000 * splits + 16, 'slabs')
        return _ints(g, -1000, 1000, splits, M, N)
    return torch.randn(splits, M, N, generator=g)


def layer_norm_shapes():
    return [(M, N) for M in RED_M for N in RED_N]


@functools.lru_cache(maxsize=8)
def ln_rows(M, N):
    """rows with a large mean (3 randn + 100): a one-pass variance E[x^2] - E[x]^2 in fp32 would miss the bound by orders of magnitude"""
    return torch.randn(M, N, generator=_gen('ln_rows', M, N)) * 3 + 100


# sbev_ln_linear_f32: X, Xn [M, K] dense
LnLinCase = collections.namedtuple('LnLinCase', 'M N K ldw ldy ln_relu ln_add relu res')
LNL_M, LNL_N = [1, 31, 32, 33, 2048, 2049], [1, 33, 776]
LN_FUSE_MAX_ROWS = 2048                                       # the header: one launch when K == 256, M <= 2048 and the small-tile kernel takes the shape


@functools.lru_cache(maxsize=None)
def ln_linear_cases():
    out = []
    for i, (M, N) in enumerate((M, N) for M in LNL_M for N in LNL_N):
        a, b, c, d = EPILOGUE_GRID[(5 * i + 1) % 16]
        out.append(LnLinCase(M, N, 256, 256 + 4 * (i % 2), N + (i % 3), a, b, c, d))
    out += [LnLinCase(33, 33, 256, 256, 33, a, b, c, d) for a, b, c, d in EPILOGUE_GRID]
    out += [LnLinCase(33, 33, 512, 512, 36, 1, 1, 1, 1), LnLinCase(33, 33, 100, 104, 33, 1, 0, 0, 1)]       # other K: always two launches
    return out


# sbev_linear_group_f32: three problems of different M, N and leading dimensions in one launch
GROUPS = {256: [_lin('SMALL256', 33, 10, 256, 1, ldx=260, ldw=256, ldy=11, yoff=1),
                _lin('SMALL256', 1, 776, 256, 3, ldx=256, ldw=264, ldy=776),
                _lin('SMALL256', 65, 33, 256, 2, ldx=256, ldw=256, ldy=36)],
          512: [_lin('SMALL512', 31, 5, 512, 0, ldx=512, ldw=516, ldy=5),
                _lin('SMALL512', 64, 36, 512, 4, ldx=516, ldw=512, ldy=40),
                _lin('SMALL512', 3, 130, 512, 5, ldx=512, ldw=512, ldy=133, yoff=1)]}

# sbev_linear3_ln_relu(_ex)_f32
LIN3_M, LIN3_N, LIN3_LDX = [1, 3, 4, 5, 900], [4, 252, 256, 260, 1024], [4, 10]


@functools.lru_cache(maxsize=8)
def lin3_case(M, N, leg):
    """(x [M, 3], w [N, 3], b [N]) -- read-only.  Integer leg: the pre-LayerNorm rows are integers of at most 27 + 8"""
    g = _gen('lin3', M, N, leg)
    if leg == 'int':
        assert_exact(3 * 9 + 8, 'lin3')
        return _ints(g, -3, 3, M, 3), _ints(g, -3, 3, N, 3), _ints(g, -8, 8, N)
    return torch.randn(M, 3, generator=g), torch.randn(N, 3, generator=g) * 3 ** -0.5, torch.randn(N, generator=g)


# ---- a case's operands and reference ------------------------------------------------------------------------------------------------------
def linear_operands(c, leg):
    """(X, W, bias or None, residual or None, fp64 reference) of a LinCase"""
    X, W = rows(c.M, c.K, leg), weights(c.N, c.K, leg)
    b = vector(c.N, leg) if c.bias else None
    res = matrix(c.M, c.N, leg) if c.res else None
    return X, W, b, res, linear_ref(X, W, b, res, c.relu, xw=product(c.M, c.N, c.K, leg))


def splitk_operands(c, leg, with_ln):
    """(X, W, bias, residual, ln or None, fp64 reference) of a SplitCase; with_ln = False drops the LayerNorm (the integer leg)"""
    X, W = rows(c.M, c.K, leg), weights(c.N, c.K, leg)
    b = vector(c.N, leg) if c.bias else None
    res = matrix(c.M, c.N, leg) if c.res else None
    ln = ln_params(c.N) if (c.ln and with_ln) else None
    return X, W, b, res, ln, splitk_ref(X, W, b, res, ln, c.relu, xw=product(c.M, c.N, c.K, leg))


def reduce_operands(c, leg, with_ln):
    S = slabs(c.M, c.N, c.splits, leg)
    b = vector(c.N, leg) if c.bias else None
    res = matrix(c.M, c.N, leg) if c.res else None
    ln = ln_params(c.N) if (c.ln and with_ln) else None
    return S, b, res, ln, reduce_ref(S, b, res, ln, c.relu)
