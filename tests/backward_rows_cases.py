"""Shapes, inputs and fp64 references of the row-wise backward sweep (tests/test_gpu_backward_rows.py on the device,
tests/test_backward_rows_host.py for what can be checked without one): the bias / ReLU column sums, the LayerNorm backward, the two
grouped parameter-gradient launches (csrc/backward_ops.hip) and the multi-segment weight-gradient GEMM (csrc/gemm_any.hip).

Every reduction has two kinds of input.  The INTEGER leg draws small integers, so that every partial sum in any order is an integer below
2^24 and therefore exact in fp32: the kernel must be bit-equal to the reference whatever its summation order, split plan or layout -- a
dropped or doubled row, k-step or segment cannot hide in a tolerance.  The REAL leg draws randn and is compared with fp64 by the project's
measure for these functions (test_gpu_backward.py::test_linear_function_vs_torch): max |err| / max |ref| < TOL.

Everything here is torch on the CPU; the references are plain fp64 restatements of the kernels' contracts (include/sbev_hip.h)."""
import functools
import zlib

import torch

TOL = 2e-5                      # max |err| / max |ref| of a parameter gradient (test_linear_function_vs_torch, test_layer_norm_function_vs_torch)
EXACT_LIMIT = 2 ** 24           # integers below it are exact in fp32
EPS = 1e-5                      # LayerNorm epsilon
NEAR_ZERO = 1e-4                # relu LayerNorm: dY = 0 where the fp64 pre-activation is this close to 0 (fp32 may see the other sign)
MAX_ZEROED_SHARE = 1e-3

# ---- shapes: the smallest row counts that reach every loop ---------------------------------------------------------------------------
BIAS_M_ONE_PASS = [1, 15, 16, 17, 48, 49, 63, 64, 65, 900, 2047, 2048]      # 16 row lanes, 64-row trips (m + 48 < M), <= ONE_PASS_ROWS
BIAS_M_TWO_PASS = [2049, 2080, 2081, 3600]                                  # 32-row chunks: one row into a new chunk, a full one, 3600 = 112.5
BIAS_M = BIAS_M_ONE_PASS + BIAS_M_TWO_PASS
BIAS_N = [1, 3, 10, 63, 64, 65, 256, 776]                                   # 64-column blocks: partial, full, one over, several + a partial one
LN_M = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 900, 2047, 2048, 2049, 2081, 3600]    # 4 rows per block; 16 lanes x 2 rows per trip; chunks
LN_N = [4, 8, 252, 256, 260, 512, 1020, 1024]                               # 1 .. 4 float4 slots per lane, the last one full / partial
COLSUM_GROUP_M = [1, 16, 17, 112, 113, 127, 128, 129, 240, 241, 900, 2049]  # 128-row trips (m + 112 < M): zero, one, two trips and tails
LN_GROUP_M = [1, 16, 17, 48, 49, 64, 65, 900, 2049]                         # 64-row trips (m + 48 < M)
GEMM_MULTI_SHAPES = [(256, 256, 900),       # (M, N, K): the shared-Linear weight gradient
                     (130, 129, 33),        # ragged tiles, one ragged K step
                     (10, 256, 37),         # element-wise staging: ld % 4 != 0
                     (1, 5, 7),
                     (256, 256, 64),        # K / 64 = 1: one split per segment
                     (256, 512, 2049)]      # 8 tiles, several splits per segment, a one-row last K step
GEMM_NSEGS = [1, 2, 3, 8]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (a_kmajor, b_kmajor)

# one sbev_colsum_group launch: 16 biases of different widths (no multiple of 64 among most: blk0 differs from 64-column strides)
COLSUM_WIDTHS = [1, 3, 10, 63, 64, 65, 256, 776, 2, 5, 17, 100, 127, 128, 129, 300]
COLSUM_NSEGS = [8, 7, 6, 5, 4, 3, 2, 1, 8, 7, 6, 5, 4, 3, 2, 1]
COLSUM_ACC = [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0]
# one sbev_layer_norm_param_group launch: 8 LayerNorms
LN_GROUP_WIDTHS = [256, 512, 260, 64, 4, 1024, 252, 8]
LN_GROUP_NSEGS = [3, 2, 4, 8, 7, 1, 5, 6]
LN_GROUP_RELU = [1, 0, 1, 0, 1, 1, 0, 0]
LN_GROUP_ACC = [0, 1, 1, 0, 1, 0, 0, 1]


def _unique(pairs):
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def bias_shapes():
    """every M at N in {10, 256}, every N at M in {17, 2049}"""
    return _unique([(M, N) for N in (10, 256) for M in BIAS_M] + [(M, N) for M in (17, 2049) for N in BIAS_N])


def ln_shapes():
    """every M at N = 256, every N at M in {5, 33, 2049}"""
    return _unique([(M, 256) for M in LN_M] + [(M, N) for M in (5, 33, 2049) for N in LN_N])


# ---- measures ------------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """the project's measure of a gradient: max |got - ref| / max |ref|"""
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


SPECIAL_Y = [0.0, -0.0, 1e-40, -1e-40]       # 1e-40 is a denormal in fp32


# ---- bias / ReLU column sums -----------------------------------------------------------------------------------------------------------
def relu_output_like(g, M, N):
    """a ReLU's forward output as the mask sees it: about half zeros, and exact +0, -0, a positive and a negative denormal spread over the
    rows -- zero does not pass the gradient (Y > 0 is false for both signs), a positive denormal does"""
    Y = torch.randn(M, N, generator=g).clamp_min(0.0)
    flat = Y.view(-1)
    for i, s in enumerate(SPECIAL_Y):
        flat[i::7] = s
    return Y


def bias_relu_ref(dY, Y=None, db_before=None):
    """dZ = dY * (Y > 0);  db = sum_m dZ (+ db_before).  fp64."""
    dZ = dY.double()
    if Y is not None:
        dZ = torch.where(Y > 0, dZ, torch.zeros_like(dZ))
    db = dZ.sum(0)
    if db_before is not None:
        db = db + db_before.double()
    return dZ, db


@functools.lru_cache(maxsize=8)
def bias_case(M, N, leg, with_y):
    """(dY [M, N], Y [M, N] or None, db_before [N]) -- read-only"""
    g = _gen('bias', M, N, leg, with_y)
    if leg == 'int':
        dY, db0 = _ints(g, -3, 3, M, N), _ints(g, -3, 3, N)
        assert_exact(3 * M + 3, 'bias M=%d' % M)
    else:
        dY, db0 = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    Y = relu_output_like(g, M, N) if with_y else None
    return dY, Y, db0


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------------
def layer_norm_ref(dY, X, gamma, beta, relu, dgamma_before=None, dbeta_before=None, eps=EPS):
    """fp64: xhat = (x - mean) rstd;  g = dY (xhat gamma + beta > 0) if relu else dY;
    dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat));  dgamma = sum_m g xhat;  dbeta = sum_m g.
    Returns dict(dX, dgamma, dbeta, mean, rstd, pre)."""
    dY, X, gamma = dY.double(), X.double(), gamma.double()
    mean = X.mean(1, keepdim=True)
    rstd = ((X - mean).pow(2).mean(1, keepdim=True) + eps).rsqrt()
    xhat = (X - mean) * rstd
    pre = xhat * gamma + (beta.double() if beta is not None else 0.0)
    g = torch.where(pre > 0, dY, torch.zeros_like(dY)) if relu else dY
    gg = g * gamma
    dX = rstd * (gg - gg.mean(1, keepdim=True) - xhat * (gg * xhat).mean(1, keepdim=True))
    dgamma, dbeta = (g * xhat).sum(0), g.sum(0)
    if dgamma_before is not None:
        dgamma = dgamma + dgamma_before.double()
    if dbeta_before is not None:
        dbeta = dbeta + dbeta_before.double()
    return dict(dX=dX, dgamma=dgamma, dbeta=dbeta, mean=mean[:, 0], rstd=rstd[:, 0], pre=pre)


def _ln_inputs(g, M, N, gamma, beta, relu):
    """(dY, X, zeroed share): with relu, dY = 0 wherever the fp64 pre-activation lies within NEAR_ZERO of 0, so that the sign fp32 sees
    there cannot matter; no element is left out of any comparison"""
    X = torch.randn(M, N, generator=g) * 2 + 0.3
    dY = torch.randn(M, N, generator=g)
    share = 0.0
    if relu:
        near = layer_norm_ref(dY, X, gamma, beta, True)['pre'].abs() < NEAR_ZERO
        dY[near] = 0.0
        share = near.double().mean().item() if near.numel() else 0.0
    return dY, X, share


def _ln_params(g, N):
    """gamma in [0.5, 1.5] (the density of xhat gamma + beta near 0 is then at most 0.4 / 0.5 = 0.8: a share of about 1.6e-4 within
    NEAR_ZERO), beta ~ 0.2 randn, and the buffers an accumulating call adds to"""
    return (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2, torch.randn(N, generator=g), torch.randn(N, generator=g))


@functools.lru_cache(maxsize=8)
def ln_case(M, N, relu):
    """dict(dY, X, gamma, beta, dgamma_before, dbeta_before, share) -- read-only"""
    g = _gen('ln', M, N, relu)
    gamma, beta, dg0, db0 = _ln_params(g, N)
    dY, X, share = _ln_inputs(g, M, N, gamma, beta, relu)
    return dict(dY=dY, X=X, gamma=gamma, beta=beta, dgamma_before=dg0, dbeta_before=db0, share=share)


# ---- grouped launches ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def colsum_group_case(M, leg, widths=tuple(COLSUM_WIDTHS), nsegs=tuple(COLSUM_NSEGS)):
    """list over groups of (segments [nseg][M, N], out_before [N]) -- read-only"""
    g = _gen('colsum_group', M, leg, widths, nsegs)
    groups = []
    for N, ns in zip(widths, nsegs):
        if leg == 'int':
            segs, out0 = [_ints(g, -3, 3, M, N) for _ in range(ns)], _ints(g, -3, 3, N)
            assert_exact(3 * M * ns + 3, 'colsum_group M=%d nseg=%d' % (M, ns))
        else:
            segs, out0 = [torch.randn(M, N, generator=g) for _ in range(ns)], torch.randn(N, generator=g)
        groups.append((segs, out0))
    return groups


def colsum_group_ref(segs, out_before=None):
    s = sum(t.double().sum(0) for t in segs)
    return s + out_before.double() if out_before is not None else s


@functools.lru_cache(maxsize=1)
def ln_group_case(M):
    """list over the 8 LayerNorms of dict(gamma, beta, dgamma_before, dbeta_before, relu, accumulate, segs = [(dY, X)], share) -- read-only"""
    g = _gen('ln_group', M)
    groups = []
    for N, ns, relu, acc in zip(LN_GROUP_WIDTHS, LN_GROUP_NSEGS, LN_GROUP_RELU, LN_GROUP_ACC):
        gamma, beta, dg0, db0 = _ln_params(g, N)
        segs, zeroed = [], 0.0
        for _ in range(ns):
            dY, X, share = _ln_inputs(g, M, N, gamma, beta, relu)
            segs.append((dY, X))
            zeroed += share / ns
        groups.append(dict(gamma=gamma, beta=beta, dgamma_before=dg0, dbeta_before=db0, relu=relu, accumulate=acc, segs=segs, share=zeroed))
    return groups


def ln_group_ref(group):
    """(dgamma, dbeta) of one LayerNorm of ln_group_case: sums over its segments (+ the buffers' contents under accumulate), and the
    per-segment references"""
    refs = [layer_norm_ref(dY, X, group['gamma'], group['beta'], group['relu']) for dY, X in group['segs']]
    dg, db = sum(r['dgamma'] for r in refs), sum(r['dbeta'] for r in refs)
    if group['accumulate']:
        dg, db = dg + group['dgamma_before'].double(), db + group['dbeta_before'].double()
    return dg, db, refs


# ---- multi-segment GEMM ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def gemm_case(M, N, K, leg):
    """8 operand pairs as logical matrices (A_s [M, K], B_s [K, N]), C_before [M, N], and the fp64 products A_s B_s -- read-only.
    nseg < 8 uses the first nseg pairs."""
    g = _gen('gemm', M, N, K, leg)
    if leg == 'int':
        A, B = [_ints(g, -2, 2, M, K) for _ in range(8)], [_ints(g, -2, 2, K, N) for _ in range(8)]
        C0 = _ints(g, -3, 3, M, N)
        assert_exact(8 * K * 4 + 3, 'gemm K=%d' % K)
    else:
        A, B = [torch.randn(M, K, generator=g) for _ in range(8)], [torch.randn(K, N, generator=g) for _ in range(8)]
        C0 = torch.randn(M, N, generator=g)
    prods = [a.double() @ b.double() for a, b in zip(A, B)]
    return A, B, C0, prods


def gemm_ref(case, nseg, accumulate):
    """C (+)= sum_s A_s B_s in fp64"""
    _, _, C0, prods = case
    ref = sum(prods[:nseg]) if nseg else torch.zeros_like(prods[0])
    return ref + C0.double() if accumulate else ref


def stored(mat, kmajor, outer_is_rows):
    """the storage of a logical operand: A [M, K] is k-major as [K, M]; B [K, N] is k-major as it stands, row-major as [N, K]"""
    if outer_is_rows:                       # A: logical [outer, k]
        return mat.t().contiguous() if kmajor else mat.contiguous()
    return mat.contiguous() if kmajor else mat.t().contiguous()
