"""Inputs and yardstick of the stand-alone sampler's forward matrix (tests/test_gpu_sampling_matrix.py on the device,
tests/test_sampling_matrix_host.py for what can be checked without one).

Reference: O.msmv_sampling_kernel_semantics with fp64 features and weights and an fp32 ``loc`` -- the coordinate products stay in fp32, so
the fp64 evaluation picks the kernel's taps.  Yardstick: the SAME oracle in fp32 on the same inputs; its worst error against fp64 is what
fp32 arithmetic in another summation order costs (4 L terms per output), and the kernel may be at most 4 times worse."""
import functools

import torch

from oracle import sparsebev_oracle as O

SIZES = [(9, 14), (5, 7), (3, 4), (2, 2), (1, 3)]          # small, odd, down to a one-row level
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
C_LIST = [4, 24, 64, 68, 128]          # one lane quad; a partial trip; a full trip; a second trip with one live quad; two full trips
P_LIST = [1, 3, 4, 5, 8, 32]           # partial chunk; the float4 row store (P == 4); chunk + tail; two chunks; the reference's MAX_POINT
N_LIST = [1, 2, 6, 7]                  # nm1 = 0; the view clamp at other camera counts than the rig's 6
BP, Q, T, G = 6, 11, 2, 3              # B' = B * T * G with B = 1
TOL = 1e-4                             # the project's bound on sampled features
FACTOR = 4.0                           # kernel error <= FACTOR x the fp32 oracle's, both against fp64


def matrix_cells():
    """The full cross L x storage type x buffer taps; (C, P, N) rotate through their lists so that every L meets every value."""
    cells = []
    for L in range(1, 6):
        for j, (name, buf) in enumerate((n, b) for n in DTYPES for b in (1, 0)):
            cells.append((L, name, buf, C_LIST[(j + L) % 5], P_LIST[(j + 2 * L) % 6], N_LIST[(j + L) % 4]))
    return cells


def cell_id(cell):
    return 'L%d-%s-%s-C%d-P%d-N%d' % (cell[0], cell[1], 'buf' if cell[2] else 'global', *cell[3:])


def edge_locs(Bp, Q, P, N, sizes, g):
    """Interior points, exact 0 and 1, within one pixel outside, far outside; views k / (N - 1) plus a z beyond either end (the clamp)."""
    loc = torch.rand(Bp, Q, P, 3, generator=g)
    k = torch.randint(0, N, (Bp, Q, P), generator=g).float()
    loc[..., 2] = k / (N - 1) if N > 1 else torch.rand(Bp, Q, P, generator=g) * 3 - 1
    H0, W0 = sizes[0]
    specials = [0.0, 1.0, -0.5 / (W0 - 1), 1 + 0.5 / (W0 - 1), -0.5 / (H0 - 1), 1 + 0.99 / (H0 - 1),
                -1.0 / (W0 - 1), 1 + 1.0 / (W0 - 1), -3.0, 4.0, 0.5, 1e-7, 1 - 1e-7]
    flat = loc.view(-1, 3)
    step = max(1, flat.shape[0] // (3 * len(specials)))           # spread over the items, not only the first
    for i, s in enumerate(specials):
        r = (3 * i * step) % flat.shape[0]
        flat[r, 0] = s
        flat[(r + step) % flat.shape[0], 1] = s
        flat[(r + 2 * step) % flat.shape[0], 0] = s
        flat[(r + 2 * step) % flat.shape[0], 1] = specials[(i + 5) % len(specials)]
    if N > 1:                                                     # round(z * (N - 1)) = N and -1: clamped to the last / first view
        flat[1::7, 2] = 1 + 0.7 / (N - 1)
        flat[4::7, 2] = -0.7 / (N - 1)
    return loc


def make_inputs(L, C, P, N, dtype_name, Bp=BP, Q=Q, seed=0):
    """(stored features [B', N, H, W, C] per level, loc, weights).  2-byte storage rounds the features ONCE, here: every consumer sees the
    stored values."""
    g = torch.Generator().manual_seed(seed + 1000 * L + 10 * C + P + 100000 * N)
    sizes = SIZES[:L]
    feats = [torch.randn(Bp, N, h, w, C, generator=g).to(DTYPES[dtype_name]) for h, w in sizes]
    loc = edge_locs(Bp, Q, P, N, sizes, g)
    wts = torch.softmax(torch.randn(Bp, Q, P, L, generator=g), -1)
    return feats, loc, wts


def yardstick(feats, loc, wts):
    """(fp64 reference [B', Q, C, P], worst error of the fp32 oracle against it)."""
    wide = [f.float() for f in feats]                                   # exact for bf16 / fp16
    ref = O.msmv_sampling_kernel_semantics([f.double() for f in wide], loc, wts.double())
    e32 = (O.msmv_sampling_kernel_semantics(wide, loc, wts).double() - ref).abs().max().item()
    return ref, e32


@functools.lru_cache(maxsize=None)
def cell_case(L, C, P, N, dtype_name):
    """One cell's inputs, reference and yardstick, computed once and shared (treat as read-only)."""
    feats, loc, wts = make_inputs(L, C, P, N, dtype_name)
    ref, e32 = yardstick(feats, loc, wts)
    return feats, loc, wts, ref, e32


def to_mix(out, B, T, G):
    """[B', Q, C, P] -> the mixing layout [B, Q, G, T * P, C] (b' = (b * T + t) * G + g)."""
    Bp, Q, C, P = out.shape
    return out.reshape(B, T, G, Q, C, P).permute(0, 3, 2, 1, 5, 4).reshape(B, Q, G, T * P, C)


# two items per wave: B' * Q just above the 8192-item threshold and odd (the last wave holds one item); P <= 4 and C <= 64
PIPE_BP, PIPE_Q = 3, 2731
PIPE_CASES = [(1, 1, 4, 'fp32'), (2, 3, 32, 'fp32'), (3, 4, 64, 'fp32'), (5, 2, 64, 'fp32'), (2, 3, 32, 'bf16')]       # (L, P, C, storage)


@functools.lru_cache(maxsize=None)
def pipe_case(L, P, C, dtype_name):
    feats, loc, wts = make_inputs(L, C, P, 6, dtype_name, Bp=PIPE_BP, Q=PIPE_Q, seed=7)
    ref, e32 = yardstick(feats, loc, wts)
    return feats, loc, wts, ref, e32
