"""Forward outputs of the stand-alone sampler (csrc/msmv_sampling.hip: launch_t / launch_b / launch_l) for every instantiation its
dispatch can pick: L = 1..5 x {fp32, bf16, fp16} storage x {buffer, global} taps, both output layouts, one and two items per wave, and the
ring / pool entry points -- each against the fp64 kernel-semantics oracle (tests/sampling_cases.py).

Bound per case: the project's 1e-4, and the kernel's worst error against fp64 at most 4 x the fp32 ORACLE's on the same inputs (the two
differ in summation order and FMA use over 4 L terms; a wrong tap, weight or lane shows at 1e-3 or more).  The ratio is printed per case.

Ratios measured on an MI355X (kernel error / fp32-oracle error, both against fp64; absolute errors 1.2e-7 .. 5.1e-7 on outputs of
magnitude 1.5 .. 3.5):
  the 30 cells of the cross, either layout   0.68 .. 2.08; the largest: 2.08 L5 fp16 global C4 P5 N6 (its yardstick, 1.08e-7 over 1320
                                             outputs, is the smallest of all), 1.45 L4 fp16 global C128 P3 N2, 1.32 L5 bf16 global C68 P3 N1,
                                             1.24 L1 fp16 buf C4 P1 N2 and L2 bf16 global C4 P3 N2; every other cell <= 1.11
  two items per wave (8193 items)            0.83 .. 1.17 (L5 P2 C64 fp32)
  ring / pool entry points                   0.53 .. 0.89
so the kernel is as exact as the fp32 oracle (median over the cells 0.97), and the factor of 4 leaves room for the scatter of a maximum over a few hundred
outputs, not for an error."""
import pytest
import torch

import sampling_cases as SC
from sparsebev_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(t):
    return t.to(DEV)


def judge(what, out, ref, e32):
    """out (device, reference layout) against the fp64 reference: both bounds, the ratio printed first."""
    err = (out.cpu().double() - ref).abs().max().item()
    print('%-44s kernel vs fp64 %.3e   fp32 oracle vs fp64 %.3e   ratio %.2f' % (what, err, e32, err / e32))
    assert err < SC.TOL, (what, err)
    assert err <= SC.FACTOR * e32, (what, err, e32, err / e32)


@pytest.mark.parametrize('cell', SC.matrix_cells(), ids=SC.cell_id)
def test_forward_matrix_vs_fp64_oracle(cell):
    L, name, buf, C, P, N = cell
    feats, loc, wts, ref, e32 = SC.cell_case(L, C, P, N, name)
    fd, ld, wd = [dev(f) for f in feats], dev(loc), dev(wts)
    prev = _lib.load().sbev_msmv_buffer_taps(buf)
    try:
        out = ops.msmv_sampling(fd, ld, wd)
        mix = ops.msmv_sampling(fd, ld, wd, out_layout=ops.OUT_MIX, T=SC.T, G=SC.G)
        wide = ops.msmv_sampling([f.float() for f in fd], ld, wd) if name != 'fp32' else None
    finally:
        _lib.load().sbev_msmv_buffer_taps(prev)
    assert out.shape == (SC.BP, SC.Q, C, P) and mix.shape == (1, SC.Q, SC.G, SC.T * P, C)
    judge(SC.cell_id(cell), out, ref, e32)
    judge(SC.cell_id(cell) + ' mix', mix, SC.to_mix(ref, 1, SC.T, SC.G), e32)
    assert torch.equal(mix, SC.to_mix(out, 1, SC.T, SC.G))                  # the two layouts hold the same bits
    if wide is not None:                                                    # 2-byte storage is widened exactly: the fp32 kernel's bits
        assert torch.equal(out, wide)


@pytest.mark.parametrize('case', SC.PIPE_CASES, ids=lambda c: 'L%d-P%d-C%d-%s' % c)
def test_two_items_per_wave_vs_fp64_and_vs_one_item_per_wave(case):
    """B' * Q = 8193: the two-items-per-wave launch, whose prefetch indexes lanes by P * 3 and P * L, at P < 4 and L != 4; the last wave
    holds a single item.  Against fp64, and bit for bit against the same queries in slices that take the one-item launch."""
    L, P, C, name = case
    feats, loc, wts, ref, e32 = SC.pipe_case(*case)
    fd, ld, wd = [dev(f) for f in feats], dev(loc), dev(wts)
    Bp, Q = SC.PIPE_BP, SC.PIPE_Q
    assert Bp * Q >= 8192 and (Bp * Q) % 2 == 1
    big = ops.msmv_sampling(fd, ld, wd)
    judge('pipelined L%d P%d C%d %s' % case, big, ref, e32)
    mix = ops.msmv_sampling(fd, ld, wd, out_layout=ops.OUT_MIX, T=1, G=Bp)
    assert torch.equal(mix, SC.to_mix(big, 1, 1, Bp))
    parts = [ops.msmv_sampling(fd, ld[:, s:s + 1000].contiguous(), wd[:, s:s + 1000].contiguous()) for s in range(0, Q, 1000)]
    assert all(p.shape[0] * p.shape[1] < 8192 for p in parts)
    assert torch.equal(big, torch.cat(parts, dim=1))


@pytest.mark.parametrize('name', ['fp32', 'fp16'])
@pytest.mark.parametrize('L,P', [(2, 3), (5, 5)])
def test_ring_and_pool_entry_points_equal_dense(L, P, name):
    """msmv_sampling_ring / _pool with a permuted slot table and n_slots != T against msmv_sampling_nhwc on the frames gathered into dense
    order, bit for bit, both tap paths and both layouts; the dense result itself against the fp64 oracle."""
    B, T, G, C, n_slots, N, Qn = 2, 3, 2, 8, 5, ops.N_VIEWS, 9
    g = torch.Generator().manual_seed(40 + L)
    sizes = SC.SIZES[:L]
    levels = [torch.randn(B * n_slots * N, h, w, G * C, generator=g).to(SC.DTYPES[name]) for h, w in sizes]
    ring = [3, 0, 4]
    table = torch.tensor([[3, 0, 4], [1, 4, 2]], dtype=torch.int32)
    loc = SC.edge_locs(B * T * G, Qn, P, N, sizes, g)
    wts = torch.softmax(torch.randn(B * T * G, Qn, P, L, generator=g), -1)

    def gather(tab):            # [B * n_slots * N, H, W, GC] -> the dense [B * T * N, H, W, GC] the table names
        return [f.reshape(B, n_slots, N, *f.shape[1:])[torch.arange(B)[:, None], tab.long()].reshape(B * T * N, *f.shape[1:]).contiguous()
                for f in levels]

    dense_pool, dense_ring = gather(table), gather(torch.tensor([ring] * B))
    # the reference layout of the grouped pyramid: sample batch b' = (b * T + t) * G + g reads channel slice g of image run b * T + t
    as_ref = [f.reshape(B * T, N, *f.shape[1:3], G, C).permute(0, 4, 1, 2, 3, 5).reshape(B * T * G, N, *f.shape[1:3], C) for f in dense_pool]
    ref, e32 = SC.yardstick(as_ref, loc, wts)
    ld, wd, lv = dev(loc), dev(wts), [dev(f) for f in levels]
    prev = _lib.load().sbev_msmv_buffer_taps(1)
    try:
        for buf in (1, 0):
            _lib.load().sbev_msmv_buffer_taps(buf)
            for layout in (ops.OUT_REF, ops.OUT_MIX):
                want = ops.msmv_sampling_nhwc([dev(f) for f in dense_pool], B, T, G, ld, wd, out_layout=layout)
                got = ops.msmv_sampling_pool(lv, B, T, G, dev(table), n_slots, ld, wd, out_layout=layout)
                assert torch.equal(got, want) and got.abs().max() > 0
                want_r = ops.msmv_sampling_nhwc([dev(f) for f in dense_ring], B, T, G, ld, wd, out_layout=layout)
                assert torch.equal(ops.msmv_sampling_ring(lv, B, T, G, ring, n_slots, ld, wd, out_layout=layout), want_r)
                assert not torch.equal(want_r[-1], want[-1])                  # sample 1's table is its own
                if layout == ops.OUT_REF:
                    judge('pool L%d P%d %s %s' % (L, P, name, 'buf' if buf else 'global'), got, ref, e32)
                else:
                    assert torch.equal(got, SC.to_mix(ops.msmv_sampling_pool(lv, B, T, G, dev(table), n_slots, ld, wd, out_layout=ops.OUT_REF), B, T, G))
    finally:
        _lib.load().sbev_msmv_buffer_taps(prev)
