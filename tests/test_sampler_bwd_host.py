"""What the sampler's backward matrix (tests/sampler_bwd_cases.py) rests on, checked without a device: the restatement IS the backward
(torch.autograd through the oracle's forward, in fp64); evaluated in fp32 it stays inside the bound against its fp64 self on every cell,
so the bound asks nothing an honest fp32 evaluation cannot give; non-finite coordinates give exact zeros; the four admissible
definitions are one where the coordinate products are exact; and the cell list reaches every kernel, level count and piece of index
arithmetic the device test is there for."""
import pytest
import torch

import sampler_bwd_cases as S
from oracle import sparsebev_oracle as O


def _interior_inputs(L=5, C=7, P=6, N=3, Bp=2, Q=5, seed=3):
    """points at least 1e-3 of a pixel away from every pixel boundary and map edge of every level, inside and up to 0.3 outside the map"""
    g = torch.Generator().manual_seed(seed)
    sizes = S.SIZES[:L]
    loc = torch.rand(Bp, Q, P, 3, generator=g) * 1.6 - 0.3
    loc[..., 2] = torch.randint(0, N, (Bp, Q, P), generator=g).float() / (N - 1)
    for _ in range(100):
        bad = torch.zeros(Bp, Q, P, 2, dtype=torch.bool)
        for h, w in sizes:
            for k, m in ((1, h - 1), (0, w - 1)):
                v = loc[..., k].double() * m                   # (m = 0, the one-row level: the product is 0 wherever the point is)
                bad[..., k] |= ((v - torch.round(v)).abs() < 1e-3) & (m > 0)
        if not bad.any():
            break
        loc[..., :2] = torch.where(bad, torch.rand(Bp, Q, P, 2, generator=g) * 1.6 - 0.3, loc[..., :2])
    assert not bad.any()
    feats = [torch.randn(Bp, N, h, w, C, generator=g, dtype=torch.float64) for h, w in sizes]
    wts = torch.softmax(torch.randn(Bp, Q, P, L, generator=g, dtype=torch.float64), -1)
    gout = torch.randn(Bp, Q, C, P, generator=g, dtype=torch.float64)
    return feats, loc, wts, gout


@torch.enable_grad()
def test_restatement_is_the_autograd_of_the_oracle_forward():
    """fp64 loc leaf through O.msmv_sampling_kernel_semantics: all three gradients to 1e-12 relative (away from every boundary the
    products of an fp64 loc decide as the fp32 ones do, and the fractions are those of the exact product)"""
    feats, loc, wts, gout = _interior_inputs()
    fl = [f.clone().requires_grad_(True) for f in feats]
    lc, ww = loc.double().requires_grad_(True), wts.clone().requires_grad_(True)
    O.msmv_sampling_kernel_semantics(fl, lc, ww).backward(gout)
    r = S.restate(feats, loc, wts, gout, torch.float64, exact=(True, True))

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    errs = {'grad_loc': rel(r['gloc'], lc.grad), 'grad_weights': rel(r['gw'], ww.grad)}
    errs.update({'grad_feats[%d]' % l: rel(r['gf'][l], f.grad) for l, f in enumerate(fl)})
    print(errs)
    assert lc.grad[..., 2].abs().max() == 0 and r['gloc'][..., 2].abs().max() == 0
    assert lc.grad[..., :2].abs().max() > 1 and all(f.grad.abs().max() > 0.1 for f in fl)
    assert all(e < 1e-12 for e in errs.values()), errs
    # the same inputs: n and A are what they are said to be
    assert r['gw_n'] == 4 * 7 and r['gloc_n'] == 4 * 7 * 5
    assert all(bool((r[k + '_A'] >= r[k].abs() * (1 - 1e-12)).all()) for k in ('gloc', 'gw'))
    assert all(bool((a >= f.abs() * (1 - 1e-12)).all()) for a, f in zip(r['gf_A'], r['gf']))
    assert sum(int(n.sum()) for n in r['gf_n']) <= 2 * 5 * 6 * 5 * 4 and all(int(n.max()) >= 1 for n in r['gf_n'])


@pytest.mark.parametrize('name', list(S.CELLS))
def test_fp32_restatement_meets_the_bound_against_its_fp64_self(name):
    """The condition that the reference alone stays inside the bound: the restatement in fp32 (rounded fractions) against the four fp64
    definitions.  measured worst error / bound over all cells: grad_loc 0.23, grad_weights 0.27, grad_feats 0.32."""
    c = S.cell_case(name)
    print('fp32 restatement / bound  %-40s %s  (%s kernel)' % (name, ' '.join('%s %.3f' % kv for kv in sorted(c['fp32'].items())), S.kernel_of(c['cell'])))
    assert all(v <= 1 for v in c['fp32'].values()), c['fp32']


@pytest.mark.parametrize('name', list(S.CELLS))
def test_fp32_restatement_with_fma_fractions_meets_the_bound(name):
    """The kernels' arithmetic: each fraction and its complement one fma on the exact product (corner_frac in msmv_sampling_bwd.hip),
    the rest in fp32.  It is inside the bound on every cell (measured worst: grad_loc 0.23, grad_weights 0.27, grad_feats 0.33) -- through the 'one of the four' rule only: against the rounded-fraction
    definition alone it is off by factors up to 3e5 at elements whose A is 0 there.  Taking the complement as 1 - (rounded fraction)
    instead misses the bound about 30 times where a query's points sit just below a pixel boundary (cell L5-C128-P4-N2-ref-bp-alt)."""
    c = S.cell_case(name)
    r = S.restate(c['feats'], c['loc'], c['wts'], c['gout'], torch.float32, exact=(True, True), contracted=True)
    worst = S.check_outputs(c['refs'], r['gloc'], r['gw'], r['gf'])
    print('fp32 restatement, fma fractions / bound  %-40s %s' % (name, ' '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(v <= 1 for v in worst.values()), worst


def test_fma_fractions_pass_only_through_one_of_the_four():
    c = S.cell_case('L4-C64-P8-N6-mix-bp-std')
    r = S.restate(c['feats'], c['loc'], c['wts'], c['gout'], torch.float32, exact=(True, True), contracted=True)
    one = c['refs'][:1]
    alone = max([S.excess(r['gw'], one, 'gw', one[0]['gw_n']), S.excess(r['gloc'], one, 'gloc', one[0]['gloc_n'])] +
                [S.excess(r['gf'][l], S.level_refs(one, l), 'gf', one[0]['gf_n'][l]) for l in range(len(r['gf']))])
    print('against the rounded-fraction definition alone: worst error / bound', alone)
    assert alone > 1


def test_a_dropped_term_breaks_the_bound():
    """one channel's four corner terms missing from the C = 64 grad_weights elements of level 0"""
    c = S.cell_case('L4-C64-P8-N6-mix-bp-std')
    r0 = c['refs'][0]
    full = S.restate(c['feats'], c['loc'], c['wts'], c['gout'], torch.float32)
    cut = [f.clone() for f in c['feats']]
    cut[0][..., 17] = 0                                        # channel 17 of level 0 no longer contributes
    part = S.restate(cut, c['loc'], c['wts'], c['gout'], torch.float32)
    gw = full['gw'].clone()
    gw[..., 0] = part['gw'][..., 0]
    e = S.excess(gw, c['refs'], 'gw', r0['gw_n'])
    print('grad_weights with channel 17 of level 0 dropped: error / bound', e)
    assert e > 50


@pytest.mark.parametrize('name', ['L4-C64-P4-N1-ref-bp-std', 'L5-C24-P32-N1-mix-grouped-std', 'L5-C64-P8-N2-ref-bp-alt', 'padded-C64', 'one-item-C24'])
def test_nonfinite_coordinates_give_exact_zeros(name):
    """a point with a NaN or Inf coordinate: zero grad_loc and grad_weights (and zero A: the device test then demands exact zeros),
    no term in any feature gradient; a finite 1e30 likewise at every level it lies outside of"""
    c = S.cell_case(name)
    cell, loc = c['cell'], c['loc']
    flat = loc.view(-1, 3)
    rows = S.nonfinite_rows(loc)
    kinds = flat[rows, :2]
    assert len(rows) >= 4 and torch.isnan(kinds).any() and torch.isposinf(kinds).any() and torch.isneginf(kinds).any()
    huge = [(r, k) for r in S.special_rows(flat.shape[0]) for k in (0, 1) if bool(flat[r, k].abs() == 1e30) and r not in rows]
    assert huge
    gout0 = c['gout'].clone().permute(0, 1, 3, 2).reshape(-1, cell['C'])
    gout0[rows] = 0
    gout0 = gout0.reshape(cell['Bp'], cell['Q'], cell['P'], cell['C']).permute(0, 1, 3, 2).contiguous()
    for d, r in zip(S.DEFINITIONS, c['refs']):
        for k, width in (('gloc', 3), ('gw', cell['L'])):
            assert bool((r[k].view(-1, width)[rows] == 0).all()) and bool((r[k + '_A'].view(-1, width)[rows] == 0).all())
        for row, k in huge:
            for l, hw in enumerate(cell['sizes']):
                if hw[1 - k] > 1:                              # x scales with W - 1, y with H - 1: 1e30 * 0 = 0 is inside
                    assert r['gw_A'].view(-1, cell['L'])[row, l] == 0
        assert all(bool(torch.isfinite(t).all()) for t in [r['gloc'], r['gw']] + r['gf'])
        without = S.restate(c['feats'], loc, c['wts'], gout0, torch.float64, exact=d)           # the same points with a zero grad_out
        assert all(torch.equal(a, b) for a, b in zip(r['gf'], without['gf']))


def test_four_definitions_coincide_where_the_products_are_exact():
    g = torch.Generator().manual_seed(5)
    L, C, P, N, Bp, Q = 5, 5, 4, 2, 2, 6
    loc = torch.randint(-24, 90, (Bp, Q, P, 3), generator=g).float() / 64          # 7-bit dyadics: x (W - 1) is exact in fp32
    loc[..., 2] = torch.randint(0, N, (Bp, Q, P), generator=g).float()
    feats = [torch.randn(Bp, N, h, w, C, generator=g) for h, w in S.SIZES[:L]]
    wts = torch.softmax(torch.randn(Bp, Q, P, L, generator=g), -1)
    gout = torch.randn(Bp, Q, C, P, generator=g)
    refs = S.references(feats, loc, wts, gout)
    assert refs[0]['gw'].abs().max() > 0.1
    for r in refs[1:]:
        for k in ('gloc', 'gw', 'gloc_A', 'gw_A'):
            assert torch.equal(r[k], refs[0][k]), k
        for k in ('gf', 'gf_A', 'gf_n'):
            assert all(torch.equal(a, b) for a, b in zip(r[k], refs[0][k])), k


def test_the_cells_reach_every_kernel_level_count_and_path():
    cells = S.all_cells()
    assert len(S.CELLS) == len(cells)                          # names are unique
    # every (kernel, L) pair, by the restated rule of launch_bwd, in both grad_out layouts and both pyramid layouts
    for kernel in ('c64', 'generic'):
        for L in range(1, 6):
            mine = [c for c in S.matrix_cells() if S.kernel_of(c) == kernel and c['L'] == L]
            assert {(c['layout'], c['pyr']) for c in mine} == {(a, b) for a in ('ref', 'mix') for b in ('bp', 'grouped')}, (kernel, L)
            assert {len(c['sizes']) for c in mine} == {L}
    # every L meets every C of the generic kernel, every P and every N
    for L in range(1, 6):
        mine = [c for c in S.matrix_cells() if c['L'] == L]
        assert {c['C'] for c in mine} == set(S.C_GENERIC) | {64}, L
        assert {c['P'] for c in mine} == set(S.P_LIST) and {c['N'] for c in mine} == set(S.N_LIST), L
    assert all(c['C'] == 64 or S.kernel_of(c) == 'generic' for c in cells)
    assert all((c['Bp'], c['Q']) == (6, 11) for c in S.matrix_cells())
    missing = [k for k, v in S.coverage(cells).items() if not v]
    assert not missing, missing
    fb, twin = S.CELLS['fallback-px2^20'], S.CELLS['fallback-twin-px64']
    assert (S.kernel_of(fb), S.kernel_of(twin)) == ('generic', 'c64') and fb['stride_px'] == 1 << 20 and twin['stride_px'] == 64
    a, b = S.cell_case(fb['name']), S.cell_case(twin['name'])                  # the same data behind both pixel strides
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ('loc', 'wts', 'gout')) and all(torch.equal(x, y) for x, y in zip(a['feats'] + a['pre'], b['feats'] + b['pre']))
    # in every cell: non-finite coordinates of every kind at the fixed indices, finite points next to them, a query on one pixel, and
    # feature-gradient elements both with and without a live tap (the pre-filled buffers test the addition AND the untouched rest)
    for c in cells:
        case = S.cell_case(c['name'])
        flat = case['loc'].view(-1, 3)
        rows = S.special_rows(flat.shape[0])
        assert torch.isnan(flat[rows]).any() and torch.isinf(flat[rows]).any() and (flat[rows].abs() == 1e30).any(), c['name']
        assert torch.isfinite(flat[:, :2]).all(1).sum() >= flat.shape[0] // 2, c['name']
        n = torch.cat([t.reshape(-1) for t in case['refs'][0]['gf_n']])
        assert n.max() >= min(c['P'], 4), c['name']                 # the query whose points share a pixel
        assert all(p.abs().min() > 0 for p in case['pre'])
    # the padded cells leave room that must stay NaN; the grouped cells really use gdiv = G and stride_g
    assert all(S.descriptor(c)[4] == (c['G'] if c['pyr'] == 'grouped' else 1) * c['C'] + 4 for c in cells if c['pad'])
    assert all(S.descriptor(c)[:1] + S.descriptor(c)[2:3] == ((c['G'], c['C']) if c['pyr'] == 'grouped' else (1, 0)) for c in cells)
    untouched = [c['name'] for c in cells if not any((t == 0).any() for t in S.cell_case(c['name'])['refs'][0]['gf_n'])]
    print('cells in which every pixel has a live tap:', untouched)
    assert len(untouched) < len(cells) // 2


def test_layout_helpers_round_trip():
    for name in ('padded-C24', 'L3-C64-P5-N6-mix-grouped-std'):
        cell = S.CELLS[name]
        f = S.cell_case(name)['feats']
        for l, t in enumerate(f):
            rows = S.device_rows(cell, t)
            assert rows.shape[1] == cell['G'] * cell['C'] and torch.equal(S.host_level(cell, rows, l), t)
        # group g of sample batch b' = bt G + g is the channel slice [g C, (g + 1) C) of image run bt
        g0 = S.to_grouped(f[0], cell['G'])
        assert torch.equal(g0[1 * cell['N'] + 1, :, :, 2 * cell['C']:3 * cell['C']], f[0][1 * cell['G'] + 2, 1])
