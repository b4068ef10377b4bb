"""The atomics-free, bit-reproducible feature gradient of the sampler on the device (ops.deterministic_feature_grad; sbev_msmv_bwd_taps,
torch.sort, sbev_msmv_bwd_sum_sorted): the tap list against an independent restatement, the sum BIT FOR BIT against the host model of
its definition (tests/det_grad_cases.py), run-to-run identity, the existing references through autograd with the switch on, and the
decoder's training step -- eager twice and as a captured graph -- by torch.equal."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import det_grad_cases as D
import test_gpu_backward as TB          # its decoder builder, G11 runner and relative error (helpers only)
from conftest import load_golden, feats_of
from sparsebev_amd import _lib, ops, synthetic as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4          # tests/test_gpu_sampling.py


@pytest.fixture
def det_on():
    prev = ops.deterministic_feature_grad(True)
    yield
    ops.deterministic_feature_grad(prev)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _layout_of(case_index, layout):
    """(feature shapes' leading dims, G for ops._pyramid, T, G of the call) -- 'ref': the stand-alone op's [B', N, H, W, C]; 'mix': grouped
    channels-last [B*T*N, H, W, G*C] with B = 1 and B' = 3 as (T, G) = (1, 3) or (3, 1), alternating over the cases."""
    if layout == 'ref':
        return None, 1, 1
    return ((3, 1, 3), (1, 3, 1))[case_index % 2]


def _buffers(sizes, C, layout_g, T, G, seed):
    """The gradient buffers of one layout, pre-filled with random values (so the final addition is tested).  They also stand in for the
    features where an entry point wants their description: the tap list reads no feature values."""
    g = torch.Generator().manual_seed(seed)
    if layout_g is None:
        return [torch.randn(D.BP, D.N, h, w, C, generator=g).to(DEV) for h, w in sizes]
    return [torch.randn(T * D.N, h, w, G * C, generator=g).to(DEV) for h, w in sizes]


def _device_taps(bufs, layout_g, C, loc, wts):
    (c_feats, c_hw, L), strides = ops._pyramid(bufs, D.N, layout_g)
    Bp, Q, P, _ = loc.shape
    lib = _lib.load()
    n = lib.sbev_msmv_bwd_tap_count(Bp, Q, P, L)
    assert n == Bp * Q * P * L * 4
    keys = torch.full((n,), -7, device=DEV, dtype=torch.int64)
    coefs = torch.full((n,), float('nan'), device=DEV)
    _lib.check(lib.sbev_msmv_bwd_taps(c_feats, c_hw, L, Bp, D.N, C, Q, P, *strides, _p(loc), _p(wts), _p(keys), _p(coefs), _stream()), 'taps')
    return keys, coefs, strides


def _device_sum(bufs, keys, coefs, gout_dev, layout_code, Bp, C, Q, P, T, G):
    L = len(bufs)
    sk, order = torch.sort(keys, stable=True)
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * L)(*[b.data_ptr() for b in bufs])
    _lib.check(lib.sbev_msmv_bwd_sum_sorted(ptrs, L, _p(sk), _p(order), _p(coefs), keys.numel(), _p(gout_dev), layout_code, Bp, C, Q, P, T, G,
                                            _stream()), 'sum')


@pytest.mark.parametrize('layout', ['ref', 'mix'])
@pytest.mark.parametrize('case', D.CASES, ids=D.case_id)
def test_taps_equal_the_restated_geometry(case, layout):
    P, L, C = case
    layout_g, T, G = _layout_of(D.CASES.index(case), layout)
    sizes = D.SIZES[:L]
    loc, wts, _ = D.make_case(P, L, C)
    bufs = _buffers(sizes, C, layout_g, T, G, 1)
    keys, coefs, (gdiv, sbo, sg, sv, spx) = _device_taps(bufs, layout_g, C, loc.to(DEV), wts.to(DEV))
    rk, rc = D.ref_taps(loc, wts, sizes, D.N, gdiv, list(sbo), sg, list(sv), spx)
    keys, coefs = keys.cpu().numpy(), coefs.cpu().numpy()
    assert np.array_equal(keys, rk)                                   # live / sentinel pattern included
    dead = rk == D.KEY_DEAD
    assert dead.any() and (~dead).any() and dead[(1 * D.Q + 2) * P * L * 4:][:L * 4].all()          # the NaN point: no tap is live
    assert not coefs[dead].any() and np.abs(coefs - rc).max() <= 1e-6
    for l, b in enumerate(bufs):                                      # every live offset + its C channels lies inside its level's buffer
        offs = rk[~dead & ((rk >> D.LEVEL_SHIFT) == l)] & ((1 << D.LEVEL_SHIFT) - 1)
        assert offs.size and offs.min() >= 0 and offs.max() + C <= b.numel()


@pytest.mark.parametrize('layout', ['ref', 'mix'])
@pytest.mark.parametrize('case', D.CASES, ids=D.case_id)
def test_sum_equals_the_host_model_bit_for_bit(case, layout):
    P, L, C = case
    layout_g, T, G = _layout_of(D.CASES.index(case), layout)
    sizes = D.SIZES[:L]
    loc, wts, gout = D.make_case(P, L, C)
    bufs = _buffers(sizes, C, layout_g, T, G, 2)
    before = [b.cpu().numpy().reshape(-1) for b in bufs]
    keys, coefs, _ = _device_taps(bufs, layout_g, C, loc.to(DEV), wts.to(DEV))
    want = D.host_feature_grad(keys.cpu().numpy(), coefs.cpu().numpy(), D.to_rows(gout), before, L)
    gdev = (gout if layout == 'ref' else D.to_mix(gout, 1, T, G)).to(DEV)
    _device_sum(bufs, keys, coefs, gdev, ops.OUT_REF if layout == 'ref' else ops.OUT_MIX, D.BP, C, D.Q, P, T, G)
    for l, b in enumerate(bufs):
        got = b.cpu().numpy().reshape(-1)
        assert np.array_equal(got.view(np.uint32), want[l].view(np.uint32)), (l, np.abs(got - want[l]).max())
        assert not np.array_equal(got, before[l])                     # and something was added


def test_long_runs_are_summed_front_to_back():
    """One 1 x 3 level, 700 queries x 4 points at ONE location: two destinations of 2 800 terms each (w = 0.6: columns 0 and 1; the row
    below the map is outside).  Equal to the host model's ascending sum, on inputs where the descending sum of the same terms differs."""
    Q, P, C, L = 700, 4, 64, 1
    g = torch.Generator().manual_seed(3)
    loc = torch.tensor([0.3, 0.5, 0.4]).repeat(1, Q, P, 1).contiguous()
    wts = torch.rand(1, Q, P, L, generator=g) + 0.5
    gout = torch.randn(1, Q, C, P, generator=g)
    bufs = [torch.randn(1, D.N, 1, 3, C, generator=g).to(DEV)]
    before = [bufs[0].cpu().numpy().reshape(-1)]
    keys, coefs, _ = _device_taps(bufs, None, C, loc.to(DEV), wts.to(DEV))
    k = keys.cpu().numpy()
    live = k[k != D.KEY_DEAD]
    assert sorted(np.unique(live, return_counts=True)[1].tolist()) == [2800, 2800]
    rows = D.to_rows(gout)
    want, = D.host_feature_grad(k, coefs.cpu().numpy(), rows, before, L)
    back, = D.host_feature_grad(k, coefs.cpu().numpy(), rows, before, L, descending=True)
    assert not np.array_equal(want, back)                             # these inputs tell the two orders apart
    _device_sum(bufs, keys, coefs, gout.to(DEV), ops.OUT_REF, 1, C, Q, P, 1, 1)
    got = bufs[0].cpu().numpy().reshape(-1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()


def test_run_to_run_and_under_a_busy_device():
    P, L, C = D.CASES[0]
    sizes = D.SIZES[:L]
    loc, wts, gout = D.make_case(P, L, C)
    loc, wts, gout = loc.to(DEV), wts.to(DEV), gout.to(DEV)
    start = _buffers(sizes, C, None, 1, 1, 4)

    def run():
        bufs = [b.clone() for b in start]
        keys, coefs, _ = _device_taps(bufs, None, C, loc, wts)
        _device_sum(bufs, keys, coefs, gout, ops.OUT_REF, D.BP, C, D.Q, P, 1, 1)
        return bufs

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], start[0])
    # a third run on a second stream while a long elementwise kernel occupies the first
    big = torch.ones(1 << 27, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(4):
        big.mul_(1.0000001).add_(1e-9)
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def _with_switch(on, fn):
    prev = ops.deterministic_feature_grad(on)
    try:
        return fn()
    finally:
        ops.deterministic_feature_grad(prev)


@pytest.mark.parametrize('tag', ['L4_C8', 'L5_C64'])
@torch.enable_grad()
def test_g8_reference_gradients_with_the_switch_on(tag):
    g = load_golden('g8_msmv_bwd_' + tag)

    def run():
        feats = [f.to(DEV).requires_grad_(True) for f in feats_of(g)]
        loc, w = g['loc'].to(DEV).requires_grad_(True), g['weights'].to(DEV).requires_grad_(True)
        ops.msmv_sampling(feats, loc, w).backward(g['grad_out'].to(DEV))
        return feats, loc, w

    feats, loc, w = _with_switch(True, run)
    for i, f in enumerate(feats):
        assert (f.grad.cpu() - g['grad_feat%d' % i]).abs().max() < TOL
    assert (w.grad.cpu() - g['grad_weights']).abs().max() < TOL
    scale = max(1.0, g['grad_loc_xy'].abs().max().item())
    assert (loc.grad.cpu()[..., :2] - g['grad_loc_xy']).abs().max() < TOL * scale
    _, loc0, w0 = _with_switch(False, run)
    assert torch.equal(loc.grad, loc0.grad) and torch.equal(w.grad, w0.grad)


@pytest.mark.parametrize('P,L,C', D.CASES, ids=[D.case_id(c) for c in D.CASES])
@torch.enable_grad()
def test_tail_cases_vs_the_oracle_with_the_switch_on(P, L, C):
    from oracle import sparsebev_oracle as O
    g = torch.Generator().manual_seed(P * 10 + L)
    sizes = D.SIZES[:L]
    Bp, Q = 3, 10
    feats = [torch.randn(Bp, 6, h, w, C, generator=g) for h, w in sizes]
    loc = torch.rand(Bp, Q, P, 3, generator=g) * 1.3 - 0.15
    loc[..., 2] = torch.randint(0, 6, (Bp, Q, P), generator=g).float() / 5
    loc[0, 0, 0, :2] = torch.tensor([0.0, 1.0])
    loc[0, 1, 0, :2] = torch.tensor([0.5, 0.5])
    wts = torch.softmax(torch.randn(Bp, Q, P, L, generator=g), -1)
    gout = torch.randn(Bp, Q, C, P, generator=g)

    def run():
        fl = [f.to(DEV).requires_grad_(True) for f in feats]
        lc, ww = loc.to(DEV).requires_grad_(True), wts.to(DEV).requires_grad_(True)
        ops.msmv_sampling(fl, lc, ww).backward(gout.to(DEV))
        return fl, lc, ww

    fl, lc, ww = _with_switch(True, run)
    gf, gl, gw = O.msmv_sampling_backward(feats, loc, wts, gout)
    assert (ww.grad.cpu() - gw).abs().max() < 1e-4
    assert (lc.grad.cpu() - gl).abs().max() < 1e-4 * max(1.0, gl.abs().max().item())
    for a_, r in zip(fl, gf):
        assert (a_.grad.cpu() - r).abs().max() < 1e-4
    fl2, lc0, ww0 = _with_switch(False, run)
    assert torch.equal(lc.grad, lc0.grad) and torch.equal(ww.grad, ww0.grad)
    fl3, _, _ = _with_switch(True, run)
    assert all(torch.equal(a_.grad, b_.grad) for a_, b_ in zip(fl, fl3))


def _decoder_setup():
    B, Q, T, layers = 1, 100, 2, 3
    ih, iw, sizes = S.PYRAMIDS['tiny']
    model = TB.build(T, len(sizes), 77, layers).train()
    model.decoder.decoder_layer.self_attn.attn_drop = 0.0
    model.decoder.decoder_layer.ffn_drop = 0.0
    cot = [torch.randn(layers, B, Q, 10, generator=torch.Generator().manual_seed(5 + i)).to(DEV) for i in range(2)]
    loss_fn = lambda cls, box: (cls * cot[0]).sum() + (box * cot[1]).sum()

    def batch(seed):
        feats = [f.to(DEV) for f in S.make_features(B, T, sizes, seed=seed)]
        bbox, feat = [t.to(DEV) for t in S.make_queries(B, Q, seed=seed + 1)]
        metas = S.make_img_metas(B, T, ih, iw)
        for m in metas:
            m['img_timestamp'] = [t_ - 0.013 * seed * (i // 6) for i, t_ in enumerate(m['img_timestamp'])]
            m['lidar2img'] = [np.asarray(a, np.float32) * (1.0 + 1e-3 * seed) for a in m['lidar2img']]
        return feats, bbox, feat, metas

    return model, loss_fn, batch


def _eager_step(model, loss_fn, feats, bbox, feat, metas):
    for p in model.parameters():
        p.grad = None
    ef = [f.clone().requires_grad_(True) for f in feats]
    eq = feat.clone().requires_grad_(True)
    cls, box = model(bbox, eq, list(ef), None, copy.deepcopy(metas))
    loss = loss_fn(cls, box)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.decoder.named_parameters()}
    return loss.detach().clone(), grads, eq.grad.clone(), [f.grad.clone() for f in ef]


@torch.enable_grad()
def test_decoder_step_is_bit_reproducible_eager_and_captured(det_on):
    """The captured-step test's shapes with the feature gradient on and the switch on: two eager steps agree by torch.equal on every
    parameter, query and feature gradient; the captured step's replay equals the eager step by torch.equal (1e-5 with the atomics);
    flipping the switch after capture makes replay raise."""
    from sparsebev_amd.train_graph import CapturedTrainStep
    model, loss_fn, batch = _decoder_setup()
    # captured on batch A (before the first eager step, as train_graph asks), replayed on batch B
    fa, ba, qa, ma = batch(1)
    fb, bb, qb, mb = batch(2)
    sf = [f.clone().requires_grad_(True) for f in fa]
    sb, sq = ba.clone(), qa.clone().requires_grad_(True)
    step = CapturedTrainStep(model, sb, sq, sf, ma, loss_fn)
    assert step.det_feat_grad is True and len(step.grads) == 48
    with torch.no_grad():
        for d, s_ in zip(sf, fb):
            d.copy_(s_)
        sb.copy_(bb)
        sq.copy_(qb)
    step.replay(mb)
    torch.cuda.synchronize()
    g0 = {n: t.clone() for n, t in step.grads.items()}
    q0 = step.input_grads['query_feat'].clone()
    f0 = [t.clone() for t in step.input_grads['mlvl_feats']]
    ops.deterministic_feature_grad(False)
    try:
        with pytest.raises(RuntimeError, match='deterministic feature gradient'):
            step.replay()
    finally:
        ops.deterministic_feature_grad(True)
    step.replay()                                                     # back under the captured mode: runs, and reproduces itself
    torch.cuda.synchronize()
    assert all(torch.equal(step.grads[n], g0[n]) for n in g0) and all(torch.equal(a, b) for a, b in zip(step.input_grads['mlvl_feats'], f0))
    del step
    # two eager steps on batch B, fresh leaves
    l1, g1, q1, f1 = _eager_step(model, loss_fn, fb, bb, qb, mb)
    l2, g2, q2, f2 = _eager_step(model, loss_fn, fb, bb, qb, mb)
    assert torch.equal(q1, q2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    assert all(torch.equal(a, b) for a, b in zip(f1, f2)) and all(f.abs().max() > 0 for f in f1)
    # the replay equals the eager step on every gradient
    worst = max(TB.rel(g0[n], g1[n]) for n in g1)
    print('captured vs eager: worst relative parameter-gradient difference %.3e, features %.3e' % (worst, max(TB.rel(a, b) for a, b in zip(f0, f1))))
    assert torch.equal(q0, q1)
    for n in g1:
        assert torch.equal(g0[n], g1[n]), n
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)
    for p in model.parameters():
        p.grad = None


@torch.enable_grad()
def test_g11_two_layer_gradients_hold_with_the_switch_on(det_on):
    errs, got = TB._g11_run('L2', value_forced=True)
    ranked = sorted(errs.items(), key=lambda kv: -kv[1])
    assert ranked[0][1] < 1e-4, ranked[:8]


@torch.enable_grad()
def test_default_mode_never_builds_a_tap_list(monkeypatch):
    lib = _lib.load()
    real, calls = lib.sbev_msmv_bwd_taps, []

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, 'sbev_msmv_bwd_taps', counted)
    P, L, C = D.CASES[3]
    loc, wts, gout = D.make_case(P, L, C)
    loc[1, 2, 0, 0] = 0.5

    def run():
        feats = [torch.zeros(D.BP, D.N, h, w, C, device=DEV).requires_grad_(True) for h, w in D.SIZES[:L]]
        lc = loc.to(DEV).requires_grad_(True)
        ops.msmv_sampling(feats, lc, wts.to(DEV)).backward(gout.to(DEV))
        return feats

    assert not ops.deterministic_feature_grad() and not torch.are_deterministic_algorithms_enabled()
    off = run()
    assert calls == []
    on = _with_switch(True, run)
    assert calls == [1]                                               # the wrapper does see the call when the mode is on
    assert all((a.grad - b.grad).abs().max() < 1e-4 for a, b in zip(off, on))
