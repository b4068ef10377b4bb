"""sparsebev_amd.optim.FusedAdamW on the device (csrc/optim.hip): the update against an fp32 restatement bit for bit, the gradient norm,
clipping, the loss scale, the skipped step, version counters, capture, state dicts.  Shapes: a few tens of thousands of elements."""
import copy

import numpy as np
import pytest
import torch

from sparsebev_amd import optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = optim.CHUNK
f32 = np.float32

SIZES = [1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]
BETAS, EPS = (0.9, 0.999), 1e-8
GROUPS = [dict(lr=2e-4, weight_decay=0.01, lr_mult=1.0), dict(lr=3e-3, weight_decay=0.1, lr_mult=0.1)]


def make_params(sizes, seed, misaligned=True):
    """Parameters of the given sizes (values ~ N(0, 1)), then -- misaligned -- one whose base AND gradient sit at offset 1 of a larger
    buffer (4-byte, not 16-byte aligned) and one whose gradient alone does."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in sizes]
    if misaligned:
        buf = torch.randn(1028, generator=g).to(DEV)
        ps.append(torch.nn.Parameter(buf[1:]))
        ps.append(torch.nn.Parameter(torch.randn(2 * C + 5, generator=g).to(DEV)))
        assert ps[-2].data_ptr() % 16 == 4 and ps[-1].data_ptr() % 16 == 0
    return ps


def make_grads(ps, seed, misaligned=True):
    """magnitudes 10^U(-6, 2), random signs (host arrays); install() puts them into .grad, keeping the misaligned placement"""
    rng = np.random.default_rng(seed)
    return [(np.sign(rng.standard_normal(p.numel())) * 10.0 ** rng.uniform(-6, 2, p.numel())).astype(f32) for p in ps]


def install(ps, grads, misaligned=True, scale=1.0):
    for i, (p, g) in enumerate(zip(ps, grads)):
        t = torch.from_numpy(g * f32(scale)).to(DEV)
        if misaligned and i >= len(ps) - 2:
            buf = torch.zeros(t.numel() + 1, device=DEV)
            buf[1:] = t
            t = buf[1:]
            assert t.data_ptr() % 16 == 4
        if p.grad is not None and p.grad.shape == t.shape and getattr(p, '_static_grad', False):
            p.grad.copy_(t)
        else:
            p.grad = t


def grouped(ps):
    return [dict(params=ps[0::2], **GROUPS[0]), dict(params=ps[1::2], **GROUPS[1])]


def group_of(ps):
    return [i % 2 for i in range(len(ps))]


class Restated:
    """The definition in csrc/optim.hip restated with NumPy: every operation an fp32 operation in the kernel's order, the beta powers
    as running fp64 products, the norm summed in the kernel's order (per thread over its float4s in fp64, the xor tree of a wave, the
    waves in order, one rounding to fp32 per chunk, the chunks in fp64 in index order)."""

    def __init__(self, ps, group, groups=GROUPS, betas=BETAS, eps=EPS, max_norm=None, loss_scale=1.0, dtype=f32):
        self.T = dtype
        self.p = [p.detach().cpu().numpy().astype(dtype) for p in ps]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.group, self.groups, self.betas, self.eps, self.max_norm, self.loss_scale = group, groups, betas, eps, max_norm, loss_scale
        self.t, self.skipped, self.b1p, self.b2p = 0, 0, 1.0, 1.0
        self.norm = None

    @staticmethod
    def chunk_sum(x):                      # x: one chunk of g * inv_scale (fp32)
        n = len(x)
        quads = n // 4
        sq = x.astype(np.float64) ** 2
        acc = np.zeros(256)
        rounds = -(-quads // 256) if quads else 0
        body = np.zeros(rounds * 256 * 4)
        body[:quads * 4] = sq[:quads * 4]
        body = body.reshape(rounds, 256, 4) if rounds else body.reshape(0, 256, 4)
        for r in range(rounds):
            for e in range(4):
                acc = acc + body[r, :, e]
        tail = sq[quads * 4:]
        acc[:len(tail)] = acc[:len(tail)] + tail
        w = acc.reshape(4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lane ^ off]
        s = w[0, 0]
        for k in range(1, 4):
            s = s + w[k, 0]
        return f32(s)

    def grad_norm(self, grads):
        inv = f32(1.0 / self.loss_scale)
        total = 0.0
        for g in grads:
            x = g.astype(f32) * inv
            for first in range(0, len(x), C):
                total = total + float(self.chunk_sum(x[first:first + C]))
        return f32(np.sqrt(total))

    def step(self, grads, norm=None):
        T = self.T
        with np.errstate(all='ignore'):
            norm = self.grad_norm(grads) if norm is None else norm
        self.norm = norm
        clip = T(1)
        if self.max_norm is not None:
            clip = min(T(1), T(f32(self.max_norm)) / (T(norm) + T(f32(1e-6))))
        if not np.isfinite(norm):
            self.skipped += 1
            return
        b1, b2 = self.betas
        self.t += 1
        self.b1p, self.b2p = self.b1p * b1, self.b2p * b2
        exact = T is np.float64
        bc1 = T(1.0 - self.b1p) if exact else f32(1.0 - self.b1p)
        bc2 = T(np.sqrt(1.0 - self.b2p)) if exact else f32(np.sqrt(1.0 - self.b2p))
        c = (lambda x: T(x)) if exact else (lambda x: f32(x))
        inv, beta2, w1, w2, eps = c(1.0 / self.loss_scale), c(b2), c(1.0 - b1), c(1.0 - b2), c(self.eps)
        for i, g in enumerate(grads):
            h = self.groups[self.group[i]]
            lr = c(h['lr']) * c(h['lr_mult'])
            decay = T(1) - lr * c(h['weight_decay'])
            step_size = lr / bc1
            gp = (g.astype(T) * inv) * clip
            p = self.p[i] * decay
            m = self.m[i] + (gp - self.m[i]) * w1
            v = self.v[i] * beta2 + (gp * gp) * w2
            denom = np.sqrt(v) / bc2 + eps
            self.p[i], self.m[i], self.v[i] = p - (step_size * m) / denom, m, v


def state_of(opt, ps):
    torch.cuda.synchronize()
    return ([p.detach().cpu().numpy().copy() for p in ps], [opt.state[p]['exp_avg'].cpu().numpy() for p in ps],
            [opt.state[p]['exp_avg_sq'].cpu().numpy() for p in ps], int(opt.step_count.item()), int(opt.skipped.item()))


def same_bits(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype == f32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            (what, i, a.size, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))


def assert_matches(opt, ps, ref, what):
    p, m, v, t, skipped = state_of(opt, ps)
    same_bits(p, ref.p, what + ': p')
    same_bits(m, ref.m, what + ': exp_avg')
    same_bits(v, ref.v, what + ': exp_avg_sq')
    assert (t, skipped) == (ref.t, ref.skipped), what


def max_err(got, want):
    return max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, want))


@pytest.mark.parametrize('case', ['sizes', 'cap_plus_one'])
def test_three_steps_bit_equal_to_the_fp32_restatement(case):
    """Three consecutive steps (bias corrections at t = 1, 2, 3), two groups with different lr / weight_decay / multiplier, clipping on
    (norm far above max_norm) and a loss scale: parameters, both moments and the norm equal the NumPy fp32 restatement BIT FOR BIT.
    'sizes': 1, 3, 4, 5, 255, 256, 257, C-1, C, C+1, 2C+3 and the two misaligned tensors; 'cap_plus_one': 65 tensors -- two launches of
    each list kernel over one partials workspace.  Printed for the record: the maximum error of the kernel and of
    torch.optim.AdamW(foreach=True) after clip_grad_norm_, same inputs, against the fp64 restatement.  Measured on one MI355X
    (sizes / cap_plus_one): kernel 8.02e-07 / 6.90e-07, torch 8.02e-07 / 6.90e-07 -- the same element in both, parameters up to ~4."""
    sizes = SIZES if case == 'sizes' else [7 + 3 * i for i in range(optim.MAX_TENSORS + 1)]
    mis = case == 'sizes'
    ps = make_params(sizes, 1, mis)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    kw = dict(max_norm=35.0, loss_scale=512.0)
    opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, max_grad_norm=35.0, loss_scale=512.0)
    if case == 'cap_plus_one':
        assert optim.plan([p.numel() for p in ps])[1] == 2
    ref, ref64 = Restated(ps, group_of(ps), **kw), Restated(ps, group_of(ps), dtype=np.float64, **kw)
    topt = torch.optim.AdamW([dict(params=twin[i::2], lr=GROUPS[i]['lr'] * GROUPS[i]['lr_mult'], weight_decay=GROUPS[i]['weight_decay'])
                              for i in range(2)], betas=BETAS, eps=EPS, foreach=True)
    for k in range(3):
        grads = make_grads(ps, 10 + k)
        install(ps, grads, mis, scale=512.0)
        opt.step()
        ref.step([g * f32(512.0) for g in grads])
        assert_matches(opt, ps, ref, 'step %d' % (k + 1))
        assert np.array_equal(f32(opt.grad_norm.item()), ref.norm) and ref.norm > 35.0
        ref64.step([g * f32(512.0) for g in grads], norm=np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))
        for p, g in zip(twin, grads):
            p.grad = torch.from_numpy(g).to(DEV)
        torch.nn.utils.clip_grad_norm_(twin, 35.0, foreach=True)
        topt.step()
    assert ref.t == 3
    mine, torchs = max_err(state_of(opt, ps)[0], ref64.p), max_err([p.detach().cpu().numpy() for p in twin], ref64.p)
    print('optim %s: max |p - fp64| after 3 steps: kernel %.3e, torch AdamW(foreach) %.3e' % (case, mine, torchs))


def test_grad_norm_reproducible_and_as_close_to_fp64_as_torch():
    """The norm of two runs is the same bits, and its error against fp64 is at most twice that of clip_grad_norm_'s total norm on the same
    gradients (floor: 2^-23 relative).  Measured on one MI355X: norm 4.0769e+03, |kernel - fp64| = |clip_grad_norm_ - fp64| = 5.49e-05
    (both return the correctly rounded fp32 value)."""
    ps = make_params(SIZES, 2)
    grads = make_grads(ps, 20)
    seen = []
    for _ in range(2):
        opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, max_grad_norm=1.0)
        opt.hold = True                                   # the norm of a step that changes nothing
        install(ps, grads)
        opt.step()
        seen.append(opt.grad_norm.clone())
    assert torch.equal(seen[0], seen[1])
    want = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads))
    t_norm = torch.nn.utils.clip_grad_norm_(ps, 1e30, foreach=True)
    e_mine, e_torch = abs(float(seen[0].item()) - want), abs(float(t_norm.item()) - want)
    print('grad norm %.9e: |kernel - fp64| %.3e, |clip_grad_norm_ - fp64| %.3e' % (want, e_mine, e_torch))
    assert e_mine <= max(2.0 * e_torch, 2.0 ** -23 * want)
    assert int(opt.skipped.item()) == 1 and int(opt.step_count.item()) == 0


def run_steps(ps0, grads_per_step, misaligned=True, scale=1.0, **kw):
    ps = [torch.nn.Parameter(p.detach().clone()) for p in ps0[:len(ps0) - 2 * misaligned]]
    if misaligned:
        buf = torch.zeros(ps0[-2].numel() + 1, device=DEV)
        buf[1:] = ps0[-2].detach()
        ps += [torch.nn.Parameter(buf[1:]), torch.nn.Parameter(ps0[-1].detach().clone())]
    opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, **kw)
    for grads in grads_per_step:
        install(ps, grads, misaligned, scale)
        opt.step()
    return opt, ps


def test_clipping_below_the_norm_is_exactly_off_and_above_it_scales_the_gradients():
    ps0 = make_params(SIZES, 3)
    grads = [[g * f32(1e-3) for g in make_grads(ps0, 30 + k)] for k in range(2)]
    off, ps_off = run_steps(ps0, grads)
    norm = float(off.grad_norm.item())
    below, ps_below = run_steps(ps0, grads, max_grad_norm=4.0 * norm)
    assert float(below.clip_coef.item()) == 1.0
    a, b = state_of(off, ps_off), state_of(below, ps_below)
    for x, y, what in zip(a[:3], b[:3], ('p', 'exp_avg', 'exp_avg_sq')):
        same_bits(x, y, 'norm below max_norm: ' + what)
    above, ps_above = run_steps(ps0, grads, max_grad_norm=0.25 * norm)
    assert 0.2 < float(above.clip_coef.item()) < 0.3
    ref = Restated(ps0, group_of(ps0), max_norm=0.25 * norm)
    for g in grads:
        ref.step(g)
    assert_matches(above, ps_above, ref, 'norm above max_norm')


def test_loss_scale_512_is_exact():
    ps0 = make_params(SIZES, 4)
    grads = [make_grads(ps0, 40 + k) for k in range(2)]
    plain, ps_a = run_steps(ps0, grads, max_grad_norm=35.0)
    scaled, ps_b = run_steps(ps0, grads, scale=512.0, max_grad_norm=35.0, loss_scale=512.0)
    a, b = state_of(plain, ps_a), state_of(scaled, ps_b)
    for x, y, what in zip(a[:3], b[:3], ('p', 'exp_avg', 'exp_avg_sq')):
        same_bits(x, y, 'loss scale 512: ' + what)
    assert torch.equal(plain.grad_norm, scaled.grad_norm) and a[3] == b[3] == 2


def test_non_finite_gradient_skips_the_step_and_nothing_else():
    ps = make_params(SIZES, 5)
    opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, max_grad_norm=35.0)
    ref = Restated(ps, group_of(ps), max_norm=35.0)
    before = state_of(opt, ps)
    grads = make_grads(ps, 50)
    bad = [g.copy() for g in grads]
    bad[7][C // 2] = np.inf                          # one inf in the middle of the C-1 tensor: a data value
    install(ps, bad)
    opt.step()
    after = state_of(opt, ps)
    for x, y, what in zip(before[:3], after[:3], ('p', 'exp_avg', 'exp_avg_sq')):
        same_bits(x, y, 'skipped step: ' + what)
    assert after[3:] == (0, 1) and not np.isfinite(opt.grad_norm.item())
    bad[7][C // 2] = np.nan
    install(ps, bad)
    opt.step()
    assert state_of(opt, ps)[3:] == (0, 2)
    install(ps, grads)
    opt.step()                                       # the next finite step is step 1
    ref.step(grads)
    ref.skipped = 2
    assert ref.t == 1
    assert_matches(opt, ps, ref, 'first finite step after two skipped ones')


def test_version_counters_and_missing_grad():
    ps = make_params([5, 300], 6, misaligned=False)
    opt = optim.FusedAdamW(ps, lr=1e-3)
    install(ps, make_grads(ps, 60), False)
    before = [p._version for p in ps]
    opt.step()
    assert [p._version for p in ps] == [v + 1 for v in before]
    ps[1].grad = None
    with pytest.raises(RuntimeError, match='no .grad'):
        opt.step()
    with pytest.raises(ValueError, match='contiguous fp32'):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, 4, device=DEV).t())])
    with pytest.raises(ValueError, match='contiguous fp32'):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float64))])
    sched_opt = optim.FusedAdamW(make_params([8], 7, False), lr=1.0)
    sched = torch.optim.lr_scheduler.StepLR(sched_opt, 1, gamma=0.5)           # schedulers write group['lr']
    p = sched_opt.param_groups[0]['params'][0]
    ref = Restated([p], [0], groups=[dict(lr=1.0, weight_decay=1e-2, lr_mult=1.0)])
    for k in range(2):
        g = make_grads([p], 61 + k)
        install([p], g, False)
        sched_opt.step()
        ref.step(g)
        sched.step()
        ref.groups[0]['lr'] = sched_opt.param_groups[0]['lr']
        assert ref.groups[0]['lr'] == 0.5 ** (k + 1)
    assert_matches(sched_opt, [p], ref, 'lr from a scheduler')


def test_capture_replays_equal_eager_steps():
    """opt.step() alone under torch.cuda.graph with static gradients (one stream, no parallel branches): three replays equal three
    eager steps bit for bit, and a group's lr changed between replays (push_hyper() in front of the replay) is honoured."""
    ps0 = make_params(SIZES, 8)
    grads = [make_grads(ps0, 80 + k) for k in range(3)]
    lrs = [2e-4, 1e-4, 5e-5]

    def eager():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in ps0]
        opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, max_grad_norm=35.0)
        for g, lr in zip(grads, lrs):
            opt.param_groups[0]['lr'] = lr
            install(ps, g, False)
            opt.step()
        return state_of(opt, ps)

    want = eager()                                   # also loads the kernels before the capture
    ps = [torch.nn.Parameter(p.detach().clone()) for p in ps0]
    opt = optim.FusedAdamW(grouped(ps), betas=BETAS, eps=EPS, max_grad_norm=35.0)
    install(ps, grads[0], False)
    for p in ps:
        p._static_grad = True
    opt.param_groups[0]['lr'] = lrs[0]
    opt.push_hyper()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert state_of(opt, ps)[3] == 0                 # the capture executed nothing
    for g, lr in zip(grads, lrs):
        install(ps, g, False)
        opt.param_groups[0]['lr'] = lr
        opt.push_hyper()
        graph.replay()
    got = state_of(opt, ps)
    for x, y, what in zip(got[:3], want[:3], ('p', 'exp_avg', 'exp_avg_sq')):
        same_bits(x, y, 'three replays vs three eager steps: ' + what)
    assert got[3:] == want[3:] == (3, 0)


def test_state_dict_moves_between_fused_and_torch_adamw():
    """Two fused steps, state_dict() into torch.optim.AdamW, a third step there: against the fp64 restatement continued from the same
    state, the fused third step is not further off than twice torch's (the bound of the first test where bits cannot be equal: torch
    orders addcdiv / addcmul differently).  The torch state loads back (moments, counter), the fourth fused step equals the fp32
    restatement from that state bit for bit, and unequal ``step`` values are refused."""
    ps0 = make_params(SIZES, 9, misaligned=False)
    groups = [dict(lr=2e-4, weight_decay=0.01, lr_mult=1.0), dict(lr=3e-4, weight_decay=0.1, lr_mult=1.0)]
    grads = [make_grads(ps0, 90 + k) for k in range(4)]
    ps = [torch.nn.Parameter(p.detach().clone()) for p in ps0]
    mk = lambda q: [dict(params=q[i::2], lr=groups[i]['lr'], weight_decay=groups[i]['weight_decay']) for i in range(2)]
    opt = optim.FusedAdamW(mk(ps), betas=BETAS, eps=EPS)
    for k in range(2):
        install(ps, grads[k], False)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all(float(s['step']) == 2.0 and set(s) == {'step', 'exp_avg', 'exp_avg_sq'} for s in sd['state'].values()) and len(sd['state']) == len(ps)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = torch.optim.AdamW(mk(twin), betas=BETAS, eps=EPS, foreach=True)
    topt.load_state_dict(sd)
    ref64 = Restated(ps, group_of(ps), groups=groups, dtype=np.float64)
    ref64.m = [opt.state[p]['exp_avg'].cpu().numpy().astype(np.float64) for p in ps]
    ref64.v = [opt.state[p]['exp_avg_sq'].cpu().numpy().astype(np.float64) for p in ps]
    ref64.t, ref64.b1p, ref64.b2p = 2, BETAS[0] ** 2, BETAS[1] ** 2
    ref64.step(grads[2], norm=1.0)
    install(ps, grads[2], False)
    opt.step()
    for p, g in zip(twin, grads[2]):
        p.grad = torch.from_numpy(g).to(DEV)
    topt.step()
    torch.cuda.synchronize()
    e_mine, e_torch = max_err(state_of(opt, ps)[0], ref64.p), max_err([p.detach().cpu().numpy() for p in twin], ref64.p)
    print('third step after the state moved: max |p - fp64| fused %.3e, torch %.3e' % (e_mine, e_torch))
    assert e_mine <= 2.0 * e_torch
    assert all(float(s['step']) == 3.0 for s in topt.state_dict()['state'].values())
    # and back
    tsd = copy.deepcopy(topt.state_dict())
    back = [torch.nn.Parameter(p.detach().clone()) for p in twin]
    bopt = optim.FusedAdamW(mk(back), betas=BETAS, eps=EPS)
    ptrs = [bopt.state[p]['exp_avg'].data_ptr() for p in back]
    bopt.load_state_dict(tsd)
    assert [bopt.state[p]['exp_avg'].data_ptr() for p in back] == ptrs and int(bopt.step_count.item()) == 3
    ref = Restated(back, group_of(back), groups=groups)
    ref.m = [topt.state[p]['exp_avg'].cpu().numpy() for p in twin]
    ref.v = [topt.state[p]['exp_avg_sq'].cpu().numpy() for p in twin]
    ref.t = 3
    for _ in range(3):
        ref.b1p, ref.b2p = ref.b1p * BETAS[0], ref.b2p * BETAS[1]
    same_bits([bopt.state[p]['exp_avg'].cpu().numpy() for p in back], ref.m, 'loaded exp_avg')
    install(back, grads[3], False)
    bopt.step()
    ref.step(grads[3])
    assert_matches(bopt, back, ref, 'fourth step from the torch state')
    tsd['state'][1]['step'] = tsd['state'][1]['step'] + 1
    with pytest.raises(ValueError, match='step values differ'):
        bopt.load_state_dict(tsd)
