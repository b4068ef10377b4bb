"""csrc/optim.hip and sparsebev_amd/optim.py without a GPU: the argument validation of the three launches (nothing reaches a launch),
sbev_optim_plan as a literal table, and optim.param_groups against the rule of mmcv's DefaultOptimizerConstructor."""
import ctypes

import pytest
import torch

from sparsebev_amd import _lib, optim

C = optim.CHUNK
CAP = optim.MAX_TENSORS
VP = ctypes.c_void_p


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _entries(lib):
    """sumsq / finish / adamw as call(**overrides) over one good description with fake aligned pointers.  Every row of the table below
    is refused, or is an empty call: no row reaches a launch."""
    base = dict(n=2, numel=[0, 0], ptr=[0x1000, 0x2000], p=None, g=None, m=None, v=None, group=[0, 1], n_groups=2, hyper=0x3000, header=0x4000,
                partials=0x5000, n_partials=0, betas=(0.9, 0.999), eps=1e-8, arrays=True)

    def args(o):
        d = dict(base, **o)
        for k in 'pgmv':
            d[k] = d['ptr'] if d[k] is None else d[k]
        arr = lambda ct, v: (ct * max(len(v), 1))(*v) if d['arrays'] else None
        d['A'] = {k: arr(VP, d[k]) for k in 'pgmv'}
        d['numel_a'], d['group_a'] = arr(ctypes.c_int64, d['numel']), arr(ctypes.c_int32, d['group'])
        return d

    def sumsq(**o):
        d = args(o)
        return lib.sbev_optim_sumsq(d['A']['g'], d['numel_a'], d['n'], VP(d['hyper']), VP(d['partials']), None)

    def finish(**o):
        d = args(o)
        return lib.sbev_optim_finish(VP(d['partials']), d['n_partials'], VP(d['hyper']), VP(d['header']), d['betas'][0], d['betas'][1], None)

    def adamw(**o):
        d = args(o)
        return lib.sbev_optim_adamw(d['A']['p'], d['A']['g'], d['A']['m'], d['A']['v'], d['numel_a'], d['group_a'], d['n'], d['n_groups'],
                                    d['betas'][0], d['betas'][1], d['eps'], VP(d['hyper']), VP(d['header']), None)

    return {'sumsq': sumsq, 'finish': finish, 'adamw': adamw}


def test_validation_table(lib):
    """Status and message of sbev_optim_sumsq / _finish / _adamw.  Accepted rows are lists without elements (0, no launch); everything
    else is refused before any HIP call -- this test runs without a GPU."""
    call = _entries(lib)
    many = dict(n=CAP + 1, numel=[0] * (CAP + 1), ptr=[0x1000] * (CAP + 1), group=[0] * (CAP + 1))
    table = [
        # ---- sbev_optim_sumsq
        ('sumsq', dict(), 0, ''),                                                         # two tensors without elements
        ('sumsq', dict(n=0, arrays=False), 0, ''),
        ('sumsq', dict(numel=[0, 0], g=[0, 0], hyper=0, partials=0), 0, ''),              # nothing is looked at when there is nothing to do
        ('sumsq', dict(arrays=False), -1, 'sbev_optim_sumsq: null array'),
        ('sumsq', many, -1, 'sbev_optim_sumsq: %d tensors (at most %d per call)' % (CAP + 1, CAP)),
        ('sumsq', dict(n=-1), -1, 'sbev_optim_sumsq: -1 tensors (at most %d per call)' % CAP),
        ('sumsq', dict(numel=[4, -1]), -1, 'sbev_optim_sumsq: numel[1] = -1'),
        ('sumsq', dict(numel=[4, 4], hyper=0), -1, 'sbev_optim_sumsq: null hyper / partials'),
        ('sumsq', dict(numel=[4, 4], partials=0), -1, 'sbev_optim_sumsq: null hyper / partials'),
        ('sumsq', dict(numel=[4, 4], g=[0x1000, 0]), -1, 'sbev_optim_sumsq: g[1] is null'),
        ('sumsq', dict(numel=[4, 4], g=[0x1002, 0x2000]), -1, 'sbev_optim_sumsq: g[0] is not 4-byte aligned'),
        ('sumsq', dict(numel=[0, 4], g=[0x1002, 0x2001]), -1, 'sbev_optim_sumsq: g[1] is not 4-byte aligned'),      # an empty tensor's base is not read
        # ---- sbev_optim_finish
        ('finish', dict(n_partials=-1), -1, 'sbev_optim_finish: n_partials = -1'),
        ('finish', dict(betas=(1.0, 0.999)), -1, 'sbev_optim_finish: betas (1, 0.999) not in [0, 1)'),
        ('finish', dict(betas=(0.9, -0.1)), -1, 'sbev_optim_finish: betas (0.9, -0.1) not in [0, 1)'),
        ('finish', dict(hyper=0), -1, 'sbev_optim_finish: null pointer'),
        ('finish', dict(header=0), -1, 'sbev_optim_finish: null pointer'),
        ('finish', dict(n_partials=3, partials=0), -1, 'sbev_optim_finish: null pointer'),
        ('finish', dict(header=0x4004), -1, 'sbev_optim_finish: header is not 8-byte aligned'),
        # ---- sbev_optim_adamw
        ('adamw', dict(), 0, ''),
        ('adamw', dict(n=0, arrays=False), 0, ''),
        ('adamw', dict(arrays=False), -1, 'sbev_optim_adamw: null array'),
        ('adamw', many, -1, 'sbev_optim_adamw: %d tensors (at most %d per call)' % (CAP + 1, CAP)),
        ('adamw', dict(n_groups=0), -1, 'sbev_optim_adamw: 0 groups (1..%d)' % optim.MAX_GROUPS),
        ('adamw', dict(n_groups=optim.MAX_GROUPS + 1), -1, 'sbev_optim_adamw: %d groups (1..%d)' % (optim.MAX_GROUPS + 1, optim.MAX_GROUPS)),
        ('adamw', dict(betas=(0.9, 1.0)), -1, 'sbev_optim_adamw: betas (0.9, 1) not in [0, 1) or eps 1e-08 < 0'),
        ('adamw', dict(eps=-1.0), -1, 'sbev_optim_adamw: betas (0.9, 0.999) not in [0, 1) or eps -1 < 0'),
        ('adamw', dict(numel=[-5, 4]), -1, 'sbev_optim_adamw: numel[0] = -5'),
        ('adamw', dict(group=[0, 2]), -1, 'sbev_optim_adamw: group[1] = 2 out of range (2 groups)'),
        ('adamw', dict(group=[-1, 0]), -1, 'sbev_optim_adamw: group[0] = -1 out of range (2 groups)'),
        ('adamw', dict(numel=[0, 0], group=[0, 5]), -1, 'sbev_optim_adamw: group[1] = 5 out of range (2 groups)'),   # checked for empty tensors too
        ('adamw', dict(numel=[4, 4], hyper=0), -1, 'sbev_optim_adamw: null hyper / header'),
        ('adamw', dict(numel=[4, 4], header=0), -1, 'sbev_optim_adamw: null hyper / header'),
        ('adamw', dict(numel=[4, 4], p=[0, 0x2000]), -1, 'sbev_optim_adamw: tensor 0 has a null pointer'),
        ('adamw', dict(numel=[4, 4], g=[0x1000, 0]), -1, 'sbev_optim_adamw: tensor 1 has a null pointer'),
        ('adamw', dict(numel=[4, 4], m=[0, 0x2000]), -1, 'sbev_optim_adamw: tensor 0 has a null pointer'),
        ('adamw', dict(numel=[4, 4], v=[0x1000, 0]), -1, 'sbev_optim_adamw: tensor 1 has a null pointer'),
        ('adamw', dict(numel=[4, 4], p=[0x1001, 0x2000]), -1, 'sbev_optim_adamw: tensor 0 is not 4-byte aligned'),
        ('adamw', dict(numel=[4, 4], g=[0x1000, 0x2002]), -1, 'sbev_optim_adamw: tensor 1 is not 4-byte aligned'),
        ('adamw', dict(numel=[4, 4], m=[0x1003, 0x2000]), -1, 'sbev_optim_adamw: tensor 0 is not 4-byte aligned'),
        ('adamw', dict(numel=[4, 4], v=[0x1000, 0x2006]), -1, 'sbev_optim_adamw: tensor 1 is not 4-byte aligned'),
    ]
    for name, overrides, status, text in table:
        got = call[name](**overrides)
        err = lib.sbev_last_error().decode() if got != 0 else ''
        assert (got, err) == (status, text), (name, overrides, got, err)


def test_plan_table():
    """sbev_optim_plan: (chunks, launches of each of the two list kernels, workspace bytes).  A chunk belongs to one tensor; a launch
    takes at most 64 tensors; a group of 64 tensors without any element launches nothing."""
    assert C == 8192 and CAP == 64
    table = [
        ([], (0, 0, 0)),
        ([0], (0, 0, 0)),
        ([1], (1, 1, 4)),
        ([1, 3, 4, 5, 255, 256, 257], (7, 1, 28)),
        ([C - 1], (1, 1, 4)),
        ([C], (1, 1, 4)),
        ([C + 1], (2, 1, 8)),
        ([2 * C + 3], (3, 1, 12)),
        ([1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3], (14, 1, 56)),        # 7 + 1 + 1 + 2 + 3
        ([C, 0, C + 1], (3, 1, 12)),
        ([5] * CAP, (CAP, 1, 4 * CAP)),
        ([5] * (CAP + 1), (CAP + 1, 2, 4 * (CAP + 1))),
        ([0] * CAP + [7], (1, 1, 4)),                       # the first group of 64 has no element: one launch
        ([3] * (2 * CAP) + [C + 1], (2 * CAP + 2, 3, 4 * (2 * CAP + 2))),
        ([8388608, 256, 8388608, 256], (2050, 1, 8200)),    # the two big mixing weights and their biases
    ]
    for numels, want in table:
        assert optim.plan(numels) == want, (numels, optim.plan(numels))
    lib = _lib.load()
    out = (ctypes.c_int64 * 3)()
    assert lib.sbev_optim_plan((ctypes.c_int64 * 1)(-1), 1, out) == -1 and b'sbev_optim_plan: numel[0] = -1' in lib.sbev_last_error()
    assert lib.sbev_optim_plan(None, 1, out) == -1 and lib.sbev_optim_plan((ctypes.c_int64 * 1)(1), 1, None) == -1


def _named(names):
    return [(n, torch.nn.Parameter(torch.empty(2, 3, device='meta'))) for n in names]


HEAD_NAMES = [
    'init_query_bbox.weight', 'label_enc.weight',
    'transformer.decoder.decoder_layer.position_encoder.0.weight',
    'transformer.decoder.decoder_layer.self_attn.gen_tau.weight',
    'transformer.decoder.decoder_layer.sampling.sampling_offset.weight',
    'transformer.decoder.decoder_layer.sampling.sampling_offset.bias',
    'transformer.decoder.decoder_layer.sampling.scale_weights.weight',
    'transformer.decoder.decoder_layer.mixing.out_proj.bias',
    'transformer.decoder.decoder_layer.norm1.weight',
]


def test_param_groups_reference_recipe():
    """configs/r50_nuimg_704x256.py:186-193: AdamW lr 2e-4, weight decay 0.01, custom_keys = {'sampling_offset': lr_mult 0.1}."""
    named = _named(HEAD_NAMES)
    groups = optim.param_groups(named, 2e-4, 0.01, {'sampling_offset': dict(lr_mult=0.1)})
    assert len(groups) == 2
    slow = [g for g in groups if g['lr'] == 2e-4 * 0.1]
    assert len(slow) == 1 and slow[0]['names'] == [n for n in HEAD_NAMES if 'sampling_offset' in n] and len(slow[0]['names']) == 2
    assert slow[0]['weight_decay'] == 0.01
    rest = [g for g in groups if g is not slow[0]][0]
    assert rest['lr'] == 2e-4 and rest['weight_decay'] == 0.01 and rest['names'] == [n for n in HEAD_NAMES if 'sampling_offset' not in n]
    by_name = dict(named)
    assert all(p is by_name[n] for g in groups for n, p in zip(g['names'], g['params']))
    # the groups are what torch's own AdamW takes (meta parameters: nothing is computed)
    torch.optim.AdamW([{k: v for k, v in g.items() if k != 'names'} for g in groups], lr=2e-4, weight_decay=0.01)


def test_param_groups_longest_key_wins_and_decay_mult():
    named = _named(HEAD_NAMES)
    keys = {'sampling': dict(lr_mult=0.5), 'sampling_offset': dict(lr_mult=0.1), 'norm': dict(decay_mult=0.0), 'bias': dict(decay_mult=0.5, lr_mult=2.0)}
    groups = optim.param_groups(named, 1e-3, 0.1, keys)
    where = {n: (g['lr'], g['weight_decay']) for g in groups for n in g['names']}
    assert where['transformer.decoder.decoder_layer.sampling.sampling_offset.weight'] == (1e-3 * 0.1, 0.1)       # 'sampling_offset' before 'sampling'
    assert where['transformer.decoder.decoder_layer.sampling.sampling_offset.bias'] == (1e-3 * 0.1, 0.1)         # ... and before 'bias'
    assert where['transformer.decoder.decoder_layer.sampling.scale_weights.weight'] == (1e-3 * 0.5, 0.1)
    assert where['transformer.decoder.decoder_layer.norm1.weight'] == (1e-3, 0.1 * 0.0)
    assert where['transformer.decoder.decoder_layer.mixing.out_proj.bias'] == (1e-3 * 2.0, 0.1 * 0.5)
    assert where['init_query_bbox.weight'] == (1e-3, 0.1)
    # equal length: alphabetical ('bias' before 'norm'), mmcv's sorted(sorted(keys), key=len, reverse=True)
    named = _named(['norm.bias'])
    assert optim.param_groups(named, 1.0, 1.0, {'norm': dict(lr_mult=3.0), 'bias': dict(lr_mult=5.0)})[0]['lr'] == 5.0
    # frozen parameters are left out
    named = _named(['a.weight', 'b.weight'])
    named[1][1].requires_grad_(False)
    groups = optim.param_groups(named, 1.0, 1.0)
    assert [g['names'] for g in groups] == [['a.weight']]


def test_constructor_refusals_without_gpu():
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match='amsgrad'):
        optim.FusedAdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        optim.FusedAdamW([p], maximize=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        optim.FusedAdamW([p])

