"""Generate fixture G16 (g16_image_front.npz) by running the REFERENCE's own image stage on the CPU: the pre-backbone statements of
SparseBEV.extract_feat (models/sparsebev.py) with pad_multiple, GpuPhotoMetricDistortion and GridMask of models/utils.py.

Runs only in the authoring container (needs /root/reference; never on the GPU box).  models/utils.py needs torch and numpy only and is
loaded as it stands.  models/sparsebev.py imports mmcv / mmdet, so it is not imported: its ``extract_feat`` is located in the parsed
source, cut in front of the ``stop_prev_grad`` branch (everything from there on is the backbone), given a ``return img`` and compiled
with a plain namespace as ``self``.  GridMask is then applied as ``extract_img_feat`` does.  Nothing of either file is written anywhere:
only the arrays below are recorded.

Per call (tests/image_front_cases.py: G16_CALLS) the fixture holds, under ``<call>_``:
  img        uint8 input [n, 3, H, W]
  out        the reference's fp32 result [n, 3, Hp, Wp]
  d64        float16(2^20 * (fp64 run - out)): the same code with ``.float()`` read as ``.double()`` on the same draws; the difference
             is at most 1e-5, so out + d64 / 2^20 restores the fp64 run to about 1e-8 at a sixth of the bytes
  log_name / log_val   every numpy.random call the reference made, in order, and what it returned (permutation: three values)
  meta_img_shape / meta_ori_shape / meta_pad_shape [B, N, 3], meta_input_shape [2]
and ``seeds`` (one per call).  The two training seeds are searched such that between the two calls every branch occurs: brightness on
and off, contrast applied in mode 0 and in mode 1, saturation, hue with a wrap in each direction, a non-identity swap, GridMask
applied in one call and skipped in the other; the script fails otherwise.

    python tests/golden/make_golden_image_front.py
"""
import ast
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_front_cases as C   # noqa: E402  (shapes and input generators only)

REF = '/root/reference'
OUT = os.path.join(HERE, 'g16_image_front.npz')
D64_SCALE = 2.0 ** 20


def load_utils():
    spec = importlib.util.spec_from_file_location('ref_utils', os.path.join(REF, 'models', 'utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Double(ast.NodeTransformer):
    """img.float() -> img.double(): the fp64 run"""

    def visit_Attribute(self, node):
        self.generic_visit(node)
        if node.attr == 'float':
            node.attr = 'double'
        return node


def load_front(utils, double):
    tree = ast.parse(open(os.path.join(REF, 'models', 'sparsebev.py')).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'SparseBEV')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == 'extract_feat')
    cut = next(i for i, s in enumerate(fn.body) if isinstance(s, ast.If) and 'stop_prev_grad' in ast.unparse(s.test))
    fn = copy.deepcopy(fn)
    fn.body = fn.body[:cut] + [ast.Return(value=ast.Name(id='img', ctx=ast.Load()))]
    fn.decorator_list = []
    if double:
        fn = _Double().visit(fn)
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    ns = {'torch': torch, 'pad_multiple': utils.pad_multiple}
    exec(compile(mod, 'extract_feat', 'exec'), ns)
    return ns['extract_feat']


class Recorder:
    """numpy.random's functions wrapped while the reference runs"""
    NAMES = ('randint', 'uniform', 'permutation', 'rand')

    def __init__(self):
        self.log = []

    def __enter__(self):
        self.saved = {k: getattr(np.random, k) for k in self.NAMES}
        for k, f in self.saved.items():
            setattr(np.random, k, self._wrap(k, f))
        return self

    def _wrap(self, name, f):
        def g(*a, **kw):
            v = f(*a, **kw)
            self.log.append((name, np.atleast_1d(np.asarray(v, dtype=np.float64))))
            return v
        return g

    def __exit__(self, *exc):
        for k, f in self.saved.items():
            setattr(np.random, k, f)

    def arrays(self):
        val = np.full((len(self.log), 3), np.nan)
        for i, (_, v) in enumerate(self.log):
            val[i, :len(v)] = v
        return np.array([n for n, _ in self.log], dtype='U11'), val


def run(utils, front, img, n_views, training, seed, hsv_tap=None):
    """the reference's stage on img [n, 3, H, W]; returns (out, metas, recorder)"""
    n = img.shape[0]
    B = n // n_views
    self = types.SimpleNamespace(data_aug=copy.deepcopy(C.DATA_AUG), training=training, color_aug=utils.GpuPhotoMetricDistortion(),
                                 stop_prev_grad=0)
    grid = utils.GridMask(ratio=0.5, prob=0.7)
    grid.train(training)
    metas = [dict(ori_shape=[(1, 1, 3)] * n_views) for _ in range(B)]
    real_hsv = utils.rgb_to_hsv
    if hsv_tap is not None:
        def tapped(image, *a, **kw):
            out = real_hsv(image, *a, **kw)
            hsv_tap.append(out[:, 0].clone())
            return out
        utils.rgb_to_hsv = tapped
    np.random.seed(seed)
    try:
        with Recorder() as rec, torch.no_grad():
            x = front(self, torch.from_numpy(img).view(B, n_views, *img.shape[1:]), metas)
            x = grid(x)                                # extract_img_feat: use_grid_mask is True
    finally:
        utils.rgb_to_hsv = real_hsv
    return x, metas, rec


def branches(rec, n, hue_before):
    """which branches a training call took, from its random log"""
    names = [k for k, _ in rec.log]
    vals = [v for _, v in rec.log]
    it = iter(range(len(names)))
    take = lambda: next(it)
    got = set()
    modes = [int(vals[take()][0]) for _ in range(n)]
    for i in range(n):
        if vals[take()][0]:
            take(); got.add('bright_on')
        else:
            got.add('bright_off')
        if modes[i] == 0 and vals[take()][0]:
            take(); got.add('contrast_mode0')
    for i in range(n):
        if vals[take()][0]:
            take(); got.add('sat')
        if vals[take()][0]:
            hue = float(vals[take()][0])
            h = hue_before[i].double() + hue
            if bool((h > 360).any()):
                got.add('hue_wrap_down')
            if bool((h < 0).any()):
                got.add('hue_wrap_up')
    for i in range(n):
        if modes[i] == 1 and vals[take()][0]:
            take(); got.add('contrast_mode1')
        if vals[take()][0]:
            if list(vals[take()]) != [0, 1, 2]:
                got.add('swap')
    assert names[take()] == 'rand'
    got.add('mask_on' if next(it, None) is not None else 'mask_off')
    return got


WANTED = {'bright_on', 'bright_off', 'contrast_mode0', 'contrast_mode1', 'sat', 'hue_wrap_up', 'hue_wrap_down', 'swap'}


def main():
    utils = load_utils()
    front32, front64 = load_front(utils, False), load_front(utils, True)
    imgs = {'train_a': C.make_images(C.G16_SHAPES['train_a'], 161), 'train_b': C.make_images(C.G16_SHAPES['train_b'], 162),
            'eval': C.make_images(C.G16_SHAPES['eval'], 163, special=False), 'aligned': C.make_images(C.G16_SHAPES['aligned'], 164, special=False)}

    def taken(call, seed):
        tap = []
        _, _, rec = run(utils, front32, imgs[call], C.G16_VIEWS[call], True, seed, hsv_tap=tap)
        return branches(rec, imgs[call].shape[0], tap[0])

    seeds = None
    for sa in range(40):
        ta = taken('train_a', sa)
        for sb in range(sa + 1, 40):
            tb = taken('train_b', sb)
            if WANTED <= (ta | tb) and {'mask_on', 'mask_off'} == ({t for t in ta if t.startswith('mask')} | {t for t in tb if t.startswith('mask')}):
                seeds = (sa, sb)
                break
        if seeds:
            break
    assert seeds, 'no pair of seeds below 40 takes every branch'
    seed_of = {'train_a': seeds[0], 'train_b': seeds[1], 'eval': 7, 'aligned': 8}
    both = taken('train_a', seeds[0]) | taken('train_b', seeds[1])
    assert WANTED | {'mask_on', 'mask_off'} <= both, both
    print('seeds', seed_of, 'branches', sorted(both))

    out = {'seeds': np.array([seed_of[c] for c in C.G16_CALLS], dtype=np.int64)}
    worst = 0.0
    for call in C.G16_CALLS:
        img, nv, training = imgs[call], C.G16_VIEWS[call], C.G16_TRAINING[call]
        x32, metas, rec = run(utils, front32, img, nv, training, seed_of[call])
        x64, metas64, rec64 = run(utils, front64, img, nv, training, seed_of[call])
        assert x32.dtype == torch.float32 and x64.dtype == torch.float64
        name, val = rec.arrays()
        name64, val64 = rec64.arrays()
        assert list(name) == list(name64) and np.array_equal(val, val64, equal_nan=True), 'the fp64 run drew other numbers'
        if not training:
            assert list(name) == ['rand'], name              # eval: rand() is consumed, nothing else
        diff = x64.numpy() - x32.numpy().astype(np.float64)
        worst = max(worst, float(np.abs(diff).max()))
        d64 = (diff * D64_SCALE).astype(np.float16)
        assert np.abs(d64.astype(np.float64) / D64_SCALE - diff).max() < 2e-8
        B = len(metas)
        out[call + '_img'] = img
        out[call + '_out'] = x32.numpy()
        out[call + '_d64'] = d64
        out[call + '_log_name'] = name
        out[call + '_log_val'] = val
        for key in ('img_shape', 'ori_shape', 'pad_shape'):
            out[call + '_meta_' + key] = np.array([[list(s) for s in metas[b][key]] for b in range(B)], dtype=np.int64)
        assert all(isinstance(m['input_shape'], torch.Size) for m in metas)
        out[call + '_meta_input_shape'] = np.array(list(metas[0]['input_shape']), dtype=np.int64)
        print(call, tuple(x32.shape), 'random calls', len(name), 'max |fp32 - fp64| %.3g' % np.abs(diff).max())
    out['ref_fp32_vs_fp64'] = np.array(worst)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes; reference fp32 vs fp64: %.3g' % worst)
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == '__main__':
    main()
