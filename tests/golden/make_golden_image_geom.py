"""Generate fixture G17 (g17_image_geom.npz) by running the REFERENCE's own ``RandomTransformImage``
(loaders/pipelines/transforms.py) on small seeded images; Pillow does the pixels.

Runs only in the authoring container (needs /root/reference and Pillow; never on the GPU box).  The module imports mmcv / mmdet, so it
is not imported: the class is located in the parsed source, its registry decorator dropped, and compiled with numpy, torch and
``PIL.Image`` as its globals.  Nothing of the file is written anywhere: only the arrays below are recorded.

Per configuration (tests/image_geom_cases.py: G17_CONFS) the fixture holds under ``<conf>_``:
  img        uint8 [V, H, W, 3]: view 0 random bytes, view 1 a 0 / 255 pattern (both clamps)
  l2i        float64 [V, 4, 4]: ``lidar2img`` before the call
and per call -- ``train<seed>`` in training mode under ``np.random.seed(seed)`` for the seeds of G17_SEEDS, and ``eval`` -- under
``<conf>_<call>_``:
  tuple      float64 [9]: what sample_augmentation returned: resize, newW, newH, crop (4), flip, rotate
  out        uint8 [V, fH, fW, 3]: the images the call left in results['img']
  ida        float32 [4, 4]: img_transform's matrix
  l2i_after  [V, 4, 4]: results['lidar2img'] after the call, in the dtype the reference's expression gave (float64)
  l2i32_after  the same for a float32 ``lidar2img`` (float32)
  shapes     int64 [V, 3]: results['img_shape'] (ori_shape and pad_shape are asserted equal to it here)

    python tests/golden/make_golden_image_geom.py
"""
import ast
import copy
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_geom_cases as C   # noqa: E402  (configurations and input generators only)

REF = '/root/reference'
OUT = os.path.join(HERE, 'g17_image_geom.npz')


def load_class():
    tree = ast.parse(open(os.path.join(REF, 'loaders', 'pipelines', 'transforms.py')).read())
    cls = copy.deepcopy(next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'RandomTransformImage'))
    cls.decorator_list = []
    ns = {'np': np, 'torch': torch, 'Image': Image}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[cls], type_ignores=[])), 'RandomTransformImage', 'exec'), ns)
    return ns['RandomTransformImage']


def inputs(conf, key):
    V, H, W = C.G17_VIEWS, conf['H'], conf['W']
    seed = 170 + sorted(C.G17_CONFS).index(key)
    img = np.stack([C.random_bytes((H, W, 3), seed)] + [C.extremes((H, W, 3), seed + 10 + v) for v in range(1, V)])
    l2i = np.random.RandomState(seed + 20).uniform(-2, 2, size=(V, 4, 4)) * np.array([800.0, 800.0, 1.0, 1.0])[:, None]
    return img, l2i


def main():
    cls = load_class()
    out = {}
    seen = set()
    for key, conf in C.G17_CONFS.items():
        img, l2i = inputs(conf, key)
        out[key + '_img'], out[key + '_l2i'] = img, l2i
        for call in ['train%d' % s for s in C.G17_SEEDS] + ['eval']:
            training = call != 'eval'
            log = {}

            class Tapped(cls):
                def sample_augmentation(self):
                    log['tuple'] = super().sample_augmentation()
                    return log['tuple']

                def img_transform(self, *a, **kw):
                    im, mat = super().img_transform(*a, **kw)
                    log['ida'] = mat
                    return im, mat

            after = {}
            for name, dtype in (('l2i_after', np.float64), ('l2i32_after', np.float32)):
                t = Tapped(ida_aug_conf=copy.deepcopy(conf), training=training)
                results = dict(img=[v.copy() for v in img], lidar2img=[m.astype(dtype) for m in l2i])
                if training:
                    np.random.seed(int(call[5:]))
                results = t(results)
                after[name] = np.stack(results['lidar2img'])
            resize, dims, crop, flip, rotate = log['tuple']
            assert rotate == 0 and log['ida'].dtype == np.float32
            assert results['img_shape'] == results['ori_shape'] == results['pad_shape']
            pre = '%s_%s_' % (key, call)
            out[pre + 'tuple'] = np.array([resize, dims[0], dims[1], *crop, float(flip), rotate], dtype=np.float64)
            out[pre + 'out'] = np.stack(results['img'])
            out[pre + 'ida'] = log['ida']
            out[pre + 'l2i_after'], out[pre + 'l2i32_after'] = after['l2i_after'], after['l2i32_after']
            out[pre + 'shapes'] = np.array([list(s) for s in results['img_shape']], dtype=np.int64)
            assert after['l2i_after'].dtype == np.float64 and after['l2i32_after'].dtype == np.float32
            fH, fW = conf['final_dim']
            if dims[0] - crop[0] < fW:
                seen.add('overhang_right')
            if crop[1] < 0:
                seen.add('negative_crop_y')
            seen.add('flip' if flip else 'no_flip')
            if max(conf['H'] / dims[1], conf['W'] / dims[0]) < 1:
                seen.add('enlarge')
            print(pre, log['tuple'], out[pre + 'out'].shape)
    want = {'overhang_right', 'negative_crop_y', 'flip', 'no_flip', 'enlarge'}
    assert want <= seen, want - seen
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == '__main__':
    main()
