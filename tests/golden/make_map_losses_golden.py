#!/usr/bin/env python3
"""tests/golden/make_map_losses_golden.py REFERENCE_ROOT -- writes tests/golden/map_losses.npz: the reference's own depth_smoothness_loss
(src/Optim/Losses/DepthSmoothness.py:31-43) and background_entropy (src/Optim/Losses/BackgroundEntropy.py:6-8), imported from a checkout of the
reference at REFERENCE_ROOT, evaluated in float64 with autograd for the three gradients on the inputs of tests/map_losses_ref.py (`draw`, SHAPES,
GOLDEN_CONFIGS, weights LAMBDA_SMOOTH / LAMBDA_ENTROPY).  The file holds arrays only: per case the inputs (f32) and loss, S, E, g_depth, g_alpha,
g_image in float64, and the same from a float32 evaluation of the same functions (keys with _f32).  Run where the reference is at hand; the tests read the .npz only."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import map_losses_ref as ref  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(reference_root):
    losses = Path(reference_root) / 'src' / 'Optim' / 'Losses'
    smooth = _load(losses / 'DepthSmoothness.py', 'ref_depth_smoothness').depth_smoothness_loss
    entropy = _load(losses / 'BackgroundEntropy.py', 'ref_background_entropy').background_entropy
    out = {}
    for shape in ref.SHAPES:
        depth, alpha, image = ref.draw(shape)
        key0 = 'x'.join(map(str, shape))
        out[key0 + '_depth'], out[key0 + '_alpha'], out[key0 + '_image'] = depth, alpha, image
        for normalize, symmetrical in ref.GOLDEN_CONFIGS:
            key = ref.golden_key(shape, normalize, symmetrical)
            for dtype, tag in ((np.float64, ''), (np.float32, '_f32')):          # float64: the reference; float32: what plain f32 tensor operations give
                d, a, i = (torch.from_numpy(t.astype(dtype)).requires_grad_(True) for t in (depth, alpha, image))
                dn = d / (a + ref.EPS) if normalize else d
                S = smooth(dn[:, None], i)
                E = entropy(a, symmetrical)
                loss = ref.f32(ref.LAMBDA_SMOOTH) * S + ref.f32(ref.LAMBDA_ENTROPY) * E
                loss.backward()
                out[key + tag + '_loss'], out[key + tag + '_S'], out[key + tag + '_E'] = (np.asarray(t.item(), dtype) for t in (loss, S, E))
                out[key + tag + '_g_depth'], out[key + tag + '_g_alpha'], out[key + tag + '_g_image'] = d.grad.numpy(), a.grad.numpy(), i.grad.numpy()
    np.savez_compressed(ROOT / 'tests' / 'golden' / 'map_losses.npz', **out)
    print('wrote', len(out), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
