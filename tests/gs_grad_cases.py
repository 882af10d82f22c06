"""The cases of the 3DGS backward budget tests (tests/test_gs_grad_ref_cpu.py on the f32 oracle, tests/test_gpu_gs_grad_budget.py on the kernels) and the
pipeline from a case to its judged reference (tests/gs_grad_ref.py).  Plain module: no test functions.

Base case: scene A's generator settings (seed 11, extent 1.0, log-scale mean log 0.06) with 300 Gaussians at 70 x 45 -- the right tile column is 6 pixels
wide, the bottom tile row 13 pixels high -- orbit pose (0.5, 0.3, 3.0), background (0.2, 0.4, 0.1), N(0, 1) pixel gradients."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle
from tests import gs_grad_ref as R
from tests import scenes

BG = (0.2, 0.4, 0.1)
POSE = (0.5, 0.3, 3.0)
f32 = np.float32


def _scene(n=300, deg=3):
    return scenes.gs_random_scene(n, seed=11, extent=1.0, log_scale_mean=math.log(0.06), sh_degree=deg)


def _case(name, sc=None, w=70, h=45, pose=POSE, cam=None, aux=None, grad='normal', scale_modifier=1.0, form='sh', bg=BG, seed=0):
    sc = _scene() if sc is None else sc
    cam = scenes.gs_camera(w, h, scenes.orbit_pose(*pose)) if cam is None else cam
    return SimpleNamespace(name=name, sc=sc, cam=cam, w=cam['width'], h=cam['height'], aux=aux, grad=grad, scale_modifier=scale_modifier, form=form,
                           bg=np.asarray(bg, f32), seed=seed, n=sc['means3D'].shape[0])


def _sh_dc_times_3():
    sc = _scene()
    sc['shs'][:, 0] *= 3.0
    return sc


def _opaque_third():
    sc = _scene()
    sc['opacities'][::3] = 0.999
    return sc


def _single_wide():
    from tests.test_gpu_gs_pose_grad import _single
    return _single('wide')


def _dense():
    from tests.test_gpu_gs_depth_alpha import _dense_scene
    return _dense_scene()


def _with_camera(name, make, **kw):
    sc, cam = make()
    return _case(name, sc, cam=cam, **kw)


def _precomp():
    """colors_precomp + cov3D_precomp: random colours, the covariances the f32 oracle forms from the base scene's scales and rotations."""
    sc = _scene()
    c = _case('tmp', sc)
    sc['cov3D_precomp'] = forward(c)[0].cov3D.copy()
    sc['colors_precomp'] = np.random.default_rng(1).random((c.n, 3)).astype(f32)
    return sc


def activate(raw, xp=np):
    """Model.py:45-87 in the kernel's own operation order (act_sigmoid, act_scales, act_rotation of gs_raster.hip): 1 / (1 + exp(-x)), exp, q / max(|q|, 1e-12)
    with the squares added left to right.  xp = numpy (float32 arrays) or torch."""
    q = raw['quat']
    norm = xp.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    norm = xp.maximum(norm, f32(1e-12)) if xp is np else norm.clamp_min(1e-12)
    return dict(opacities=(1.0 / (1.0 + xp.exp(-raw['logit'])))[:, 0], scales=xp.exp(raw['log_scale']), rotations=q / norm[:, None]), norm


def _raw():
    """raw_parameters=True with split SH: the model's own tensors.  sc holds the activations (numpy float32; the GPU test replaces them by the device's)."""
    base = _scene()
    rng = np.random.default_rng(7)
    raw = dict(means3D=base['means3D'], dc=base['shs'][:, :1].copy(), rest=base['shs'][:, 1:].copy(),
               logit=np.log(base['opacities'] / (1 - base['opacities'])).astype(f32)[:, None], log_scale=np.log(base['scales']).astype(f32),
               quat=(base['rotations'] * rng.uniform(0.5, 2.0, size=(300, 1))).astype(f32))
    return raw


def with_activations(raw, act, norm):
    sc = dict(means3D=raw['means3D'], shs=np.concatenate([raw['dc'], raw['rest']], 1), sh_degree=3, raw=raw, q_norm=np.asarray(norm, f32))
    sc.update({k: np.ascontiguousarray(v, f32) for k, v in act.items()})
    return sc


def _raw_case():
    raw = _raw()
    act, norm = activate(raw)
    return with_activations(raw, act, norm)


CASES = {
    'partial-70x45-deg3': lambda: _case('partial-70x45-deg3'),
    'partial-9x5': lambda: _case('partial-9x5', w=9, h=5),
    'full-16x16': lambda: _case('full-16x16', w=16, h=16),
    'partial-113x71-2000-deg2': lambda: _case('partial-113x71-2000-deg2', _scene(2000, 2), w=113, h=71),
    'single-wide': lambda: _with_camera('single-wide', _single_wide),
    'dense-plain': lambda: _with_camera('dense-plain', _dense),
    'dense-aux': lambda: _with_camera('dense-aux', _dense, aux='all'),
    'grad-one-pixel': lambda: _case('grad-one-pixel', grad='one_pixel'),
    'grad-tile-exponents': lambda: _case('grad-tile-exponents', grad='tile_exponents'),
    'grad-hot-pixel': lambda: _case('grad-hot-pixel', grad='hot_pixel'),
    'grad-2^-70': lambda: _case('grad-2^-70', grad='tiny'),
    'grad-alternate-tiles-zero': lambda: _case('grad-alternate-tiles-zero', grad='alternate_tiles'),
    'clamp-sh-dc-x3': lambda: _case('clamp-sh-dc-x3', _sh_dc_times_3()),
    'clamp-alpha-0.999': lambda: _case('clamp-alpha-0.999', _opaque_third()),
    'clamp-fov-radius-1.6': lambda: _case('clamp-fov-radius-1.6', pose=(0.5, 0.3, 1.6)),
    'scale-modifier-0.7': lambda: _case('scale-modifier-0.7', scale_modifier=0.7),
    'precomp': lambda: _case('precomp', _precomp(), form='precomp'),
    'raw-split-sh': lambda: _case('raw-split-sh', _raw_case(), form='raw'),
    'aux-all': lambda: _case('aux-all', aux='all'),
    'aux-depth-only': lambda: _case('aux-depth-only', aux='depth_only'),
    'aux-alpha-only': lambda: _case('aux-alpha-only', aux='alpha_only'),
}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------------------------------ pixel gradients
def pixel_gradients(c, seed=None, kind=None):
    """(g (3, H, W), g_d (H, W), g_a (H, W)) float32 of a case, unmasked.  Kinds: N(0, 1) everywhere; ONE non-zero pixel; every tile's gradients times 2^e, e
    drawn per tile from -30 .. 30; one pixel 2^12 times its tile's rest; everything times 2^-70 (BW_E_MIN is -60); every second tile exactly zero."""
    w, h = c.w, c.h
    kind = c.grad if kind is None else kind
    rng = np.random.default_rng(1000 + c.seed if seed is None else seed)
    g, g_d, g_a = (rng.normal(size=s).astype(f32) for s in ((3, h, w), (h, w), (h, w)))
    ty, tx = np.meshgrid(np.arange(h) // 16, np.arange(w) // 16, indexing='ij')
    gx = (w + 15) // 16
    scale = np.ones((h, w), f32)
    if kind == 'one_pixel':
        scale[:] = 0
        scale[h // 2 - 3, w // 2 + 2] = 1
    elif kind == 'tile_exponents':
        e = rng.integers(-30, 31, size=gx * ((h + 15) // 16))
        scale = np.ldexp(f32(1), e[ty * gx + tx]).astype(f32)
    elif kind == 'hot_pixel':
        scale[h // 2 + 1, w // 2 - 5] = 4096
    elif kind == 'tiny':
        scale[:] = 2.0 ** -70
    elif kind == 'alternate_tiles':
        scale[(ty * gx + tx) % 2 == 1] = 0
    else:
        assert kind == 'normal', kind
    g, g_d, g_a = g * scale, g_d * scale, g_a * scale
    if c.aux == 'depth_only':
        g[:], g_a[:] = 0, 0
    elif c.aux == 'alpha_only':
        g[:], g_d[:] = 0, 0
    return g, g_d, g_a


# ------------------------------------------------------------------------------------------------------------------------ the f32 oracle
def forward(c, sc=None):
    """(st, st2): the f32 oracle's forward state of a case, and with the maps the second run whose colours are (z, 1, 0) (gs_depth_alpha_ref.oracle_pair)."""
    sc, cam = c.sc if sc is None else sc, c.cam
    geo = dict(cov3D_precomp=sc['cov3D_precomp']) if 'cov3D_precomp' in sc else dict(scales=sc['scales'], rotations=sc['rotations'])
    col = dict(colors_precomp=sc['colors_precomp']) if 'colors_precomp' in sc else dict(shs=sc['shs'])
    args = (sc['means3D'], sc['opacities'], cam['viewmatrix'], cam['projmatrix'], cam['campos'], cam['tanfovx'], cam['tanfovy'], c.w, c.h)
    _, _, st = oracle.gs_forward(*args, c.bg, sh_degree=sc['sh_degree'], scale_modifier=c.scale_modifier, **col, **geo)
    st2 = None
    if c.aux:
        channels = np.stack([st.depths, np.ones_like(st.depths), np.zeros_like(st.depths)], -1)
        _, _, st2 = oracle.gs_forward(*args, np.zeros(3, f32), sh_degree=sc['sh_degree'], colors_precomp=channels, scale_modifier=c.scale_modifier, **geo)
    return st, st2


SUM_COLUMNS = (('color', 0), ('color', 1), ('color', 2), ('opacity', None), ('mean2D', 0), ('mean2D', 1), ('conic', 0), ('conic', 1), ('conic', 3))


def sums_of(grads, gz=None):
    """(P, 9 | 10) in gs_grad_ref's column order from a dict in the oracle's names."""
    cols = [grads[k] if j is None else grads[k][:, j] for k, j in SUM_COLUMNS] + ([] if gz is None else [gz])
    return np.stack(cols, 1)


def raw_chain_f32(c, leaves):
    """The raw-parameter chain of preprocess_bw_one in float32 numpy, on a dict of activated-leaf gradients (the f32 oracle's)."""
    sc = c.sc
    o, s, q, n = sc['opacities'], sc['scales'], sc['rotations'], sc['q_norm']
    out = dict(leaves)
    out['opacity'] = leaves['opacity'] * (o * (f32(1) - o))
    out['scale'] = leaves['scale'] * s
    g = leaves['rot']
    dot = q[:, 0] * g[:, 0] + q[:, 1] * g[:, 1] + q[:, 2] * g[:, 2] + q[:, 3] * g[:, 3]
    out['rot'] = (g - q * dot[:, None]) / n[:, None]
    return out


def oracle_leaves(c, st, st2, S32):
    """The f32 oracle's stage 2 on f32 sums S32 (P, NQ) (its own, or a test's planted variant): every leaf in the oracle's names, float32."""
    S32 = np.asarray(S32, f32)
    m2, con, op, col = R._sums_to_inputs(S32.astype(np.float64), st.P)
    out = oracle.gs_gaussian_backward(st, m2, con, op, col)
    if S32.shape[1] == 10:
        out['mean3D'] = out['mean3D'] + (S32[:, 9, None] * np.asarray(c.cam['viewmatrix'], f32)[None, :3, 2]) * (st.radii > 0)[:, None]
    if c.form == 'raw':
        out = raw_chain_f32(c, out)
    return out


def oracle_sums(c, st, st2, g, g_d, g_a):
    """The f32 oracle's (serial, one thread) blend sums (P, 9 | 10) of masked gradients; with the maps the sum of its two passes."""
    a = oracle.gs_backward(st, g)
    if not c.aux:
        return sums_of(a)
    b = oracle.gs_backward(st2, np.stack([g_d, g_a, np.zeros_like(g_d)]))
    S = sums_of(a, gz=b['color'][:, 0])
    S[:, 3:9] += sums_of(b)[:, 3:9]
    return S


# ------------------------------------------------------------------------------------------------------------------------ the reference
def reference(c, st, kernel_state=None, grads=None, order='kernel'):
    """SimpleNamespace(blend, g, g_d, g_a, ref, B, leaf, masked): the judged reference of a case.  st: the f32 oracle's state; kernel_state: float32 arrays
    of the kernel's saved state that replace the oracle's (points_xy, conic_opacity, rgb, cov3D, depths); grads: (g, g_d, g_a) unmasked, default the case's."""
    st64 = R.promote(st, **(kernel_state or {}))
    blend = R.BlendRef(st64, c.bg, aux=bool(c.aux))
    return reference_for(c, st64, blend, grads, order)


def reference_for(c, st64, blend, grads=None, order='kernel'):
    g, g_d, g_a = pixel_gradients(c) if grads is None else grads
    masked = int(blend.ambiguous.sum())
    assert masked <= 0.005 * c.w * c.h, f'{masked} of {c.w * c.h} pixels are ambiguous'
    g, g_d, g_a = blend.mask_ambiguous(g), blend.mask_ambiguous(g_d), blend.mask_ambiguous(g_a)
    ref = blend.sums(g, g_d, g_a) if c.aux else blend.sums(g)
    B = R.blend_budget(ref, c.w, c.h, order)
    leaf = R.LeafRef(st64, ref, B, view_z=np.asarray(c.cam['viewmatrix'])[:3, 2])
    if c.form == 'raw':
        # o: the state's own (0 for a culled Gaussian, whose gradients are zero anyway); |q| in float64 from the raw quaternion
        leaf.to_raw_parameters(st64.conic_opacity[:, 3], c.sc['scales'], c.sc['rotations'], np.sqrt((np.asarray(c.sc['raw']['quat'], np.float64) ** 2).sum(1)))
    return SimpleNamespace(blend=blend, st64=st64, g=g, g_d=g_d, g_a=g_a, ref=ref, B=B, leaf=leaf, masked=masked)


def leaf_names(c):
    """(name in the oracle's dict, ...) of the leaves a case's call has."""
    if c.form == 'precomp':
        return ('mean3D', 'mean2D', 'opacity', 'color', 'cov3D')
    return ('mean3D', 'mean2D', 'opacity', 'scale', 'rot', 'sh')


def judge_all(c, got, leaf, label=''):
    """Judges every leaf of `got` (dict in the oracle's names), prints the worst err / budget per leaf, returns {name: (worst, over, nonzero)}."""
    out = {}
    for name in leaf_names(c):
        arr = np.asarray(got[name], np.float64)
        assert np.isfinite(arr).all(), (c.name, name, 'not finite')
        out[name] = R.judge(arr, leaf.want[name], leaf.budget[name], leaf.A[name])
        live = leaf.A[name] > 0
        print(f'{label}{c.name} {name}: worst err / budget {out[name][0]:.3f}, {out[name][1]} of {int(live.sum())} over budget, '
              f'{out[name][2]} of {int((~live).sum())} A == 0 elements not zero')
    return out
