"""The reference of the rasterizer's depth and alpha maps, built from the CPU oracle as it stands (nothing under oracle/ changes).

Depth and alpha are two further blended channels with background 0 -- depth has the channel value z_i (the view-space depth the sort orders by), alpha
the channel value 1 -- so a SECOND oracle run on the same geometry with colors_precomp = (z_i, 1, 0) and bg = 0 yields both maps in planes 0 and 1, and
its backward pass their gradients.  The only piece the oracle does not chain is dL/dz_i -> mean3D (precomputed colours are inputs to it): z = mean3D .
viewmatrix[:3, 2] + viewmatrix[3, 2], so that term is the oracle's colour gradient of plane 0 times viewmatrix[:3, 2]."""
import numpy as np

import oracle


def oracle_pair(sc, cam, bg, dtype=np.float32, scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None):
    """(colour, aux, st, st2): the colour run as every parity test makes it, and the run whose planes 0 / 1 are the depth / alpha maps."""
    geo = dict(scales=sc['scales'], rotations=sc['rotations']) if cov3D_precomp is None else dict(cov3D_precomp=cov3D_precomp)
    col = dict(shs=sc['shs']) if colors_precomp is None else dict(colors_precomp=colors_precomp)
    args = (sc['means3D'], sc['opacities'], cam['viewmatrix'], cam['projmatrix'], cam['campos'], cam['tanfovx'], cam['tanfovy'], cam['width'], cam['height'])
    colour, _, st = oracle.gs_forward(*args, np.asarray(bg, dtype), sh_degree=sc['sh_degree'], scale_modifier=scale_modifier, dtype=dtype, **col, **geo)
    channels = np.stack([st.depths, np.ones_like(st.depths), np.zeros_like(st.depths)], -1)
    aux, _, st2 = oracle.gs_forward(*args, np.zeros(3, dtype), sh_degree=sc['sh_degree'], colors_precomp=channels, scale_modifier=scale_modifier, dtype=dtype, **geo)
    return colour, aux, st, st2


def expected_gradients(st, st2, cam, g_rgb, g_d, g_a):
    """Gradients of <g_rgb, colour> + <g_d, depth> + <g_a, alpha>: dict with mean3D, mean2D, opacity, scale, rot, cov3D (the sum of the two oracle backward
    passes, plus the depth term of mean3D) and sh / color (the colour run alone)."""
    a = oracle.gs_backward(st, g_rgb)
    b = oracle.gs_backward(st2, np.stack([g_d, g_a, np.zeros_like(g_d)]))
    out = {k: a[k] + b[k] for k in ('mean3D', 'mean2D', 'opacity', 'scale', 'rot', 'cov3D')}
    out['mean3D'] = out['mean3D'] + b['color'][:, 0, None] * np.asarray(cam['viewmatrix'], st.dtype)[None, :3, 2]
    out['sh'], out['color'] = a['sh'], a['color']
    return out
