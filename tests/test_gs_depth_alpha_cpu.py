"""CPU: depth and alpha maps of the 3DGS rasterizer -- the C ABI of the two new entry points (exported, declared, a band validated before any HIP
call), and the REFERENCE CONSTRUCTION the GPU tests rely on, checked on the oracle alone: a second oracle run with colors_precomp = (z, 1, 0) and
background 0 carries the depth map in plane 0 and the alpha map in plane 1, and the sum of the two oracle backward passes (plus dL/dz through the view
matrix) is the gradient of the three outputs together, against a float64 central finite difference."""
import numpy as np
import pytest

from nerficg_amd import _lib
from tests import scenes
from tests.gs_depth_alpha_ref import expected_gradients, oracle_pair

AUX_SYMBOLS = ('nrc_gs_bin_render_aux_band', 'nrc_gs_backward_aux_band')
NRC_ERR_INVALID = -1


@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    """The entry point with null pointers and zeros everywhere except the named arguments (tests/test_gs_bands_cpu.py)."""
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_aux_entry_points_are_exported_and_declared(lib):
    protos = _lib.parse_header()
    for name, extra in zip(AUX_SYMBOLS, ('out_depth_alpha', 'dL_ddepth_alpha')):
        assert name in protos, name
        assert hasattr(lib, name), name
        band_args = [a for _, a in protos[name.replace('_aux_band', '_band')][1]]
        assert [a for _, a in protos[name][1] if a != extra] == band_args, name          # the band entry point's arguments plus the one map
        assert extra in [a for _, a in protos[name][1]]
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 8
    assert not any(n.startswith('nrc_gs_backward_rest_step') and 'aux' in n for n in protos)      # no aux form of the in-backward Adam step


@pytest.mark.parametrize('name', AUX_SYMBOLS)
@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_a_bad_band_is_invalid_before_any_device_call(lib, name, begin, n):
    """H = 64: four tile rows.  On a machine without a GPU a status comes back: the band is checked in front of every HIP call."""
    protos = _lib.parse_header()
    assert _call(lib, protos, name) == NRC_ERR_INVALID                                   # H = 0: no band is valid
    assert _call(lib, protos, name, P=0, W=64, H=64, tile_row_begin=begin, n_tile_rows=n) == NRC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- the reference construction, on the oracle alone
W, H, N = 64, 48, 300


def _scene():
    sc = scenes.gs_random_scene(N, seed=11, extent=1.0, log_scale_mean=np.log(0.06), sh_degree=3)
    cam = scenes.gs_camera(W, H, scenes.orbit_pose(0.5, 0.3, 3.0))
    return sc, cam


@pytest.fixture(scope='module')
def pair32():
    sc, cam = _scene()
    return (sc, cam) + oracle_pair(sc, cam, [0.2, 0.4, 0.1])


def test_second_run_carries_alpha_and_depth(pair32):
    sc, cam, colour, aux, st, st2 = pair32
    assert np.abs(aux[1].reshape(-1) - (1.0 - st.final_T)).max() <= 2e-6                 # the project's final_T tolerance
    assert not aux[2].any()                                                              # exactly 0
    np.testing.assert_array_equal(st2.ranges, st.ranges)
    np.testing.assert_array_equal(st2.point_list, st.point_list)
    np.testing.assert_array_equal(st2.n_contrib, st.n_contrib)
    np.testing.assert_array_equal(st2.final_T, st.final_T)
    vis = st.radii > 0
    zmin, zmax = st.depths[vis].min(), st.depths[vis].max()
    hit = aux[1] > 0
    assert hit.sum() > 100
    mean_z = aux[0][hit] / aux[1][hit]
    slack = 4 * np.finfo(np.float32).eps * zmax                                          # a weighted mean of f32 sums: a few ulp of the largest depth
    assert mean_z.min() >= zmin - slack and mean_z.max() <= zmax + slack


def test_assembled_gradient_against_a_float64_central_difference():
    """d/dtheta of sum(depth g_d + alpha g_a) for three mean3D components and three opacities, oracle in float64.
    Tolerance, from the step error observed on this scene: the six picked elements differ from the assembled gradient by at most 1.9e-8 of the largest
    picked gradient with the step 1e-5 and by at most 2.9e-10 with the step 1e-6 -- the h^2 law of the truncation error (1.9e-8 / 100 = 1.9e-10) plus
    a float64 rounding part of about eps |f| / h = 1e-10.  The bound is ten times the observed step error at h = 1e-6: 3e-9 relative."""
    sc, cam = _scene()
    rng = np.random.default_rng(5)
    g_d, g_a = rng.normal(size=(H, W)), rng.normal(size=(H, W))
    f64 = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    cam64 = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}

    def value(scene):
        _, aux, _, _ = oracle_pair(scene, cam64, [0.0, 0.0, 0.0], dtype=np.float64)
        return float((aux[0] * g_d).sum() + (aux[1] * g_a).sum())

    _, _, st, st2 = oracle_pair(f64, cam64, [0.0, 0.0, 0.0], dtype=np.float64)
    want = expected_gradients(st, st2, cam64, np.zeros((3, H, W)), g_d, g_a)
    assert not want['sh'].any()                                                           # the colour run alone feeds SH: no colour gradient here
    order_m = np.argsort(-np.abs(want['mean3D']).max(1))[:3]
    picks = [('means3D', (int(i), int(np.argmax(np.abs(want['mean3D'][i])))), want['mean3D']) for i in order_m]
    picks += [('opacities', (int(i),), want['opacity']) for i in np.argsort(-np.abs(want['opacity']))[:3]]
    scale = max(abs(float(ref[idx])) for _, idx, ref in picks)
    assert scale > 0
    h = 1e-6
    for key, idx, ref in picks:
        vals = []
        for sign in (+1.0, -1.0):
            pert = dict(f64)
            pert[key] = f64[key].copy()
            pert[key][idx] += sign * h
            vals.append(value(pert))
        fd = (vals[0] - vals[1]) / (2 * h)
        print(key, idx, 'assembled', float(ref[idx]), 'central difference', fd, 'relative', abs(fd - float(ref[idx])) / scale)
        assert abs(fd - float(ref[idx])) <= 3e-9 * scale, (key, idx, fd, float(ref[idx]))
