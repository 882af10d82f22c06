"""CPU-only checks of the ray-list door of the fused InstantNGP frame (include/nerficg_hip.h group 6, nrc_ngp_render_count_rays): declared, exported,
versioned, and refusing bad arguments before anything is launched (there is no GPU here)."""
import ctypes

import pytest

from nerficg_amd import _lib

NAME = 'nrc_ngp_render_count_rays'


@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_header_declares_the_ray_list_count_pass_like_the_camera_one():
    protos = _lib.parse_header()
    assert NAME in protos
    ret, args = protos[NAME]
    assert ret == 'int'
    assert [a for _, a in args[:5]] == ['width', 'height', 'n_rays', 'origin', 'view_direction']
    assert [t for t, _ in args[:5]] == ['int32_t', 'int32_t', 'int64_t', 'const float*', 'const float*']
    # behind the rays: the tail of nrc_ngp_render_count from center3 on, type for type and name for name
    cam = protos['nrc_ngp_render_count'][1]
    first = [a for _, a in cam].index('center3')
    assert args[5:] == cam[first:]


def test_abi_version_and_export(lib):
    assert _lib.header_abi_version() == lib.nrc_abi_version() >= 12
    assert hasattr(lib, NAME)


def _call(lib, **over):
    """One call whose every argument is acceptable -- a 16 x 16 image (2 x 2 tiles) of 256 rays, host dummies where device pointers go -- except what
    `over` replaces; the replaced argument must be refused before a launch is reached."""
    keep = []

    def buf(nbytes):
        b = ctypes.create_string_buffer(nbytes)
        keep.append(b)
        return ctypes.cast(b, ctypes.c_void_p)

    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    keep.append(f3)
    args = dict(width=16, height=16, n_rays=256, origin=buf(256 * 12), view_direction=buf(256 * 12), center3=ctypes.cast(f3, ctypes.c_void_p),
                half3=ctypes.cast(f3, ctypes.c_void_p), near_plane=0.2, far_plane=1000.0, tile_begin=0, n_tiles=4, density_bitfield=buf(64), cascades=1,
                scale=0.5, exp_step_factor=0.0, grid_size=128, max_samples=1024, ray_od=buf(64), ray_t=buf(64), ray_cnt=buf(64), tile_rows=buf(64),
                tile_off=buf(64), counter=buf(64), ts_provisional=None, count_mailbox=None, mailbox_ticket=0, stream=None)
    assert list(args) == [a for _, a in _lib.parse_header()[NAME][1]]
    args.update(over)
    return getattr(lib, NAME)(*args.values())


@pytest.mark.parametrize('over', [dict(n_rays=-1), dict(n_rays=16 * 16 + 1), dict(n_rays=1, origin=None), dict(n_rays=1, view_direction=None),
                                  dict(tile_begin=3, n_tiles=2), dict(tile_begin=0, n_tiles=5), dict(width=0), dict(counter=None)],
                         ids=lambda o: ' '.join(f'{k}={v}' for k, v in o.items()))
def test_bad_arguments_are_refused_before_a_launch(lib, over):
    assert _call(lib, **over) == -1   # NRC_ERR_INVALID
