"""CPU: the vertex view's size function against 4 * sum(R^3), R = res + 2, over the consecutive hashed levels behind the leading dense ones (at most four,
below 128 MB) for the shipped grid and grids around it; the block view's size is untouched; ABI 22 exports the four new entry points."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from nerficg_amd import _lib
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _levels(lib, n, log2_T, base, growth):
    """(res, hashed) per level, restated as in tests/test_gpu_encoder_block_view.py and checked against nrc_grid_layout"""
    offs = (ctypes.c_uint32 * (n + 1))()
    assert lib.nrc_grid_layout(n, log2_T, base, growth, ctypes.cast(offs, ctypes.c_void_p)) == 0
    out = []
    for l in range(n):
        scale = float(np.float32(np.exp2(np.float32(l) * np.log2(np.float32(growth)))) * np.float32(base) - np.float32(1))
        res = int(np.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << log2_T)
        assert offs[l + 1] - offs[l] == size, l
        out.append((res, size < res ** 3))
    return out


SHIPPED = (16, 19, 16, 1.381912879967776)


@pytest.mark.parametrize('cfg', [SHIPPED, (16, 14, 16, SHIPPED[3]), (16, 11, 16, SHIPPED[3]), (16, 21, 16, SHIPPED[3]), (16, 24, 16, SHIPPED[3]),
                                 (16, 19, 400, 1.115), (8, 19, 16, 1.5), (16, 19, 16, 1.05), (16, 19, 16, 1.6)])
def test_size_is_four_bytes_per_vertex_of_the_levels_that_fit(lib, cfg):
    lv = _levels(lib, *cfg)
    first = 0
    while first < 5 and first < len(lv) and not lv[first][1]:
        first += 1
    # the block view stops at 64 MB as well; none of these grids gets there with five dense levels
    assert 32 * sum((r + 1) ** 3 for r, _ in lv[:first]) < 64 << 20
    want, held = 0, 0
    for res, hashed in lv[first:first + 4]:
        if not hashed or want + 4 * (res + 2) ** 3 > 128 << 20:
            break
        want += 4 * (res + 2) ** 3
        held += 1
    assert int(lib.nrc_ngp_vertex_view_bytes(*cfg)) == want
    assert int(lib.nrc_ngp_block_view_bytes(*cfg)) == 32 * sum((r + 1) ** 3 for r, _ in lv[:first])
    if cfg == SHIPPED:
        assert (first, held, want) == (5, 4, 4 * (83 ** 3 + 114 ** 3 + 156 ** 3 + 215 ** 3))
    if cfg[2] == 400:
        assert (first, held, want) == (0, 0, 0)          # the first hashed level alone (402^3 vertices, 260 MB) passes the cap
    if cfg[3] == 1.6:
        assert (first, held) == (4, 3)                             # the view stops in front of the level that would pass the cap


def test_size_refuses_what_the_layout_refuses(lib):
    assert lib.nrc_ngp_vertex_view_bytes(0, 19, 16, 1.38) < 0 and lib.nrc_ngp_vertex_view_bytes(16, 31, 16, 1.38) < 0
    assert lib.nrc_ngp_vertex_view_bytes(16, 19, 16, 0.0) < 0


def test_abi_22_exports_the_vertex_view(lib):
    from nerficg_amd import _lib
    assert _lib.header_abi_version() == 22 == lib.nrc_abi_version()
    protos = _lib.parse_header()
    for name in ('nrc_ngp_vertex_view_bytes', 'nrc_ngp_build_vertex_view', 'nrc_ngp_set_encoder_vertex_view', 'nrc_ngp_set_encoder_vertex_levels'):
        assert name in protos and hasattr(lib, name), name
    assert protos['nrc_ngp_vertex_view_bytes'][0] == 'int64_t' and protos['nrc_ngp_build_vertex_view'][1][-1][0] == 'nrc_stream_t'
    # per host thread, -1 = the compiled default, 0 .. 4
    try:
        assert [lib.nrc_ngp_set_encoder_vertex_levels(v) for v in (-2, -1, 0, 4, 5)] == [-1, 0, 0, 0, -1]
        assert lib.nrc_ngp_set_encoder_vertex_view(None) == 0
    finally:
        lib.nrc_ngp_set_encoder_vertex_levels(-1)
