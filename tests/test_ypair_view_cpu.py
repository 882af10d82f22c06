"""CPU: the y-pair view's size function against 8 * sum(R^3), R = res + 2, over the consecutive hashed levels behind the leading dense ones (as many as the
library reads by default, at most six, below 1 GiB) for the grids of tests/test_vertex_view_cpu.py; the caps and the error codes; the four entry points in
the header and in the library under ABI 22; the vertex view's size is what it was."""
import pytest

from tests.test_vertex_view_cpu import SHIPPED, _levels, lib  # noqa: F401  (lib: the module's fixture)

YPAIR_MAX, YPAIR_MAX_BYTES = 6, 1 << 30
YPAIR_LEVELS = 5          # NRC_ENC_YPAIR_LEVELS, the measured default: a view holds no level the encoder would not read


def _ypair(lv, first):
    want, held = 0, 0
    for res, hashed in lv[first:first + min(YPAIR_LEVELS, YPAIR_MAX)]:
        if not hashed or want + 8 * (res + 2) ** 3 > YPAIR_MAX_BYTES:
            break
        want += 8 * (res + 2) ** 3
        held += 1
    return want, held


@pytest.mark.parametrize('cfg', [SHIPPED, (16, 14, 16, SHIPPED[3]), (16, 11, 16, SHIPPED[3]), (16, 21, 16, SHIPPED[3]), (16, 24, 16, SHIPPED[3]),
                                 (16, 19, 400, 1.115), (8, 19, 16, 1.5), (16, 19, 16, 1.05), (16, 19, 16, 1.6)])
def test_size_is_eight_bytes_per_vertex_of_the_levels_that_fit(lib, cfg):
    lv = _levels(lib, *cfg)
    first = 0
    while first < 5 and first < len(lv) and not lv[first][1]:
        first += 1
    want, held = _ypair(lv, first)
    assert int(lib.nrc_ngp_ypair_view_bytes(*cfg)) == want < 1 << 32
    if cfg == SHIPPED:
        sizes = [8 * (r + 2) ** 3 for r in (81, 112, 154, 213, 295, 407)]
        assert [round(s / 1e6, 1) for s in sizes] == [4.6, 11.9, 30.4, 79.5, 209.6, 547.3]
        assert (first, held, want) == (5, YPAIR_LEVELS, sum(sizes[:YPAIR_LEVELS]))
    if cfg[1] == 14:
        assert (first, [r for r, _ in lv[2:8]]) == (2, [31, 43, 59, 81, 112, 154])      # the grid of the GPU tests: hashed from res 31
    if cfg[2] == 400:
        assert (first, held, want) == (0, 1, 8 * 402 ** 3)       # level 1 (448^3 records, 719 MB) would pass 1 GiB behind level 0 (520 MB)
    if cfg[3] == 1.05:
        assert held == 0 or lv[first + held - 1][1]               # only hashed levels
    # the vertex view and the block view: what they were
    vwant = 0
    for res, hashed in lv[first:first + 4]:
        if not hashed or vwant + 4 * (res + 2) ** 3 > 128 << 20:
            break
        vwant += 4 * (res + 2) ** 3
    assert int(lib.nrc_ngp_vertex_view_bytes(*cfg)) == vwant
    assert int(lib.nrc_ngp_block_view_bytes(*cfg)) == 32 * sum((r + 1) ** 3 for r, _ in lv[:first])
    if cfg == SHIPPED:
        assert vwant == 4 * (83 ** 3 + 114 ** 3 + 156 ** 3 + 215 ** 3)


def test_size_refuses_what_the_layout_refuses(lib):
    assert lib.nrc_ngp_ypair_view_bytes(0, 19, 16, 1.38) < 0 and lib.nrc_ngp_ypair_view_bytes(16, 31, 16, 1.38) < 0
    assert lib.nrc_ngp_ypair_view_bytes(16, 19, 16, 0.0) < 0
    assert lib.nrc_ngp_build_ypair_view(None, 0, 19, 16, 1.38, None, None) < 0
    assert lib.nrc_ngp_build_ypair_view(None, *SHIPPED, None, None) == (-1 if YPAIR_LEVELS else 0)      # a view to fill and no table, no buffer


def test_abi_22_exports_the_ypair_view(lib):
    from nerficg_amd import _lib
    assert _lib.header_abi_version() == 22 == lib.nrc_abi_version()
    protos = _lib.parse_header()
    for name in ('nrc_ngp_ypair_view_bytes', 'nrc_ngp_build_ypair_view', 'nrc_ngp_set_encoder_ypair_view', 'nrc_ngp_set_encoder_ypair_levels'):
        assert name in protos and hasattr(lib, name), name
    for name in ('bytes', 'build'):        # the same signatures as the vertex view's
        assert protos[f'nrc_ngp_ypair_view_{name}' if name == 'bytes' else f'nrc_ngp_{name}_ypair_view'] == \
            protos[f'nrc_ngp_vertex_view_{name}' if name == 'bytes' else f'nrc_ngp_{name}_vertex_view']
    assert protos['nrc_ngp_set_encoder_ypair_view'] == protos['nrc_ngp_set_encoder_vertex_view']
    assert protos['nrc_ngp_set_encoder_ypair_levels'] == protos['nrc_ngp_set_encoder_vertex_levels']
    # per host thread, -1 = the compiled default, 0 .. 6; the vertex view's setter keeps its range
    try:
        assert [lib.nrc_ngp_set_encoder_ypair_levels(v) for v in (-2, -1, 0, 6, 7, 2 ** 31 - 1)] == [-1, 0, 0, 0, -1, -1]
        assert lib.nrc_ngp_set_encoder_ypair_view(None) == 0
        assert [lib.nrc_ngp_set_encoder_vertex_levels(v) for v in (4, 5)] == [0, -1]
    finally:
        lib.nrc_ngp_set_encoder_ypair_levels(-1)
        lib.nrc_ngp_set_encoder_vertex_levels(-1)
