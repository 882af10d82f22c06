"""CPU: one 3DGS view as tile-row bands -- the C ABI of the band entry points (exported, declared, validated before any HIP call), the partition
rule of parallel.tile_row_band, and the host logic of the band-parallel step on two and four gloo ranks with a fake per-band renderer: the gather
composes the frame, its backward hands each rank its own rows, and the summed sparse exchange equals a dense all-reduce-sum."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nerficg_amd import _lib, parallel

BAND_SYMBOLS = ('nrc_gs_bin_hist_bytes_band', 'nrc_gs_preprocess_band', 'nrc_gs_bin_render_band', 'nrc_gs_backward_band')
NRC_OK, NRC_ERR_INVALID = 0, -1


@pytest.fixture(scope='module')
def lib():
    if not _lib.LIB_PATH.exists():
        from nerficg_amd.build import build
        build(verbose=False)
    return _lib.load()


def _call(lib, protos, name, **values):
    """The entry point with null pointers and zeros everywhere except the named arguments."""
    args = []
    for t, arg in protos[name][1]:
        if arg in values:
            args.append(values[arg])
        else:
            args.append(None if ('*' in t or t == 'nrc_stream_t') else (0.0 if t in ('float', 'double') else 0))
    return getattr(lib, name)(*args)


def test_band_entry_points_are_exported_and_declared(lib):
    protos = _lib.parse_header()
    for name in BAND_SYMBOLS:
        assert name in protos, name
        assert hasattr(lib, name), name
        arg_names = [a for _, a in protos[name][1]]
        assert 'tile_row_begin' in arg_names and 'n_tile_rows' in arg_names, name
    assert not any(n.startswith('nrc_gs_backward_rest_step') and 'band' in n for n in protos)     # Adam on a partial gradient: no band form
    assert lib.nrc_abi_version() == _lib.header_abi_version() >= 7
    # the earlier signatures are what they were: a band is an addition
    for old, new in (('nrc_gs_preprocess', 'nrc_gs_preprocess_band'), ('nrc_gs_bin_render', 'nrc_gs_bin_render_band'), ('nrc_gs_backward', 'nrc_gs_backward_band')):
        old_args, new_args = [a for _, a in protos[old][1]], [a for _, a in protos[new][1]]
        assert [a for a in new_args if a not in ('tile_row_begin', 'n_tile_rows', 'band_mask')] == old_args


@pytest.mark.parametrize('name', BAND_SYMBOLS)
def test_band_entry_points_return_a_status_for_null_pointers(lib, name):
    """Null pointers and zero sizes on a machine without a GPU: a status comes back, nothing is dereferenced or launched."""
    protos = _lib.parse_header()
    assert _call(lib, protos, name) == NRC_ERR_INVALID                                                      # H = 0 has no tile rows: no band is valid
    status = _call(lib, protos, name, W=64, H=64, tile_row_begin=0, n_tile_rows=4)                           # a valid band, nothing else
    if name == 'nrc_gs_bin_hist_bytes_band':
        assert status == lib.nrc_gs_bin_hist_bytes(0, 64, 64, 0) > 0
    else:
        assert status == NRC_ERR_INVALID                                                                    # the entry point's own argument checks


@pytest.mark.parametrize('name', BAND_SYMBOLS)
@pytest.mark.parametrize('begin,n', [(-1, 2), (0, 0), (3, 2), (4, 1), (0, 5), (2, -1)])
def test_out_of_range_bands_are_invalid(lib, name, begin, n):
    """H = 64: gy = 4 tile rows.  tile_row_begin < 0, n_tile_rows < 1 and begin + n > gy are NRC_ERR_INVALID, from every band entry point."""
    protos = _lib.parse_header()
    assert _call(lib, protos, name, P=0, W=64, H=64, tile_row_begin=begin, n_tile_rows=n) == NRC_ERR_INVALID


def test_workspace_bytes_of_a_valid_band(lib):
    whole = lib.nrc_gs_bin_hist_bytes(1000, 640, 840, 0)
    assert whole > 0
    for begin, n in ((0, 53), (0, 1), (52, 1), (10, 7)):
        assert lib.nrc_gs_bin_hist_bytes_band(1000, 640, 840, 0, begin, n) == whole      # the layout depends on the span capacity alone
    assert lib.nrc_gs_bin_hist_bytes_band(1000, 640, 840, 0, 0, 54) == NRC_ERR_INVALID
    assert lib.nrc_gs_bin_hist_bytes_band(1000, 640, 840, 5000, 3, 4) == lib.nrc_gs_bin_hist_bytes(1000, 640, 840, 5000) < whole


@pytest.mark.parametrize('gy', [53, 67])          # H = 840 and H = 1060
@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_tile_row_band_partitions_the_rows(gy, world):
    bands = [parallel.tile_row_band(gy, r, world) for r in range(world)]
    assert bands[0][0] == 0 and bands[-1][0] + bands[-1][1] == gy
    for (b0, n0), (b1, _) in zip(bands, bands[1:]):
        assert b0 + n0 == b1                                      # contiguous, in rank order
    sizes = [n for _, n in bands]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and sum(sizes) == gy
    assert bands == [(b, e - b) for b, e in (parallel.shard_range(gy, r, world) for r in range(world))]
    H = 16 * gy - 4                                               # a last tile row of 12 pixel rows
    rows = [parallel.band_pixel_rows(H, b) for b in bands]
    assert rows[0][0] == 0 and rows[-1][1] == H and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))


def test_tile_row_band_refuses_more_ranks_than_rows():
    """The stated rule for gy < world: a clear error (a band has at least one tile row)."""
    assert parallel.tile_row_band(3, 2, 3) == (2, 1)
    with pytest.raises(ValueError, match='3 tile rows cannot be split into 8 non-empty bands'):
        parallel.tile_row_band(3, 0, 8)
    with pytest.raises(ValueError):
        parallel.tile_row_band(53, 8, 8)


def test_tile_rows_are_validated_on_the_python_side():
    from nerficg_amd.diff_gaussian_rasterization import check_tile_rows
    assert check_tile_rows(None, 840) is None and check_tile_rows((0, 53), 840) == (0, 53) and check_tile_rows([52, 1], 840) == (52, 1)
    for bad in ((-1, 2), (0, 0), (50, 4), (53, 1)):
        with pytest.raises(ValueError, match='tile_rows'):
            check_tile_rows(bad, 840)


# ---------------------------------------------------------------------------------------------------- gloo ranks, fake per-band renderer
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, fn, ret):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    parallel.init_distributed('gloo')
    try:
        ret[rank] = fn(rank, world)
    finally:
        dist.destroy_process_group()


def _run(fn, world):
    ctx = mp.get_context('spawn')
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, fn, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(180)
            assert p.exitcode == 0
        return dict(ret)


H, W, P = 70, 24, 40          # gy = 5 tile rows, the last one 6 pixel rows high


def _fake_scene():
    g = torch.Generator().manual_seed(11)
    centre = torch.rand(P, generator=g) * H                       # every "Gaussian" covers the pixel rows within `reach` of its centre row
    reach = torch.rand(P, generator=g) * 12 + 1
    reach[::7] = 0.0                                              # some cover nothing at all
    colour = torch.rand(P, 3, generator=g)
    target = torch.rand(3, H, W, generator=g)
    return centre, reach, colour, target


def _fake_render(params, centre, reach, rows):
    """A stand-in for the per-band renderer, linear in `params` (P, 3): pixel row y of the image is sum_i w_i(y) params_i over the "Gaussians" that
    cover it.  `rows` = (y0, y1): only those rows are rendered, the rest is zero.  Returns (image, mask of the Gaussians that touch the rows)."""
    y = torch.arange(H, dtype=torch.float32)
    w = ((y[None] - centre[:, None]).abs() < reach[:, None]).float() * (1.0 + 0.1 * y[None])       # (P, H)
    inside = ((y >= rows[0]) & (y < rows[1])).float()
    w = w * inside[None]
    image = torch.einsum('ph,pc->ch', w, params)[:, :, None].expand(3, H, W) * torch.linspace(0.5, 1.5, W)[None, None]
    return image, w.sum(1) > 0


def _loss(image, target):
    return ((image - target) ** 2).sum() + image[:, 1:].mul(image[:, :-1]).sum()        # couples neighbouring pixel rows, like an SSIM window across a band edge


def _t_band_step(rank, world):
    centre, reach, colour, target = _fake_scene()
    gy = (H + 15) // 16
    band = parallel.tile_row_band(gy, rank, world)
    rows = parallel.band_pixel_rows(H, band)
    # single-process reference
    ref_p = colour.clone().requires_grad_(True)
    ref_img, _ = _fake_render(ref_p, centre, reach, (0, H))
    ref_img.retain_grad()
    _loss(ref_img, target).backward()
    # band-parallel: own band, gather, whole-frame loss, backward, summed sparse exchange
    p = torch.nn.Parameter(colour.clone())
    band_img, mask = _fake_render(p, centre, reach, rows)
    junk = band_img.detach().clone()
    junk[:, :rows[0]] = 7.0; junk[:, rows[1]:] = -7.0             # whatever a rank holds outside its own rows must not reach the frame
    band_in = band_img + (junk - band_img.detach())               # the band's rows (and gradient path) of band_img, junk values elsewhere
    band_in.retain_grad()
    full = parallel.gather_band_images(band_in)
    composed = bool(torch.equal(full.detach(), ref_img.detach()))
    _loss(full, target).backward()
    own_rows = bool(torch.equal(band_in.grad[:, rows[0]:rows[1]], ref_img.grad[:, rows[0]:rows[1]]))
    elsewhere_zero = bool((band_in.grad[:, :rows[0]] == 0).all() and (band_in.grad[:, rows[1]:] == 0).all())
    share = p.grad.clone()
    outside_mask_zero = bool((share[~mask] == 0).all())
    # dense all-reduce-sum of the shares = what the sparse exchange must produce
    dense = share.clone()
    dist.all_reduce(dense, op=dist.ReduceOp.SUM)
    union = mask.to(torch.uint8)
    dist.all_reduce(union, op=dist.ReduceOp.MAX)
    marker = 123.0
    p.grad[union == 0] = marker                                   # rows outside every mask: the exchange must not touch them
    ex = parallel.UnionRowExchange(P, p.device)
    ex.begin(mask)
    n_union = ex.finish([p], average=False)
    touched = union.bool()
    return dict(composed=composed, own_rows=own_rows, elsewhere_zero=elsewhere_zero, outside_mask_zero=outside_mask_zero,
                n_union=n_union, n_expected=int(touched.sum()), n_untouched=int((~touched).sum()),
                sparse_equals_dense=bool(torch.equal(p.grad[touched], dense[touched])),
                untouched_kept=bool((p.grad[~touched] == marker).all()),
                matches_single=float((p.grad[touched] - ref_p.grad[touched]).abs().max() / ref_p.grad.abs().max()),
                band=band)


@pytest.mark.parametrize('world', [2, 4])
def test_gather_and_summed_sparse_exchange_on_gloo_ranks(world):
    out = _run(_t_band_step, world)
    assert sorted(out) == list(range(world))
    assert [out[r]['band'] for r in range(world)] == [parallel.tile_row_band(5, r, world) for r in range(world)]
    for r in range(world):
        o = out[r]
        assert o['composed'], 'the gathered band rows are the whole frame, bit for bit'
        assert o['own_rows'] and o['elsewhere_zero'], 'the backward of the gather hands a rank its own rows of the image gradient and nothing else'
        assert o['outside_mask_zero'], 'a Gaussian outside the band mask has a zero share'
        assert o['n_union'] == o['n_expected'] > 0 and o['n_untouched'] > 0
        assert o['sparse_equals_dense'], 'summed sparse exchange == dense all-reduce-sum'
        assert o['untouched_kept'], 'rows outside every mask are not touched'
        assert o['matches_single'] <= 1e-5, 'after the exchange every rank holds the single-process gradient (f32 summation order only)'


def test_gather_is_the_identity_in_a_single_process():
    img = torch.rand(3, 40, 8, requires_grad=True)
    assert parallel.gather_band_images(img) is img
