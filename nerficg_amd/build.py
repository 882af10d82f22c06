"""nerficg_amd/build.py -- compiles csrc/*.hip for gfx950 into nerficg_amd/lib/libnerficg_hip.so (in-tree).

hipcc cross-compiles without a GPU, so this runs in the build container as well as on the MI355X box.
Usage: python -m nerficg_amd.build [--force]
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / 'csrc'
LIBDIR = PKG / 'lib'
LIB = LIBDIR / 'libnerficg_hip.so'
OBJDIR = LIBDIR / 'obj'
ARCH = 'gfx950'

COMMON_FLAGS = ['-O3', '-fPIC', f'--offload-arch={ARCH}', '-std=c++17', '-Wall', '-Wno-unused-function',
                '-Wno-unused-result', '-Wno-unused-value', '-fno-gpu-rdc', '-DNDEBUG']
# The translation units that include csrc/gs_blend.h get ONE flag list: the feature and contribution passes recompute the colour pass's alpha with the
# header's statements and must get the same bits (weight_max is w = alpha T itself).
#   no FMA contraction: see below
#   no SLP vectoriser: it packs the blend arithmetic of two list entries into v_pk_* and pays in v_mov (the blend states its own pairs: blend_power)
#   no atomic optimizer: it rewrites the one-lane LDS atomics of k_render_bw, and the per-row LDS float atomics of the two other passes, into
#   15-instruction wave-reduction loops
GS_BLEND_FLAGS = ['-ffp-contract=off', '-fno-slp-vectorize', '-mllvm', '-amdgpu-atomic-optimizer-strategy=None']
# translation units whose f32 arithmetic decides integer indices: no FMA contraction (bit-exact vs oracle/)
PER_FILE_FLAGS = {
    'ngp_march.hip': ['-ffp-contract=off'],
    'adam.hip': ['-ffp-contract=off'],
    'adam_rows.hip': ['-ffp-contract=off'],    # the masked step includes adam_math.h: the same bits as adam.hip's dense step on every visible row
    'knn.hip': ['-ffp-contract=off'],
    'gs_densify.hip': ['-ffp-contract=off'],   # thresholds decide the row list: same f32 sequence as oracle/gs_densify.py   # squared distances decide the neighbour set: same f32 sequence as oracle/knn_oracle.c
  # HBM-bound anyway; keeps the update bit-identical to oracle/adam_oracle.c
    'gs_raster.hip': GS_BLEND_FLAGS,
    'gs_features.hip': GS_BLEND_FLAGS,
    'gs_contrib.hip': GS_BLEND_FLAGS,
    # no SLP vectoriser either: packed f32 VALU next to MFMAs is priced above its issue slot on this chip (MI355X_MICROARCH.md), and the packing
    # costs v_mov: k_nwie_bwd 2 641 -> 2 451 vector instructions, k_gb_split 3 015 -> 2 853; the fused training iteration -1 %, the image path unchanged
    'ngp_net.hip': ['-fno-slp-vectorize'],
    # no FMA contraction: sign(lap) and the exact zeros of flat depth / equal neighbouring pixels are decided by the written f32 sequence, the one the tests'
    # error budget counts rounding by rounding; the launches are bound by memory and launch latency, so the contraction would buy nothing.  No fast-math
    # (COMMON_FLAGS has none): expf / logf / the divisions are the accurate ones the budget assumes.
    'map_losses.hip': ['-ffp-contract=off'],
    # no FMA contraction: the f32 sequence of the two input-gradient kernels is the one tests/input_grad_ref.py counts rounding by rounding (the
    # grid kernel waits for its gathers, the SH kernel for its rows: a fused multiply-add would buy nothing)
    'ngp_input_grad.hip': ['-ffp-contract=off'],
    # no FMA contraction: the noise kernel's f32 sequence is the one tests/gs_mcmc_ref.py counts rounding by rounding, and its two load shapes
    # (16-byte words, single floats) must give a row the same bits; the kernels wait for memory, or run every 100 iterations
    'gs_mcmc.hip': ['-ffp-contract=off'],
    # no SLP vectoriser, for the reason given for ngp_net.hip: the accumulator -> operand conversions sit between MFMAs (the packed fp16 max / min are written out)
    'nerf_net.hip': ['-fno-slp-vectorize'],
    'nerf_grad.hip': ['-fno-slp-vectorize'],   # the backward of the same block: masks and conversions between MFMAs
    # no FMA contraction: sampling and resampling are compared bit for bit with the numpy restatement of their f32 sequence (tests/nerf_rays_ref.py), and the
    # compositing budgets count that sequence rounding by rounding; the kernels stream a few dozen bytes per sample, a fused multiply-add would buy nothing
    'nerf_rays.hip': ['-ffp-contract=off'],
    # the input gradient of the same block: the same matrix pipeline (no SLP vectoriser, as for nerf_net.hip); its f32 encoding backward is written in
    # explicit single-rounding operations, so the contraction setting has nothing to decide
    'nerf_input_grad.hip': ['-fno-slp-vectorize'],
    # no FMA contraction: the written f32 sequence of the slice, its two gradients and the TV stencil is what the budget of tests/bilateral_grid_ref.py counts,
    # rounding by rounding, and the host evaluates the kernels' own cell function to size the tile windows: both sides must round alike.  The kernels move
    # 24 to 36 bytes per pixel and wait for them; a fused multiply-add would buy nothing
    'bilateral_grid.hip': ['-ffp-contract=off'],
}


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if cand and (Path(cand).exists() or cand == 'hipcc'):
            return cand
    raise RuntimeError('hipcc not found')


def _digest(paths: list[Path], extra: str) -> str:
    h = hashlib.sha256(extra.encode())
    for p in sorted(paths):
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> Path:
    sources = sorted(CSRC.glob('*.hip'))
    headers = sorted(CSRC.glob('*.h')) + sorted((PKG.parent / 'include').glob('*.h'))
    if not sources:
        raise RuntimeError(f'no .hip sources in {CSRC}')
    OBJDIR.mkdir(parents=True, exist_ok=True)
    hipcc = _hipcc()
    hdr_digest = _digest(headers, ' '.join(COMMON_FLAGS))

    def compile_one(src: Path) -> tuple[Path, bool]:
        flags = COMMON_FLAGS + PER_FILE_FLAGS.get(src.name, [])
        obj = OBJDIR / (src.stem + '.o')
        stamp = OBJDIR / (src.stem + '.sha')
        digest = _digest([src], hdr_digest + ' '.join(flags))
        if not force and obj.exists() and stamp.exists() and stamp.read_text() == digest:
            return obj, False
        cmd = [hipcc, *flags, '-c', str(src), '-o', str(obj)]
        if verbose:
            print('[build]', ' '.join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError(f'hipcc failed on {src.name}')
        if r.stderr.strip() and verbose:
            sys.stderr.write(r.stderr)
        stamp.write_text(digest)
        return obj, True

    with ThreadPoolExecutor(max_workers=min(4, len(sources))) as ex:
        results = list(ex.map(compile_one, sources))
    objs = [o for o, _ in results]
    if force or any(changed for _, changed in results) or not LIB.exists():
        cmd = [hipcc, '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', str(LIB), *map(str, objs)]
        if verbose:
            print('[build]', ' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
