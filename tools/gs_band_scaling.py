#!/usr/bin/env python3
"""tools/gs_band_scaling.py -- what ONE GPU's share of a band-parallel 3DGS frame costs: the synthetic 1 M-Gaussian scene (bench.build_gs_scene) at 1297x840 and
1600x1060, the whole frame and every band of parallel.tile_row_band for N = 2, 4, 8, forward and forward + backward, all on one GPU, one band after the other.

    python tools/gs_band_scaling.py [--out profiles/NAME.md]      device-event timing: warmed up, windows of >= --window seconds, median of --trials windows
    rocprofv3 --kernel-trace --stats ... -- python tools/gs_band_scaling.py --kernels whole|N [--size W H]
                                                                   the launches of --reps forward + backward frames (whole) or of every band of N in turn, for the
                                                                   per-kernel times (a separate run: nothing is timed here)

The figure reported per (size, N) is whole-frame time / slowest band's time -- the speed-up of the rasterizer calls if N GPUs ran one band each and nothing else
cost anything (no wire, no gather) -- next to the Amdahl bound from the per-kernel times of the committed whole-frame profile (profiles/*_gs_kernel_stats.csv):
preprocess, depth sort and the per-Gaussian backward run over all P on every rank; only binning and the two blend kernels shrink with the band."""
import argparse
import csv
import glob
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import bench  # noqa: E402
from nerficg_amd import parallel  # noqa: E402

SIZES = ((1297, 840), (1600, 1060))
SHRINKS = ('k_span_sweep', 'k_item_count', 'k_item_scan', 'k_item_scatter', 'k_render_bw', 'k_render')       # binning behind the clipped rectangles + the blends
REPLICATED = ('k_preprocess_bw', 'k_preprocess', 'k_depth_keys', 'k_radix_pass', 'k_zero_grads')


def frame_fn(gs, band, backward):
    t, rast = gs['tensors'], gs['rast']
    g = torch.ones(3, gs['h'], gs['w'], device=t['means3D'].device)
    kw = {} if band is None else {'tile_rows': band}

    def body():
        a = {k: v.detach().requires_grad_(backward) for k, v in t.items()}
        m2d = torch.zeros_like(a['means3D'], requires_grad=backward)
        color, _ = rast(means3D=a['means3D'], means2D=m2d, opacities=a['opacities'], shs=a['shs'], scales=a['scales'], rotations=a['rotations'], **kw)
        if backward:
            color.backward(g)
    return body


def timed_ms(body, window_s, trials):
    """Median and spread of `trials` windows; a window = enough back-to-back calls for `window_s` seconds between two device events."""
    for _ in range(3):
        body()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(); body(); stop.record(); stop.synchronize()
    reps = max(5, int(window_s * 1e3 / max(start.elapsed_time(stop), 1e-3)))
    out = []
    for _ in range(trials):
        start.record()
        for _ in range(reps):
            body()
        stop.record(); stop.synchronize()
        out.append(start.elapsed_time(stop) / reps)
    return statistics.median(out), min(out), max(out), reps


def amdahl_from_profile():
    """Per-kernel microseconds per frame of the newest committed whole-frame profile (1 M Gaussians, 1297x840, forward + backward) -> the bound for N bands."""
    files = sorted(glob.glob(str(ROOT / 'profiles' / 'r*_gs_kernel_stats.csv')))
    if not files:
        return None
    rows = list(csv.DictReader(open(files[-1])))
    shrink = repl = 0.0
    for r in rows:
        per_frame = float(r['AverageNs']) / 1e3 * (4 if 'k_radix_pass' in r['Name'] else 1)      # one launch per frame, four sort passes (k_item_scatter: one of its two forms)
        if 'k_item_scatter' in r['Name'] and int(r['Calls']) < max(int(q['Calls']) for q in rows if 'k_item_scatter' in q['Name']):
            continue
        if any(k + '(' in r['Name'] or k + '<' in r['Name'] for k in SHRINKS):
            shrink += per_frame
        elif any(k + '(' in r['Name'] or k + '<' in r['Name'] for k in REPLICATED):
            repl += per_frame
    return dict(file=Path(files[-1]).name, shrinking_us=round(shrink, 1), replicated_us=round(repl, 1),
                bound={n: round((shrink + repl) / (repl + shrink / n), 2) for n in (2, 4, 8)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', type=float, default=0.4)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--kernels', default=None, help="'whole' or a band count N: only launch (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument('--size', type=int, nargs=2, default=None)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sizes = (tuple(args.size),) if args.size else SIZES
    if args.kernels is not None:
        w, h = sizes[0]
        gs = bench.build_gs_scene(dev, 1_000_000, w=w, h=h)
        gy = (h + 15) // 16
        bands = [None] if args.kernels == 'whole' else [parallel.tile_row_band(gy, r, int(args.kernels)) for r in range(int(args.kernels))]
        for band in bands:
            body = frame_fn(gs, band, True)
            for _ in range(args.reps + 3):
                body()
        torch.cuda.synchronize()
        print(json.dumps({'kernels': args.kernels, 'size': [w, h], 'frames_per_band': args.reps + 3, 'bands': len(bands)}))
        return
    lines = ['# One 3DGS frame as tile-row bands: what one GPU\'s band costs (1 M Gaussians, one MI355X, one band after the other)', '',
             f'`python tools/gs_band_scaling.py`: device events around windows of >= {args.window} s of back-to-back calls (3 warm-up calls per shape), median of {args.trials} windows',
             '(min .. max in brackets).  ratio = whole-frame time / slowest band: the speed-up of the rasterizer calls alone with one band per GPU; wire, gather and',
             'multi-GPU scaling are NOT measured here.', '']
    result = {}
    for w, h in sizes:
        gs = bench.build_gs_scene(dev, 1_000_000, w=w, h=h)
        gy = (h + 15) // 16
        for backward in (False, True):
            mode = 'forward + backward' if backward else 'forward'
            whole = timed_ms(frame_fn(gs, None, backward), args.window, args.trials)
            lines += [f'## {w}x{h}, {mode}', '', f'whole frame: {whole[0]:.3f} ms [{whole[1]:.3f} .. {whole[2]:.3f}], {whole[3]} calls per window', '',
                      '| N | band times, ms (rank 0 .. N-1) | slowest | whole / slowest |', '|---|---|---|---|']
            for n in (2, 4, 8):
                times = [timed_ms(frame_fn(gs, parallel.tile_row_band(gy, r, n), backward), args.window, args.trials)[0] for r in range(n)]
                lines.append(f'| {n} | {" ".join(f"{t:.3f}" for t in times)} | {max(times):.3f} | {whole[0] / max(times):.2f} |')
                result[f'{w}x{h} {mode} N={n}'] = dict(whole_ms=round(whole[0], 4), band_ms=[round(t, 4) for t in times], ratio=round(whole[0] / max(times), 3))
            lines.append('')
        del gs
        torch.cuda.empty_cache()
    am = amdahl_from_profile()
    if am is not None:
        lines += ['## Amdahl bound from the whole-frame kernel profile', '',
                  f'`profiles/{am["file"]}` (1 M Gaussians, 1297x840, forward + backward, per frame): {am["shrinking_us"]} us in the kernels that shrink with the band',
                  f'({", ".join(SHRINKS)}), {am["replicated_us"]} us in the kernels every rank repeats over all P ({", ".join(REPLICATED)}).',
                  'Bound on whole / band for equal shares: ' + ', '.join(f'N = {n}: {v}' for n, v in am['bound'].items()) + ' (kernel time only: no launch gaps, no host).', '']
    text = '\n'.join(lines)
    print(text)
    print('RESULT ' + json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
