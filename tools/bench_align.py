"""Images/s of alignment: LandmarkDetector.align (u8 photos, one face box each; detect()'s program plus the coefficient launch, then
one warp launch that samples the packed photos) against LandmarkDetector.keypoints and LandmarkDetector.detect on the same u8 photos
and boxes, at S = So = 128, bf16 and B in {32, 128, 256}: the three models at K = 10 and the thin-plate spline at K = 64; writes the
table to profiles/align_bench.txt.

Columns per batch B (median over windows of HIP-event-timed calls on the caller's stream, after warm-up), as a user calls them:
  detect      detector.detect(photos): pack + copy of the u8 pixels, resize, graph replay, result copy
  keypoints   detector.keypoints(photos, regressor, boxes)
  sim/aff/tps detector.align(photos, template, boxes, model): the same staging as keypoints, the graph with imm_align_coeffs, the warp
  host        what align() replaces: detect() on the photos, the landmarks copied to the host, a numpy similarity fit per photo and
              a numpy bilinear resample of the u8 photo through it (wall clock, median of 3)
The photos are 218 x 178 (the CelebA aligned size) with one box each, part of it outside the photo.
Usage: python tools/bench_align.py [--batches 32 128 256] [--windows 7] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imm_amd.alignment import LandmarkTemplate             # noqa: E402
from imm_amd.keypoints import LandmarkRegressor, box_geometry, check_boxes   # noqa: E402
from imm_amd.models.imm_model import IMMModel             # noqa: E402
from bench_detect import model_config, timed_ms           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'align_bench.txt')


def grid_template(K, S, rng):
    n = int(np.ceil(np.sqrt(K)))
    cells = rng.permutation(n * n)[:K]
    yx = np.stack([cells // n, cells % n], 1).astype(np.float64)
    return LandmarkTemplate(-0.7 + (yx + 0.5 + rng.uniform(-0.3, 0.3, size=(K, 2))) * (1.4 / n), S)


def host_align(det, photos, boxes, template, S):
    """The host detour: landmarks to the host, a numpy similarity fit and a numpy bilinear resample per photo."""
    mu = det.landmarks(photos, boxes=boxes).cpu().numpy().astype(np.float64)
    geom = box_geometry(check_boxes(boxes, len(photos)), S).astype(np.float64)
    coef = template.fit(mu, 'similarity')
    g = -1.0 + 2.0 * np.arange(S) / S
    qy, qx = np.meshgrid(g, g, indexing='ij')
    out = np.zeros((len(photos), S, S, 3), np.float32)
    for b, im in enumerate(photos):
        h, w = im.shape[:2]
        vy = coef[b, 0, 0] + qy * coef[b, 1, 0] + qx * coef[b, 2, 0]
        vx = coef[b, 0, 1] + qy * coef[b, 1, 1] + qx * coef[b, 2, 1]
        sy, sx = geom[b, 0] + (vy + 1) / 2 * S * geom[b, 2], geom[b, 1] + (vx + 1) / 2 * S * geom[b, 3]
        y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
        wy, wx = (sy - y0)[..., None], (sx - x0)[..., None]

        def tap(r, c):
            ok = (r >= 0) & (r < h) & (c >= 0) & (c < w)
            return np.where(ok[..., None], im[np.clip(r, 0, h - 1), np.clip(c, 0, w - 1)].astype(np.float32), 0.0)
        top = tap(y0, x0) * (1 - wx) + tap(y0, x0 + 1) * wx
        bot = tap(y0 + 1, x0) * (1 - wx) + tap(y0 + 1, x0 + 1) * wx
        out[b] = top * (1 - wy) + bot * wy
    return out


def main(args):
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    S, M = 128, 5
    rng = np.random.RandomState(0)
    props = torch.cuda.get_device_properties(0)
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = So %d, bf16; u8 photos 218 x 178, one box (y0, x0, y1, x1) = (-8, 10, 170, 168) each; ms per call (median of %d '
             'windows x %d calls); host = detect + numpy similarity fit + numpy resample (wall clock)' % (S, args.windows, args.reps),
             '%3s %5s %10s %10s %10s %10s %10s %10s %12s' % ('K', 'B', 'detect', 'keypoints', 'similarity', 'affine', 'tps', 'host',
                                                           'tps - detect')]
    rows = []
    for K, models in ((10, ('similarity', 'affine', 'tps')), (64, ('tps',))):
        mu = rng.uniform(-0.8, 0.8, size=(160, K, 2)).astype(np.float32)
        pts = ((mu + 1) / 2.0 * S).reshape(160, -1) @ (rng.standard_normal((2 * K, 2 * M)) * 0.3) + 30.0
        reg = LandmarkRegressor.fit({'gauss_yx': mu, 'future_landmarks': pts.reshape(160, M, 2)}, [S, S], True)
        tpl = grid_template(K, S, rng)
        for B in args.batches:
            photos = [rng.randint(0, 256, size=(218, 178, 3)).astype(np.uint8) for _ in range(B)]
            boxes = [(i, -8, 10, 170, 168) for i in range(B)]
            model = IMMModel(model_config(K), dtype=torch.bfloat16, device=dev)
            x = torch.zeros(B, S, S, 3, device=dev)
            model.build({'image': x, 'future_image': x}, training_pl=False, build_loss=False)      # the batch-B engine (variables)
            det = model.landmark_detector(S, max_batch=B)
            row = {'n_maps': K, 'batch': B}
            row['detect_ms'] = timed_ms(lambda: det.detect(photos), args.reps, args.windows, args.warmup)
            row['keypoints_ms'] = timed_ms(lambda: det.keypoints(photos, reg, boxes=boxes), args.reps, args.windows, args.warmup)
            for m in models:
                row[m + '_ms'] = timed_ms(lambda: det.align(photos, tpl, boxes=boxes, model=m), args.reps, args.windows, args.warmup)
            if K == 10 and args.host:
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host_align(det, photos, boxes, tpl, S)
                    ts.append((time.perf_counter() - t0) * 1e3)
                row['host_ms'] = float(np.median(ts))
            rows.append(row)
            f = lambda k: ('%10.3f' % row[k]) if k in row else '%10s' % '-'
            lines.append('%3d %5d %s %s %s %s %s %s %12.3f' % (K, B, f('detect_ms'), f('keypoints_ms'), f('similarity_ms'), f('affine_ms'),
                                                               f('tps_ms'), f('host_ms'), row['tps_ms'] - row['detect_ms']))
            print(lines[-1], flush=True)
            del det, model
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'image_size': S, 'dtype': 'bf16', 'rows': rows}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, nargs='+', default=[32, 128, 256])
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--no-host', dest='host', action='store_false', help='skip the numpy host detour')
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
