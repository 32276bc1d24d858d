"""Images/s of keypoints: LandmarkDetector.keypoints (u8 photos, one face box each, cut and resized on the GPU, the pose head's
keypoint epilogue) against LandmarkDetector.detect on the same u8 photos (resized whole), at S = 128, K = 10, bf16 and B in
{32, 128, 256}; writes the table to profiles/keypoints_bench.txt.

Columns per batch B (median over windows of HIP-event-timed calls on the caller's stream, after warm-up), as a user calls them:
  detect      detector.detect(photos): pack + copy of the u8 pixels, resize, graph replay, result copy
  keypoints   detector.keypoints(photos, regressor, boxes): the same plus the box rows, the geometry rows and the regressor's W / b
The photos are 218 x 178 (the CelebA aligned size) with one box each, part of it outside the photo.
Usage: python tools/bench_keypoints.py [--batches 32 128 256] [--windows 7] [--reps 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imm_amd.keypoints import LandmarkRegressor           # noqa: E402
from imm_amd.models.imm_model import IMMModel             # noqa: E402
from bench_detect import model_config, timed_ms           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'keypoints_bench.txt')


def main(args):
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    S, K, M = 128, 10, 5
    rng = np.random.RandomState(0)
    mu = rng.uniform(-0.8, 0.8, size=(64, K, 2)).astype(np.float32)
    pts = ((mu + 1) / 2.0 * S).reshape(64, -1) @ (rng.standard_normal((2 * K, 2 * M)) * 0.3) + 30.0
    reg = LandmarkRegressor.fit({'gauss_yx': mu, 'future_landmarks': pts.reshape(64, M, 2)}, [S, S], True)
    props = torch.cuda.get_device_properties(0)
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S %d, K %d, M %d, bf16; u8 photos 218 x 178, one box (y0, x0, y1, x1) = (-8, 10, 170, 168) each; ms per call (median '
             'of %d windows x %d calls)' % (S, K, M, args.windows, args.reps),
             '%5s %12s %12s %14s %14s %10s' % ('B', 'detect ms', 'keypts ms', 'detect img/s', 'keypts img/s', 'ratio')]
    rows = []
    for B in args.batches:
        photos = [rng.randint(0, 256, size=(218, 178, 3)).astype(np.uint8) for _ in range(B)]
        boxes = [(i, -8, 10, 170, 168) for i in range(B)]
        model = IMMModel(model_config(K), dtype=torch.bfloat16, device=dev)
        x = torch.zeros(B, S, S, 3, device=dev)
        model.build({'image': x, 'future_image': x}, training_pl=False, build_loss=False)      # the batch-B engine (variables)
        det = model.landmark_detector(S, max_batch=B)
        t_det = timed_ms(lambda: det.detect(photos), args.reps, args.windows, args.warmup)
        t_kp = timed_ms(lambda: det.keypoints(photos, reg, boxes=boxes), args.reps, args.windows, args.warmup)
        row = {'batch': B, 'detect_ms': t_det, 'keypoints_ms': t_kp, 'detect_images_per_s': B / t_det * 1e3,
               'keypoints_images_per_s': B / t_kp * 1e3, 'keypoints_over_detect': t_kp / t_det}
        rows.append(row)
        lines.append('%5d %12.3f %12.3f %14.0f %14.0f %10.2f' % (B, t_det, t_kp, row['detect_images_per_s'],
                                                               row['keypoints_images_per_s'], row['keypoints_over_detect']))
        print(lines[-1], flush=True)
        del det, model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'image_size': S, 'n_maps': K, 'points': M, 'dtype': 'bf16', 'rows': rows}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, nargs='+', default=[32, 128, 256])
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
