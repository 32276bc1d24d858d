"""Milliseconds per call of LandmarkDetector.redact (u8 photos and face boxes in, the same photos out with the faces pixelated or
smoothed) in both modes, with and without the landmark-hull mask, with LandmarkDetector.warp on the same photos and boxes alongside for
orientation, and frames/s of LandmarkDetector.redact_clip, at S = 128, bf16, K = 10, blocks = 8 and one bucket of B = 64 rows.  Writes
the table to profiles/redact_bench.txt and prints one JSON line.  A recording tool: it has no pass/fail threshold.

  pixelate, smooth            detector.redact(photos, boxes, mode=...): pack + copy of the u8 photos, a device copy to paste into, one
                              imm_redact_cells_u8 and one imm_redact_u8 launch; no pose program
  pixelate+hull, smooth+hull  the same with mask='hull': the box crop, the pose program's graph and one imm_hull_fit launch in front
  warp                        detector.warp(photos, poses, boxes) on the same rows: the crop, the pose program, imm_warp_fit, imm_warp_u8
  pack                        the part of each that comes before any kernel (inference.pack_u8 and a clone)
  cells, u8                   imm_redact_cells_u8 and imm_redact_u8 (pixelate, no mask) alone, on the buffers of one redact() call
  clip                        detector.redact_clip over T frames of about 512 x 384 with two faces, uploads included, in wall time
The calls are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of
the mean per-call time); the clip in wall time around a synchronised call.  The photos are about 512 x 384 with one box of about
250 x 250 each.  The model has random weights: its landmarks sit in a small cloud, so the hull of the masked calls is small; the
masked calls differ from the plain ones by the pose program and the fit, which do not depend on the hull's size.
Usage: python tools/bench_redact.py [--batch 64] [--windows 7] [--reps 10] [--frames 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUT = os.path.join(ROOT, 'profiles', 'redact_bench.txt')
S, K, BLOCKS = 128, 10, 8


def main(args):
    import torch
    from bench_detect import timed_ms
    from bench_repose import make_generator, scene
    from bench_warp import grid_poses
    from imm_amd import ops
    from imm_amd.generation import compose_inv_ramp, compose_links
    from imm_amd.inference import pack_u8, plan_buckets
    from imm_amd.keypoints import check_boxes
    B, T = args.batch, args.frames
    photos, boxes, _lm = scene(B)
    _model, gen = make_generator(B)
    det = gen.detector
    assert len(plan_buckets(B, B)) == 1
    props = torch.cuda.get_device_properties(0)
    poses = torch.from_numpy(grid_poses(B)).cuda()
    rows = check_boxes(boxes, B)
    out = det.redact(photos, boxes)
    torch.cuda.synchronize()
    changed = sum(int((o.cpu().numpy() != p).any(axis=2).sum()) for o, p in zip(out, photos))
    # the two kernels alone, on buffers like those of that call
    src, offs_d, hw_d, boxes_d = pack_u8(photos, 'cuda:0', rows)
    canvas = src.clone()
    links_d = ops.to_device_pinned(compose_links(rows), 'cuda:0')
    ramp_d = ops.to_device_pinned(compose_inv_ramp(rows, 0.0), 'cuda:0')
    area = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max())
    cells = torch.empty(B, BLOCKS * BLOCKS * 3, dtype=torch.uint8, device='cuda:0')
    fns = {'pixelate': lambda: det.redact(photos, boxes, mode='pixelate'), 'smooth': lambda: det.redact(photos, boxes, mode='smooth'),
           'pixelate+hull': lambda: det.redact(photos, boxes, mode='pixelate', mask='hull'),
           'smooth+hull': lambda: det.redact(photos, boxes, mode='smooth', mask='hull'),
           'warp': lambda: det.warp(photos, poses, boxes),
           'pack': lambda: pack_u8(photos, 'cuda:0', rows)[0].clone(),
           'cells': lambda: ops.redact_cells_u8(src, offs_d, hw_d, boxes_d, BLOCKS, cells),
           'u8': lambda: ops.redact_u8(canvas, offs_d, hw_d, boxes_d, links_d, ramp_d, cells, BLOCKS, 0, area)}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    # the clip: one photo moved a few pixels a frame, two faces, in wall time with the uploads
    rng = np.random.RandomState(5)
    big = rng.randint(0, 256, size=(512 + 2 * T, 384 + 2 * T, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(big[t:t + 512, 2 * T - 2 * t:2 * T - 2 * t + 384]) for t in range(T)]
    faces = [(60, 40, 300, 280), (250, 120, 490, 360)]
    clip_s = {}
    for name, kw in (('clip', {}), ('clip+hull', dict(mask='hull'))):
        det.redact_clip(frames[:2], faces, **kw)
        torch.cuda.synchronize()
        secs = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            det.redact_clip(frames, faces, **kw)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        clip_s[name] = float(np.median(secs))
    px = 0
    for i, y0, x0, y1, x1 in boxes:
        h, w = photos[i].shape[:2]
        px += max(0, min(y1, h) - max(y0, 0)) * max(0, min(x1, w) - max(x0, 0))
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, blocks = %d, feather 0, bf16, one bucket of B = %d rows; %d u8 photos of about 512 x 384 (%.1f MB packed), one '
             'box of about 250 x 250 each (%.2f M box pixels in all); ms per call: median (min .. max) of %d alternated windows x %d calls' % (
                 S, K, BLOCKS, B, B, sum(p.size for p in photos) / 1e6, px / 1e6, args.windows, args.reps),
             'photo pixels the default redaction changed: %d' % changed,
             '%-14s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in fns:
        lines.append('%-14s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k],
                                                 '-' if k in ('pack', 'cells', 'u8') else '%.0f' % (B / med[k] * 1e3)))
    lines.append('imm_redact_u8: %.1f ps per box pixel (%.1f GB/s of photo bytes read and written); imm_redact_cells_u8: %.1f ps per box pixel' % (
        med['u8'] * 1e9 / px, 6 * px / med['u8'] / 1e6, med['cells'] * 1e9 / px))
    for name, s in clip_s.items():
        lines.append('%-14s %d frames of 512 x 384, 2 faces: %.1f ms a call, %.0f frames/s (wall time, uploads included)' % (name, T, s * 1e3, T / s))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'batch': B, 'blocks': BLOCKS, 'pixelate_ms': med['pixelate'], 'smooth_ms': med['smooth'],
                      'pixelate_hull_ms': med['pixelate+hull'], 'smooth_hull_ms': med['smooth+hull'], 'warp_ms': med['warp'],
                      'pack_ms': med['pack'], 'cells_ms': med['cells'], 'u8_ms': med['u8'], 'clip_frames': T,
                      'clip_fps': T / clip_s['clip'], 'clip_hull_fps': T / clip_s['clip+hull']}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--frames', type=int, default=32)
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
