"""Milliseconds per call of LandmarkDetector.annotate (u8 photos and face boxes in, the same photos out with landmarks, boxes and hulls
drawn into them), with LandmarkDetector.redact on the same photos and boxes alongside as the yardstick, and frames/s of
LandmarkDetector.annotate_clip beside redact_clip, at S = 128, bf16, K = 10 and one bucket of B = 64 rows.  Writes the table to
profiles/annotate_bench.txt and prints one JSON line.  A recording tool: it has no pass/fail threshold.

  points+box, +hull           detector.annotate(photos, boxes) and with draw=('points', 'box', 'hull'): pack + copy of the u8 photos, a
                              device copy to draw into, the box crop and the pose program's graph, imm_annotate_points (imm_hull_fit),
                              one imm_annotate_u8 launch
  redact, redact+hull         detector.redact(photos, boxes) and with mask='hull' on the same rows (tools/bench_redact.py's pixelate rows)
  pack                        the part of each that comes before any kernel (inference.pack_u8 and a clone)
  annotate_u8 (+hull)         imm_annotate_u8 alone on the buffers of one annotate() call, points + box and with the hull's lines
  redact_u8                   imm_redact_u8 (pixelate, no mask) alone on the same rows
  clip                        detector.annotate_clip over T frames of about 512 x 384 with two faces at trail = 0 and trail = 8, and
                              detector.redact_clip on the same frames, uploads included, in wall time
The calls are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of
the mean per-call time); the clips in wall time around a synchronised call.  The photos are about 512 x 384 with one box of about
250 x 250 each.  The model has random weights: its landmarks sit in a small cloud, so the markers overlap and the hull is small; the
loop over the marks, which every pixel of an extent runs, does not depend on where they lie.
Usage: python tools/bench_annotate.py [--batch 64] [--windows 7] [--reps 10] [--frames 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUT = os.path.join(ROOT, 'profiles', 'annotate_bench.txt')
S, K, BLOCKS = 128, 10, 8


def main(args):
    import torch
    from bench_detect import timed_ms
    from bench_repose import make_generator, scene
    from imm_amd import annotation as AN
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
    rows = check_boxes(boxes, B)
    hull_draw = ('points', 'box', 'hull')
    (out, tr) = det.annotate(photos, boxes, draw=hull_draw, return_transform=True)
    torch.cuda.synchronize()
    changed = sum(int((o.cpu().numpy() != p).any(axis=2).sum()) for o, p in zip(out, photos))
    # the kernels alone, on buffers like those of that call
    dev = 'cuda:0'
    src, offs_d, hw_d, boxes_d = pack_u8(photos, dev, rows)
    canvas = src.clone()
    links_d = ops.to_device_pinned(compose_links(rows), dev)
    ramp_d = ops.to_device_pinned(compose_inv_ramp(rows, 0.0), dev)
    pad = AN.default_pad(2.5)
    area, ext = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max()), AN.grid_pixels(rows, pad)
    cells = torch.empty(B, BLOCKS * BLOCKS * 3, dtype=torch.uint8, device=dev)
    ops.redact_cells_u8(src, offs_d, hw_d, boxes_d, BLOCKS, cells)
    marks = tr.points.reshape(1, B, K, 2).contiguous()
    edges = tr.hull_edges
    pal, gs, ms_d = (ops.to_device_pinned(a, dev) for a in (AN.STATUS_PALETTE, AN.group_styles(2.5, 1, 1.0), AN.mark_styles(K)))
    fns = {'points+box': lambda: det.annotate(photos, boxes), 'points+box+hull': lambda: det.annotate(photos, boxes, draw=hull_draw),
           'redact': lambda: det.redact(photos, boxes), 'redact+hull': lambda: det.redact(photos, boxes, mask='hull'),
           'pack': lambda: pack_u8(photos, dev, rows)[0].clone(),
           'annotate_u8': lambda: ops.annotate_u8(canvas, offs_d, hw_d, boxes_d, links_d, pal, 3, 1, pad, 1, ext, marks=marks, group_style=gs,
                                                  mark_style=ms_d),
           'annotate_u8+hull': lambda: ops.annotate_u8(canvas, offs_d, hw_d, boxes_d, links_d, pal, 7, 1, pad, 1, ext, marks=marks,
                                                       group_style=gs, mark_style=ms_d, edges=edges),
           'redact_u8': lambda: ops.redact_u8(canvas, offs_d, hw_d, boxes_d, links_d, ramp_d, cells, BLOCKS, 0, area)}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    # the clips: one photo moved a few pixels a frame, two faces, in wall time with the uploads
    rng = np.random.RandomState(5)
    big = rng.randint(0, 256, size=(512 + 2 * T, 384 + 2 * T, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(big[t:t + 512, 2 * T - 2 * t:2 * T - 2 * t + 384]) for t in range(T)]
    faces = [(60, 40, 300, 280), (250, 120, 490, 360)]
    clips = {'annotate_clip trail=0': lambda f: det.annotate_clip(f, faces, trail=0),
             'annotate_clip trail=8': lambda f: det.annotate_clip(f, faces, trail=8),
             'redact_clip': lambda f: det.redact_clip(f, faces)}
    clip_s = {k: [] for k in clips}
    for k, fn in clips.items():
        fn(frames[:2])
        torch.cuda.synchronize()
    for _ in range(args.windows):                                   # alternated as well
        for k, fn in clips.items():
            t0 = time.perf_counter()
            fn(frames)
            torch.cuda.synchronize()
            clip_s[k].append(time.perf_counter() - t0)
    clip_med = {k: float(np.median(v)) for k, v in clip_s.items()}
    px = 0
    for i, y0, x0, y1, x1 in boxes:
        h, w = photos[i].shape[:2]
        px += max(0, min(y1 + pad, h) - max(y0 - pad, 0)) * max(0, min(x1 + pad, w) - max(x0 - pad, 0))
    kernels = ('pack', 'annotate_u8', 'annotate_u8+hull', 'redact_u8')
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, size 2.5, thickness 1, pad %d, bf16, one bucket of B = %d rows; %d u8 photos of about 512 x 384 (%.1f MB packed), '
             'one box of about 250 x 250 each (%.2f M extent pixels in all); ms per call: median (min .. max) of %d alternated windows x %d '
             'calls; redact at blocks = %d' % (S, K, pad, B, B, sum(p.size for p in photos) / 1e6, px / 1e6, args.windows, args.reps, BLOCKS),
             'photo pixels annotate(points, box, hull) changed: %d' % changed,
             '%-18s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in fns:
        lines.append('%-18s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '-' if k in kernels else '%.0f' % (B / med[k] * 1e3)))
    lines.append('imm_annotate_u8: %.1f ps per extent pixel (%.1f GB/s of photo bytes read and written), %.1f times imm_redact_u8 on the same rows; '
                 'with the hull %.1f ps, %.1f times' % (med['annotate_u8'] * 1e9 / px, 6 * px / med['annotate_u8'] / 1e6,
                                                         med['annotate_u8'] / med['redact_u8'], med['annotate_u8+hull'] * 1e9 / px,
                                                         med['annotate_u8+hull'] / med['redact_u8']))
    for name, s in clip_med.items():
        lines.append('%-22s %d frames of 512 x 384, 2 faces: %.1f ms a call, %.0f frames/s (wall time, uploads included)' % (name, T, s * 1e3, T / s))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'batch': B, 'annotate_ms': med['points+box'], 'annotate_hull_ms': med['points+box+hull'], 'redact_ms': med['redact'],
                      'redact_hull_ms': med['redact+hull'], 'pack_ms': med['pack'], 'annotate_u8_ms': med['annotate_u8'],
                      'annotate_u8_hull_ms': med['annotate_u8+hull'], 'redact_u8_ms': med['redact_u8'], 'clip_frames': T,
                      'annotate_clip_fps': T / clip_med['annotate_clip trail=0'], 'annotate_clip_trail8_fps': T / clip_med['annotate_clip trail=8'],
                      'redact_clip_fps': T / clip_med['redact_clip']}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--frames', type=int, default=32)
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
