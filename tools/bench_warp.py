"""Faces/s of LandmarkDetector.warp (u8 photos and face boxes in, the same photos out with the faces re-posed from their OWN pixels by
a thin-plate spline per face) with ImageGenerator.repose on the same photos, boxes and poses alongside for orientation (it renders
every face at 128 x 128 and pastes the resampled render back), at S = 128, bf16, K = 10, the default 2 anchors per side (M = 18 control
points) and one bucket of B = 64 rows.  Writes the table to profiles/warp_bench.txt.

  warp     detector.warp(photos, poses, boxes): pack + copy of the u8 photos, a device copy to warp into, the box crop, the pose
           program's graph, one imm_warp_fit and one imm_warp_u8 launch
  repose   gen.repose(photos, poses, boxes): the same packing and crop, the appearance and render graphs, one imm_compose_u8 launch
  pack     the part of either that comes before any kernel: the photos packed on the host, copied to the device and copied once more
           there (inference.pack_u8 and a clone)
  fit, u8  imm_warp_fit and imm_warp_u8 alone, on the buffers of one warp() call
All are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of the mean
per-call time).  The photos are about 512 x 384 (sizes vary by a few pixels) with one box of about 250 x 250 each; the poses lie on a
jittered grid, as the control points of a trained model's landmarks would (an untrained model's own landmarks, which the warp carries
them back to, sit in a small cloud: the motion is large, which costs the kernel nothing).
Usage: python tools/bench_warp.py [--batch 64] [--windows 7] [--reps 10] [--anchors 2]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUT = os.path.join(ROOT, 'profiles', 'warp_bench.txt')
S, K = 128, 10


def grid_poses(B, seed=1):
    """f32 [B, K, 2]: K cells of a 4 x 4 grid over [-0.8, 0.8]^2 per row, each point jittered by a quarter cell either way."""
    rng = np.random.RandomState(seed)
    g, cell = 4, 0.4
    out = np.zeros((B, K, 2))
    for b in range(B):
        pick = rng.permutation(g * g)[:K]
        out[b] = np.stack([pick // g, pick % g], axis=1) * cell - 0.8 + cell / 2 + rng.uniform(-cell / 4, cell / 4, size=(K, 2))
    return out.astype(np.float32)


def main(args):
    import torch
    from bench_detect import timed_ms
    from bench_repose import make_generator, scene
    from imm_amd import ops
    from imm_amd.generation import compose_inv_ramp, compose_links
    from imm_amd.inference import pack_u8, plan_buckets
    from imm_amd.keypoints import check_boxes
    B, m = args.batch, args.anchors
    photos, boxes, _lm = scene(B)
    model, gen = make_generator(B)
    det = gen.detector
    assert len(plan_buckets(B, B)) == 1
    props = torch.cuda.get_device_properties(0)
    poses = torch.from_numpy(grid_poses(B)).cuda()
    rows = check_boxes(boxes, B)
    out, pw = det.warp(photos, poses, boxes, anchors=m, return_transform=True)
    torch.cuda.synchronize()
    flagged = int(pw.flags.sum())
    changed = sum(int((o.cpu().numpy() != p).any(axis=2).sum()) for o, p in zip(out, photos))
    # the two kernels alone, on the buffers of that call
    src, offs_d, hw_d, boxes_d = pack_u8(photos, 'cuda:0', rows)
    canvas = src.clone()
    links_d = ops.to_device_pinned(compose_links(rows), 'cuda:0')
    ramp_d = ops.to_device_pinned(compose_inv_ramp(rows, 0.125), 'cuda:0')
    area = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max())
    anchors_d = None
    if m:
        from imm_amd.warping import warp_anchors
        anchors_d = ops.to_device_pinned(warp_anchors(m).astype(np.float32), 'cuda:0')
    coef, ctrl, flags = torch.empty_like(pw.coef), torch.empty_like(pw.ctrl), torch.empty_like(pw.flags)
    fns = {'warp': lambda: det.warp(photos, poses, boxes, anchors=m), 'repose': lambda: gen.repose(photos, poses, boxes),
           'pack': lambda: pack_u8(photos, 'cuda:0', rows)[0].clone(),
           'fit': lambda: ops.warp_fit(pw.poses, pw.mu, anchors_d, 1.0, 0.0, coef, ctrl, flags),
           'u8': lambda: ops.warp_u8(src, canvas, offs_d, hw_d, boxes_d, links_d, ramp_d, pw.ctrl, pw.coef, area)}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    px = 0
    for i, y0, x0, y1, x1 in boxes:
        h, w = photos[i].shape[:2]
        px += max(0, min(y1, h) - max(y0, 0)) * max(0, min(x1, w) - max(x0, 0))
    M = K + 4 * m
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, anchors = %d (M = %d control points), bf16, one bucket of B = %d rows; %d u8 photos of about 512 x 384 (%.1f MB '
             'packed), one box of about 250 x 250 each (%.2f M box pixels in all); ms per call: median (min .. max) of %d alternated '
             'windows x %d calls' % (S, K, m, M, B, B, sum(p.size for p in photos) / 1e6, px / 1e6, args.windows, args.reps),
             'rows without a usable fit: %d of %d; photo pixels the warp changed: %d' % (flagged, B, changed),
             '%-8s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in ('warp', 'repose', 'pack', 'fit', 'u8'):
        lines.append('%-8s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '%.0f' % (B / med[k] * 1e3) if k in ('warp', 'repose') else '-'))
    lines.append('imm_warp_u8: %.1f ps per box pixel at %d logarithms each (%.2f G log/s); imm_warp_fit: %.1f us per launch of %d systems of %d x %d' % (
        med['u8'] * 1e9 / px, M, px * M / med['u8'] / 1e6, med['fit'] * 1e3, B, M + 3, M + 3))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'batch': B, 'anchors': m, 'warp_ms': med['warp'], 'repose_ms': med['repose'], 'pack_ms': med['pack'],
                      'fit_ms': med['fit'], 'u8_ms': med['u8'], 'flagged': flagged}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--anchors', type=int, default=2, help='anchor points per side of the box frame')
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
