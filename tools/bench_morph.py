"""Faces/s of LandmarkDetector.morph (u8 photos, donor photos and face boxes in, the photos out with every face blended with its donor's
in shape and texture, from the pixels of the two photographs) at S = 128, bf16, K = 10, the default 2 anchors per side (M = 18 control
points) and one bucket of B = 64 rows, with what a caller had to do before alongside, for orientation only: two LandmarkDetector.warp
calls (the photos and the donor photos, each towards a common pose), both results copied to the host and the boxes cross-dissolved
there in numpy.  Writes the table to profiles/morph_bench.txt.

  morph     detector.morph(photos, donors, boxes, donor_boxes, shape=0.5): pack + copy of both photo lists, a device copy to morph into,
            the donors' landmarks (their pack, crop and pose program), the box crop, the pose program's graph, imm_morph_poses, one
            imm_warp_fit over 2 B rows and one imm_morph_u8 launch
  dissolve  two detector.warp calls, .cpu() of both results, then per face 0.5 * box + 0.5 * donor box in numpy (the common part of the
            two boxes; a real cross-dissolve would also have to resample one box to the other's size)
  pack      what comes before any kernel of morph: both photo lists packed on the host, copied to the device, one of them copied once
            more there (inference.pack_u8 twice and a clone)
  poses, fit, u8   imm_morph_poses, imm_warp_fit over 2 B rows and imm_morph_u8 alone, on the buffers of one morph() call
All are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of the mean
per-call time).  The photos and the donor photos are about 512 x 384 (sizes vary by a few pixels) with one box of about 250 x 250 each.
An untrained model's landmarks sit in a small cloud, so lam = 1 keeps the systems regular; what the kernels cost does not depend on it.
With --colour the same photos, sizes and protocol time colour matching instead: detector.morph at colour = 1 against colour = 0,
alternated window by window after warm-up, and the new launches alone on one call's buffers (imm_colour_stats_u8 over the faces and
over the donors, imm_colour_gain, imm_morph_colour_u8 next to imm_morph_u8); the table is APPENDED to profiles/morph_bench.txt.
With --mask the same photos, sizes and protocol time the landmark-hull mask: detector.morph at mask = None against mask = 'hull', at
colour 0 and 1, alternated window by window after warm-up, once with the model's own landmarks (the protocol of the tables above; an
untrained model's landmarks sit in a small cloud, so its hull is small) and once with landmarks on a jittered grid over [-0.8, 0.8]^2
given to both sides (a hull of the size a face's is), and the two new launches alone on one call's buffers (imm_hull_fit, and
imm_morph_hull_u8 next to imm_morph_u8), with the share of the box pixels whose weight is > 0; the table is APPENDED as well.
With --seamless the same photos, sizes and protocol time the mean-value membrane: detector.morph at mask = 'hull' with seamless = 1
against seamless = 0, alternated window by window after warm-up, with landmarks on the jittered grid given to both sides (a hull of the
size a face's is), at ring = 128 and ring = 16, and the two new launches alone on one call's buffers (imm_seam_fit, and imm_morph_seam_u8
next to imm_morph_hull_u8), with the ratios; the table is APPENDED as well.
With --clip the clip morph is timed instead: LandmarkDetector.morph_clip over a synthetic clip of 64 frames of 1280 x 720 with two faces
of about 250 x 250 and two donor photos, against the loop over public calls it replaces (track(), .cpu(), then per frame the landmarks
brought back into the frame's box on the host and morph([frame], donors, boxes, landmarks, donor_landmarks)), for the four pastes (plain;
colour = 1; mask = 'hull'; mask = 'hull', seamless = 1, colour = 0.5).  Both sides are wall-clock times of the whole clip, from the call
to a final synchronisation (the loop synchronises every frame by construction), alternated window by window after warm-up clips; the
loop runs calls that this tool's commit shares unchanged with its parent.  The library calls per frame are counted on the host (the
difference between a whole and a half clip).  Writes profiles/clip_morph_bench.txt.
Usage: python tools/bench_morph.py [--batch 64] [--windows 7] [--reps 10] [--anchors 2] [--colour | --mask | --seamless | --clip]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUT = os.path.join(ROOT, 'profiles', 'morph_bench.txt')
CLIP_OUT = os.path.join(ROOT, 'profiles', 'clip_morph_bench.txt')
S, K = 128, 10
LAM = 1.0


def clip_leg(args):
    """--clip: morph_clip against the loop over public calls, ms per frame, and the library calls per frame."""
    import time
    import torch
    from bench_repose import make_generator, scene
    from imm_amd import ops
    from imm_amd.tracking import OneEuro
    T, F, H, W = args.frames, 2, 720, 1280
    rng = np.random.RandomState(0)
    base = rng.randint(0, 256, size=(H + T, W + T, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(base[t:t + H, t:t + W]) for t in range(T)]          # the scene moves a pixel a frame
    faces = [(0, 120, 200, 370, 450), (0, 300, 800, 556, 1044)]
    donors, dboxes, _lm = scene(F, seed=1)
    _model, gen = make_generator(F)
    det = gen.detector
    props = torch.cuda.get_device_properties(0)
    dl = det.landmarks(donors, dboxes).clone()
    track_kw = dict(box_smooth=0.5, one_euro=OneEuro(), fps=25.0)
    common = dict(donor_boxes=dboxes, donor_landmarks=dl, shape=0.0, texture=1.0, anchors=args.anchors, lam=LAM)
    pastes = [('plain', dict()), ('colour', dict(colour=1.0)), ('hull', dict(mask='hull')), ('seamless', dict(mask='hull', seamless=1.0, colour=0.5))]

    def loop(paste):
        tr = det.track(frames, faces, **track_kw).cpu()
        boxes, pts = tr.boxes.numpy().astype(np.float64), tr.points_smooth.numpy().astype(np.float64)
        out = []
        for t in range(T):
            side = boxes[t, :, 2:] - boxes[t, :, :2]
            scale = (side.astype(np.float32) / np.float32(S)).astype(np.float64)
            own = np.clip((pts[t] - boxes[t, :, None, :2]) / scale[:, None] / S * 2.0 - 1.0, -1.0, 1.0).astype(np.float32)
            rows = [(0,) + tuple(int(v) for v in b) for b in tr.boxes[t].tolist()]
            out.append(det.morph([frames[t]], donors, boxes=rows, landmarks=torch.from_numpy(own), **dict(common, **paste))[0])
        return out

    def clip(paste, n=T):
        return det.morph_clip(frames[:n], faces, donors, colour_smooth=0.25, seam_smooth=0.25, **dict(common, **dict(track_kw, **paste)))

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def calls_per_frame(paste):
        count, real = [0], ops.call

        def counting(name, *a):
            count[0] += 1
            return real(name, *a)
        ops.call = counting
        try:
            clip(paste, T)
            whole = count[0]
            count[0] = 0
            clip(paste, T // 2)
            half = count[0]
        finally:
            ops.call = real
        return (whole - half) / float(T - T // 2)

    lines = ['==== clip morph (--clip) ====',
             'device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, anchors = %d, lam = %g, bf16; a synthetic clip of %d u8 frames of %d x %d, %d faces of about 250 x 250, %d donor '
             'photos of about 512 x 384; box_smooth 0.5, OneEuro(), 25 fps, chunk_frames 32, smooth = True, colour_smooth = seam_smooth = 0.25'
             % (S, K, args.anchors, LAM, T, W, H, F, F),
             'wall-clock ms per frame (the clip\'s time over its frames), the two sides alternating, median (min .. max) of %d windows after %d '
             'warm-up clips each' % (args.windows, args.warmup),
             'loop = track(), .cpu(), then per frame the landmarks brought back on the host and morph([frame], donors, ...): calls that this '
             'commit shares unchanged with its parent',
             'clip = LandmarkDetector.morph_clip(frames, faces, donors, ...); calls = library calls per frame of it, counted on the host (the '
             'captured pose program is one; the copy of the landmarks and the OR of the fit flags are two torch launches more)',
             '%-9s %28s %28s %8s %7s' % ('paste', 'loop ms/frame', 'clip ms/frame', 'ratio', 'calls')]
    rows = []
    for name, paste in pastes:
        for _ in range(args.warmup):
            loop(paste)
            clip(paste)
        t_loop, t_clip = [], []
        for _ in range(args.windows):
            t_loop.append(wall_ms(lambda: loop(paste)) / T)
            t_clip.append(wall_ms(lambda: clip(paste)) / T)
        ml, mc = float(np.median(t_loop)), float(np.median(t_clip))
        calls = calls_per_frame(paste)
        fmt = lambda v: '%7.3f (%7.3f .. %7.3f)' % (float(np.median(v)), min(v), max(v))
        lines.append('%-9s %28s %28s %8.2f %7.1f' % (name, fmt(t_loop), fmt(t_clip), ml / mc, calls))
        print(lines[-1], flush=True)
        rows.append({'paste': name, 'loop_ms_per_frame': ml, 'clip_ms_per_frame': mc, 'loop_over_clip': ml / mc, 'calls_per_frame': calls})
    slower = [r['paste'] for r in rows if r['loop_over_clip'] <= 1.0]
    lines.append('morph_clip is faster than the loop for every paste' if not slower else
                 'morph_clip is NOT faster than the loop for: %s' % ', '.join(slower))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'frames': T, 'faces': F, 'rows': rows}))


def main(args):
    import torch
    from bench_detect import timed_ms
    from bench_repose import make_generator, scene
    from bench_warp import grid_poses
    from imm_amd import ops
    from imm_amd.generation import compose_inv_ramp, compose_links
    from imm_amd.inference import pack_u8, plan_buckets
    from imm_amd.keypoints import check_boxes
    from imm_amd.warping import warp_anchors
    B, m = args.batch, args.anchors
    M = K + 4 * m
    photos, boxes, _lm = scene(B)
    donors, dboxes, _lm = scene(B, seed=1)
    model, gen = make_generator(B)
    det = gen.detector
    assert len(plan_buckets(B, B)) == 1
    props = torch.cuda.get_device_properties(0)
    mid = torch.from_numpy(grid_poses(B)).cuda()
    rows, drows = check_boxes(boxes, B), check_boxes(dboxes, B)
    out, pm = det.morph(photos, donors, boxes, dboxes, shape=0.5, anchors=m, lam=LAM, return_transform=True)
    torch.cuda.synchronize()
    flagged = int((pm.flags != 0).sum())
    changed = sum(int((o.cpu().numpy() != p).any(axis=2).sum()) for o, p in zip(out, photos))

    def dissolve():
        a = det.warp(photos, mid, boxes, anchors=m, lam=LAM)
        b = det.warp(donors, mid, dboxes, anchors=m, lam=LAM)
        res = []
        for (i, y0, x0, y1, x1), (j, v0, u0, v1, u1) in zip(boxes, dboxes):
            pa, pb = a[i].cpu().numpy(), b[j].cpu().numpy()
            fa, fb = pa[max(y0, 0):y1, max(x0, 0):x1], pb[max(v0, 0):v1, max(u0, 0):u1]
            h, w = min(fa.shape[0], fb.shape[0]), min(fa.shape[1], fb.shape[1])
            fa[:h, :w] = np.rint(0.5 * fa[:h, :w].astype(np.float32) + 0.5 * fb[:h, :w].astype(np.float32)).astype(np.uint8)
            res.append(pa)
        return res

    # the three kernels alone, on the buffers of that call
    src, offs_d, hw_d, boxes_d = pack_u8(photos, 'cuda:0', rows)
    don, doffs_d, dhw_d, dboxes_d = pack_u8(donors, 'cuda:0', drows)
    canvas = src.clone()
    links_d = ops.to_device_pinned(compose_links(rows), 'cuda:0')
    ramp_d = ops.to_device_pinned(compose_inv_ramp(rows, 0.125), 'cuda:0')
    shape_d = ops.to_device_pinned(pm.shape, 'cuda:0')
    texture_d = ops.to_device_pinned(pm.texture, 'cuda:0')
    area = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max())
    anchors_d = ops.to_device_pinned(warp_anchors(m).astype(np.float32), 'cuda:0') if m else None
    poses2, mu2 = torch.empty(2, B, K, 2, device='cuda:0'), torch.empty(2, B, K, 2, device='cuda:0')
    coef2, ctrl2 = torch.empty(2 * B, M + 3, 2, device='cuda:0'), torch.empty(2 * B, M, 2, device='cuda:0')
    flags2 = torch.empty(2 * B, dtype=torch.int32, device='cuda:0')
    ops.morph_poses(pm.mu, pm.donor_mu, shape_d, poses2, mu2)

    def paste_args(q):
        """ops.morph_paste's sixteen leading arguments: the buffers above with the splines of the PhotoMorph q."""
        return src, canvas, offs_d, hw_d, don, doffs_d, dhw_d, boxes_d, dboxes_d, links_d, ramp_d, texture_d, q.ctrl, q.coef_a, q.coef_b, area

    if args.colour:
        return colour_leg(args, det, photos, donors, boxes, dboxes, rows, drows, pm, props, paste_args, (src, offs_d, hw_d, boxes_d),
                          (don, doffs_d, dhw_d, dboxes_d), area)
    if args.mask:
        return mask_leg(args, det, photos, donors, boxes, dboxes, props, mid, poses2, paste_args, boxes_d)
    if args.seamless:
        return seam_leg(args, det, photos, donors, boxes, dboxes, props, mid, paste_args, lambda q, grow, dirs, ring, diff, flags: ops.seam_fit(
            q.poses, boxes_d, grow, q.hull_edges, q.hull_flags, dirs, src, offs_d, hw_d, don, doffs_d, dhw_d, dboxes_d, texture_d, q.ctrl,
            q.coef_a, q.coef_b, None, ring, diff, flags))
    fns = {'morph': lambda: det.morph(photos, donors, boxes, dboxes, shape=0.5, anchors=m, lam=LAM), 'dissolve': dissolve,
           'pack': lambda: (pack_u8(photos, 'cuda:0', rows)[0].clone(), pack_u8(donors, 'cuda:0', drows)),
           'poses': lambda: ops.morph_poses(pm.mu, pm.donor_mu, shape_d, poses2, mu2),
           'fit': lambda: ops.warp_fit(poses2.view(2 * B, K, 2), mu2.view(2 * B, K, 2), anchors_d, 1.0, LAM, coef2, ctrl2, flags2),
           'u8': lambda: ops.morph_u8(*paste_args(pm))}
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
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, anchors = %d (M = %d control points), lam = %g, bf16, one bucket of B = %d rows; %d u8 photos and %d donor photos of '
             'about 512 x 384 (%.1f MB + %.1f MB packed), one box of about 250 x 250 each (%.2f M box pixels in all); ms per call: median '
             '(min .. max) of %d alternated windows x %d calls' % (S, K, m, M, LAM, B, B, B, sum(p.size for p in photos) / 1e6,
                                                                   sum(p.size for p in donors) / 1e6, px / 1e6, args.windows, args.reps),
             'rows without a usable fit: %d of %d; photo pixels the morph changed: %d' % (flagged, B, changed),
             '%-8s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in ('morph', 'dissolve', 'pack', 'poses', 'fit', 'u8'):
        lines.append('%-8s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k],
                                                '%.0f' % (B / med[k] * 1e3) if k in ('morph', 'dissolve') else '-'))
    lines.append('imm_morph_u8: %.1f ps per box pixel at %d logarithms each (%.2f G log/s); imm_warp_fit: %.1f us per launch of %d systems of '
                 '%d x %d; imm_morph_poses: %.1f us' % (med['u8'] * 1e9 / px, M, px * M / med['u8'] / 1e6, med['fit'] * 1e3, 2 * B, M + 3, M + 3,
                                                        med['poses'] * 1e3))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'batch': B, 'anchors': m, 'morph_ms': med['morph'], 'dissolve_ms': med['dissolve'], 'pack_ms': med['pack'],
                      'poses_ms': med['poses'], 'fit_ms': med['fit'], 'u8_ms': med['u8'], 'flagged': flagged}))


def colour_leg(args, det, photos, donors, boxes, dboxes, rows, drows, pm, props, paste_args, own, donor, area):
    """--colour: morph at colour = 1 against colour = 0 on the same photos in the same run, and the new launches alone."""
    import torch
    from bench_detect import timed_ms
    from imm_amd import ops
    B, m = args.batch, args.anchors
    darea = int(((drows[:, 3] - drows[:, 1]) * (drows[:, 4] - drows[:, 2])).max())
    sums2 = torch.empty(2, B, 7, dtype=torch.int64, device='cuda:0')
    gain, cflags = torch.empty(B, 3, 2, device='cuda:0'), torch.empty(B, dtype=torch.int32, device='cuda:0')
    amount = ops.to_device_pinned(np.ones(B, np.float32), 'cuda:0')
    fns = {'colour=0': lambda: det.morph(photos, donors, boxes, dboxes, shape=0.5, anchors=m, lam=LAM),
           'colour=1': lambda: det.morph(photos, donors, boxes, dboxes, shape=0.5, anchors=m, lam=LAM, colour=1.0),
           'stats_a': lambda: ops.colour_stats_u8(own[0], own[1], own[2], own[3], area, sums2[0]),
           'stats_b': lambda: ops.colour_stats_u8(donor[0], donor[1], donor[2], donor[3], darea, sums2[1]),
           'gain': lambda: ops.colour_gain(sums2[0], sums2[1], amount, 2.0, gain, cflags),
           'u8': lambda: ops.morph_u8(*paste_args(pm)), 'colour_u8': lambda: ops.morph_paste(*paste_args(pm), gain=gain)}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    g = gain.cpu().numpy()
    region = int(sums2[0, :, 6].sum()), int(sums2[1, :, 6].sum())
    lines = ['==== colour matching (--colour) ====',
             'device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'the photos, donor photos, boxes and protocol of the tables above (B = %d, anchors = %d, lam = %g, bf16); ms per call: median '
             '(min .. max) of %d alternated windows x %d calls; max_gain = 2' % (B, m, LAM, args.windows, args.reps),
             'region pixels: %d of the faces, %d of the donors; gains %.3f .. %.3f, offsets %.1f .. %.1f; flagged rows: %d' % (
                 region[0], region[1], g[..., 0].min(), g[..., 0].max(), g[..., 1].min(), g[..., 1].max(), int(cflags.sum())),
             '%-10s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in fns:
        lines.append('%-10s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '%.0f' % (B / med[k] * 1e3) if '=' in k else '-'))
    lines.append('colour=1 - colour=0: %+.3f ms per call (%+.2f %%); the three new launches alone: %.1f us; imm_colour_stats_u8: %.1f ps per '
                 'region pixel of the faces' % (med['colour=1'] - med['colour=0'], 100 * (med['colour=1'] / med['colour=0'] - 1),
                                                (med['stats_a'] + med['stats_b'] + med['gain']) * 1e3, med['stats_a'] * 1e9 / max(region[0], 1)))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n' + text)
    print(json.dumps({'batch': B, 'anchors': m, 'colour0_ms': med['colour=0'], 'colour1_ms': med['colour=1'], 'stats_a_ms': med['stats_a'],
                      'stats_b_ms': med['stats_b'], 'gain_ms': med['gain'], 'u8_ms': med['u8'], 'colour_u8_ms': med['colour_u8']}))


def mask_leg(args, det, photos, donors, boxes, dboxes, props, grid, poses2, paste_args, boxes_d):
    """--mask: morph at mask = 'hull' against mask = None on the same photos in the same run, and the new launches alone."""
    import torch
    from bench_detect import timed_ms
    from bench_warp import grid_poses
    from imm_amd import ops
    B, m = args.batch, args.anchors
    common = dict(shape=0.5, anchors=m, lam=LAM)
    given = dict(landmarks=grid, donor_landmarks=torch.from_numpy(grid_poses(B, seed=2)).cuda(), **common)
    _out, own = det.morph(photos, donors, boxes, dboxes, mask='hull', return_transform=True, **common)
    _out, grd = det.morph(photos, donors, boxes, dboxes, mask='hull', return_transform=True, **given)
    torch.cuda.synchronize()
    share = {}
    for name, q in (('own', own), ('grid', grd)):
        w = [q.hull_weight(i) for i in range(B)]
        share[name] = (sum(int((x > 0).sum()) for x in w), sum(x.size for x in w), int((q.hull_flags != 0).sum()))
    grow_d, soft_d = ops.to_device_pinned(own.grow, 'cuda:0'), ops.to_device_pinned(own.inv_soft, 'cuda:0')
    edges, hflags = torch.empty(B, K, 3, device='cuda:0'), torch.empty(B, dtype=torch.int32, device='cuda:0')
    fns = {'None c=0': lambda: det.morph(photos, donors, boxes, dboxes, **common),
           'hull c=0': lambda: det.morph(photos, donors, boxes, dboxes, mask='hull', **common),
           'None c=1': lambda: det.morph(photos, donors, boxes, dboxes, colour=1.0, **common),
           'hull c=1': lambda: det.morph(photos, donors, boxes, dboxes, colour=1.0, mask='hull', **common),
           'grid None': lambda: det.morph(photos, donors, boxes, dboxes, **given),
           'grid hull': lambda: det.morph(photos, donors, boxes, dboxes, mask='hull', **given),
           'hull_fit': lambda: ops.hull_fit(poses2[0], boxes_d, grow_d, edges, hflags),
           'u8': lambda: ops.morph_u8(*paste_args(own)),
           'hull_u8': lambda: ops.morph_paste(*paste_args(own), edges=own.hull_edges, inv_soft=soft_d),
           'grid u8': lambda: ops.morph_u8(*paste_args(grd)),
           'grid hull_u8': lambda: ops.morph_paste(*paste_args(grd), edges=grd.hull_edges, inv_soft=soft_d)}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    lines = ['==== landmark-hull mask (--mask) ====',
             'device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'the photos, donor photos, boxes and protocol of the tables above (B = %d, anchors = %d, lam = %g, bf16); ms per call: median '
             '(min .. max) of %d alternated windows x %d calls; grow = 1.25, mask_feather = 0.1; "grid": landmarks on a jittered grid given to '
             'both sides, otherwise the untrained model\'s own (a small cloud)' % (B, m, LAM, args.windows, args.reps),
             'box pixels with w > 0: %d of %d (%.1f %%) with the model\'s landmarks, %d of %d (%.1f %%) with the grid\'s; rows with a hull '
             'flag: %d and %d' % (share['own'][0], share['own'][1], 100.0 * share['own'][0] / share['own'][1], share['grid'][0],
                                  share['grid'][1], 100.0 * share['grid'][0] / share['grid'][1], share['own'][2], share['grid'][2]),
             '%-13s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in fns:
        whole = k[:4] in ('None', 'hull', 'grid') and 'u8' not in k and k != 'hull_fit'
        lines.append('%-13s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '%.0f' % (B / med[k] * 1e3) if whole else '-'))
    lines.append('hull - None: %+.3f ms per call at colour 0, %+.3f at colour 1, %+.3f with the grid\'s landmarks; imm_hull_fit %.1f us; '
                 'imm_morph_hull_u8 against imm_morph_u8: %.1f against %.1f us with the model\'s landmarks, %.1f against %.1f us with the '
                 'grid\'s' % (med['hull c=0'] - med['None c=0'], med['hull c=1'] - med['None c=1'], med['grid hull'] - med['grid None'],
                              med['hull_fit'] * 1e3, med['hull_u8'] * 1e3, med['u8'] * 1e3, med['grid hull_u8'] * 1e3, med['grid u8'] * 1e3))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n' + text)
    print(json.dumps(dict({'batch': B, 'anchors': m, 'share_own': share['own'][0] / share['own'][1],
                           'share_grid': share['grid'][0] / share['grid'][1]}, **{k.replace(' ', '_') + '_ms': v for k, v in med.items()})))


def seam_leg(args, det, photos, donors, boxes, dboxes, props, grid, paste_args, seam_fit):
    """--seamless: morph at seamless = 1 against seamless = 0 under the hull mask on the same photos in the same run, and the new
    launches alone."""
    import torch
    from bench_detect import timed_ms
    from bench_warp import grid_poses
    from imm_amd import morphing as MP
    from imm_amd import ops
    B, m = args.batch, args.anchors
    given = dict(shape=0.5, anchors=m, lam=LAM, landmarks=grid, donor_landmarks=torch.from_numpy(grid_poses(B, seed=2)).cuda(), mask='hull')
    runs = {ring: det.morph(photos, donors, boxes, dboxes, seamless=1.0, ring=ring, return_transform=True, **given)[1] for ring in (128, 16)}
    torch.cuda.synchronize()
    q = runs[128]
    w = [q.hull_weight(i) for i in range(B)]
    share = (sum(int((x > 0).sum()) for x in w), sum(x.size for x in w))
    flagged = {ring: int((r.seam_flags != 0).sum()) for ring, r in runs.items()}
    grow_d, soft_d = ops.to_device_pinned(q.grow, 'cuda:0'), ops.to_device_pinned(q.inv_soft, 'cuda:0')
    amount = ops.to_device_pinned(np.ones(B, np.float32), 'cuda:0')
    fns = {'hull': lambda: det.morph(photos, donors, boxes, dboxes, **given),
           'hull_u8': lambda: ops.morph_paste(*paste_args(q), edges=q.hull_edges, inv_soft=soft_d)}
    for ring, r in runs.items():
        dirs = ops.to_device_pinned(MP.seam_dirs(ring), 'cuda:0')
        out = torch.empty(B, ring, 2, device='cuda:0'), torch.empty(B, ring, 3, device='cuda:0'), torch.empty(B, dtype=torch.int32, device='cuda:0')
        fns['seamless %d' % ring] = lambda ring=ring: det.morph(photos, donors, boxes, dboxes, seamless=1.0, ring=ring, **given)
        fns['seam_fit %d' % ring] = lambda r=r, dirs=dirs, out=out: seam_fit(r, grow_d, dirs, *out)
        fns['seam_u8 %d' % ring] = lambda r=r: ops.morph_paste(*paste_args(r), edges=r.hull_edges, inv_soft=soft_d, ring=r.seam_ring,
                                                               diff=r.seam_diff, seamless=amount)
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    lines = ['==== mean-value membrane (--seamless) ====',
             'device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'the photos, donor photos, boxes and protocol of the tables above (B = %d, anchors = %d, lam = %g, bf16); ms per call: median '
             '(min .. max) of %d alternated windows x %d calls; mask = hull, grow = 1.25, mask_feather = 0.1, landmarks on a jittered grid '
             'given to both sides' % (B, m, LAM, args.windows, args.reps),
             'box pixels with w > 0: %d of %d (%.1f %%); rows with a seam flag: %d at ring = 128, %d at ring = 16' % (
                 share[0], share[1], 100.0 * share[0] / share[1], flagged[128], flagged[16]),
             '%-13s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in fns:
        whole = k == 'hull' or k.startswith('seamless')
        lines.append('%-13s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '%.0f' % (B / med[k] * 1e3) if whole else '-'))
    for ring in runs:
        lines.append('ring = %d: seamless / hull = %.2f per call (%.3f against %.3f ms); imm_morph_seam_u8 / imm_morph_hull_u8 = %.2f (%.1f '
                     'against %.1f us, %.1f ps per pixel with w > 0 and ring sample); imm_seam_fit %.1f us' % (
                         ring, med['seamless %d' % ring] / med['hull'], med['seamless %d' % ring], med['hull'],
                         med['seam_u8 %d' % ring] / med['hull_u8'], med['seam_u8 %d' % ring] * 1e3, med['hull_u8'] * 1e3,
                         (med['seam_u8 %d' % ring] - med['hull_u8']) * 1e9 / (share[0] * ring), med['seam_fit %d' % ring] * 1e3))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n' + text)
    print(json.dumps(dict({'batch': B, 'anchors': m, 'share': share[0] / share[1]}, **{k.replace(' ', '_') + '_ms': v for k, v in med.items()})))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--anchors', type=int, default=2, help='anchor points per side of the box frame')
    p.add_argument('--colour', action='store_true', help='time colour matching: morph at colour = 1 against colour = 0, and the new launches alone')
    p.add_argument('--mask', action='store_true',
                   help="time the landmark-hull mask: morph at mask = 'hull' against mask = None at colour 0 and 1, and the new launches alone")
    p.add_argument('--seamless', action='store_true',
                   help="time the mean-value membrane: morph at seamless = 1 against seamless = 0 under the hull mask, and the new launches alone")
    p.add_argument('--clip', action='store_true',
                   help='time the clip morph: morph_clip against the loop over public calls it replaces, ms per frame, for the four pastes')
    p.add_argument('--frames', type=int, default=64, help='with --clip: the frames of the synthetic clip')
    p.add_argument('--out', type=str, default=None, help='default: profiles/morph_bench.txt, with --clip profiles/clip_morph_bench.txt')
    a = p.parse_args()
    if a.out is None:
        a.out = CLIP_OUT if a.clip else OUT
    if a.clip:
        clip_leg(a)
    else:
        main(a)
