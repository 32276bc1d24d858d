"""Unsupervised landmarks of a folder of images through the LandmarkDetector (imm_amd/inference.py: the pose encoder alone, batch
norm folded into its convolutions, captured HIP-graph programs per batch bucket).  Images of any size are decoded to u8 and resized
to --im-size on the GPU (TF1 bilinear, align_corners), like the data loaders do.
    python scripts/detect.py --configs configs/paths/default.yaml configs/experiments/celeba-10pts.yaml \
        --checkpoint logs/celeba-10pts/model.ckpt-2000 --images-dir faces/ --out landmarks.npz [--plot landmarks.png]
The checkpoint is a `.pt` file written by scripts/train.py or a TensorFlow bundle prefix (the authors' release).
landmarks.npz holds `files` [N], `mu` [N, K, 2] ((y, x) in [-1, 1]), `landmarks` [N, K, 2] ((y, x) pixels of the im-size x im-size
image, the convert_landmarks convention of scripts/test.py) and `sizes` [N, 2] (the decoded images' heights and widths).
With --regressor (a file written by scripts/test.py --save-regressor) it also holds the regressed annotated points of every face:
`keypoints` [F, M, 2] ((y, x) pixels of the source image), `boxes` [F, 4] ((y0, x0, y1, x1) source pixels, half-open) and `owner`
[F] (the index into `files` of each face's image).  The faces are the rows of --boxes, a CSV (`file, y0, x0, y1, x1` per line) or
JSON ([[file, y0, x0, y1, x1], ...]) file, in its order; without --boxes, one face per image, the whole image.
With --track the images of the folder, in sorted order, are the frames of one clip and --boxes holds the faces of its FIRST frame
(every row names that file; no regressor needed).  The boxes of the later frames follow the landmarks on the GPU
(LandmarkDetector.tracker, imm_amd/tracking.py), and the file holds per frame and face: `mu`, `landmarks` [T, F, K, 2], `points` and
`points_smooth` [T, F, K, 2] ((y, x) source pixels, raw and after the One-Euro filter; --no-filter makes them equal), `boxes`
[T, F, 4] (the box each frame was cut with), `flags` [T, F] (bit 0: lost, bit 1: the box left the photo) and, with --regressor,
`keypoints` [T, F, M, 2].  --fps is the clip's frame rate, --box-smooth the weight of a frame in the box filter.
With --quality the file also holds, per image, `spread` [N, K] (how widely each landmark's probability is spread), `score` [N, 2] (the
mean spread, and the residual of the --template shape under the best similarity; 0 without --template) and `quality_flags` [N] (set by
a NaN score, or by the thresholds of --gate).  With --track --gate FILE (a gate written by scripts/test.py --save-gate) a face that
fails the gate on a frame is lost on that frame, and the same three arrays are written per frame and face ([T, F, ..]; the residual is
against the face's own first-frame shape).  No thresholds are built in: how well these scores tell a face from a non-face is unmeasured
(imm_amd/quality.py).
With --redact pixelate|smooth --out-dir DIR nothing is measured: every image is written to DIR as a PNG of its own size with the faces of
--boxes (without --boxes: each whole image) made unreadable (LandmarkDetector.redact: a mosaic of --blocks cells along the longer side
of a box, or the blur of that mosaic; --mask hull keeps the redaction to the landmark hull, grown by --grow and softened over
--mask-feather; --feather fades the box into the photo).  With --track the faces of the first frame are followed and redacted on every
frame (LandmarkDetector.redact_clip); a face that enters the clip later is NOT redacted.  A face whose landmarks cannot be trusted is
redacted over its whole box.  Nobody has measured how recognisable a face stays at any setting: no anonymity is claimed.
With --annotate --out-dir DIR nothing is measured either: every image is written to DIR as a PNG of its own size with what the detector
decided drawn into it on the device (LandmarkDetector.annotate: --draw points,box,hull,label; --marker-size the markers' radius; --grow
the hull's).  With --track the faces of the first frame are followed and every frame shows its landmarks, --trail earlier frames of them,
and each face's box in the colour of its status: ok, lost, outside, unsure with --gate (LandmarkDetector.annotate_clip).  --annotate and
--redact do not go together."""
from __future__ import print_function

import argparse
import os
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from imm_amd.datasets.impair_dataset import decode_image   # noqa: E402
from imm_amd.inference import LandmarkDetector              # noqa: E402
from imm_amd.keypoints import LandmarkRegressor              # noqa: E402
from imm_amd.utils.config import load_configs               # noqa: E402

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')
ANNOTATE_ONLY = ('draw', 'trail', 'marker_size')                                       # arguments that go with --annotate alone
REDACT_ONLY = ('out_dir', 'blocks', 'mask', 'grow', 'mask_feather', 'feather')      # arguments that go with --redact alone (default None)


def read_boxes(path, files):
    """Rows `file, y0, x0, y1, x1` of a CSV or JSON file -> (owner int [F], boxes int [F, 4]); owner indexes `files`."""
    import csv
    import json
    with open(path) as f:
        text = f.read()
    if path.lower().endswith('.json'):
        rows = json.loads(text)
    else:
        rows = [r for r in csv.reader(text.splitlines()) if r and not r[0].lstrip().startswith('#')]
        if rows and rows[0][0].strip() == 'file':
            rows = rows[1:]
    index = {f: i for i, f in enumerate(files)}
    owner, boxes = [], []
    for r in rows:
        if len(r) != 5:
            raise ValueError('%s: a row is `file, y0, x0, y1, x1`, got %r' % (path, r))
        name = str(r[0]).strip()
        if name not in index:
            raise ValueError('%s: %s is not an image of the folder' % (path, name))
        owner.append(index[name])
        boxes.append([int(float(v)) for v in r[1:]])
    return np.array(owner, dtype=np.int64), np.array(boxes, dtype=np.int64).reshape(-1, 4)


def track(args, det, reg, files):
    """--track: the folder as one clip, the faces of its first frame followed through it."""
    from imm_amd.tracking import OneEuro
    if not args.boxes:
        raise ValueError('--track needs --boxes with the faces of the first frame')
    owner, boxes = read_boxes(args.boxes, files)
    if len(owner) == 0 or (owner != 0).any():
        raise ValueError('%s: with --track every row names the first frame, %s' % (args.boxes, files[0]))
    gate = None
    if args.gate:
        from imm_amd.quality import QualityGate
        gate = QualityGate.load(args.gate, detector=det)
    live = det.tracker(regressor=reg, box_smooth=args.box_smooth, one_euro=None if args.no_filter else OneEuro(), fps=args.fps, gate=gate)
    sizes = []
    for i, f in enumerate(files):                       # one decoded frame on the host at a time
        im = decode_image(osp.join(args.images_dir, f))
        sizes.append(im.shape[:2])
        if i == 0:
            live.start(im, boxes.tolist())
        else:
            live.step(im)
    tr = live.result().cpu()
    mu = tr.mu.numpy()
    out = dict(files=np.array(files), mu=mu, landmarks=((mu + 1) / 2.0) * args.im_size, sizes=np.array(sizes, dtype=np.int32),
               points=tr.points.numpy(), points_smooth=tr.points_smooth.numpy(), boxes=tr.boxes.numpy(), flags=tr.flags.numpy())
    if reg is not None:
        out['keypoints'] = tr.keypoints.numpy()
    if gate is not None:
        out.update(spread=tr.spread.numpy(), score=tr.score.numpy(), quality_flags=tr.qflags.numpy())
    np.savez(args.out, **out)
    print('%d frames, %d faces tracked, %d landmarks each -> %s (%d lost%s)' % (
        mu.shape[0], mu.shape[1], mu.shape[2], args.out, int(tr.lost.sum()), '' if gate is None else ', %d unsure' % int(tr.unsure.sum())))


def redact(args, det, files):
    """--redact: the images written back to --out-dir with their faces pixelated or smoothed."""
    from PIL import Image
    from imm_amd.tracking import OneEuro
    if not args.out_dir:
        raise ValueError('--redact goes with --out-dir (the images are written back with their faces redacted)')
    kw = dict(mode=args.redact, mask=args.mask)                    # what is not given keeps the detector's default
    kw.update({k: getattr(args, k) for k in REDACT_ONLY if k != 'out_dir' and getattr(args, k) is not None})
    ims = [decode_image(osp.join(args.images_dir, f)) for f in files]
    if args.track:
        if not args.boxes:
            raise ValueError('--track needs --boxes with the faces of the first frame')
        owner, boxes = read_boxes(args.boxes, files)
        if len(owner) == 0 or (owner != 0).any():
            raise ValueError('%s: with --track every row names the first frame, %s' % (args.boxes, files[0]))
        gate = None
        if args.gate:
            from imm_amd.quality import QualityGate
            gate = QualityGate.load(args.gate, detector=det)
        cr = det.redact_clip(ims, boxes.tolist(), box_smooth=args.box_smooth, one_euro=None if args.no_filter else OneEuro(), fps=args.fps,
                             gate=gate, **kw)
        out, said = cr.frames, '%d frames, %d faces redacted (%d lost, covered whole)' % (len(cr), len(boxes), int(cr.track.lost.sum()))
    else:
        rows = None
        if args.boxes:
            owner, boxes = read_boxes(args.boxes, files)
            rows = np.concatenate([owner[:, None], boxes], axis=1).tolist()
        out = det.redact(ims, rows, **kw)
        said = '%d faces redacted in %d images' % (len(ims) if rows is None else len(rows), len(ims))
    os.makedirs(args.out_dir, exist_ok=True)
    for f, im in zip(files, out):
        Image.fromarray(im.cpu().numpy()).save(osp.join(args.out_dir, osp.splitext(osp.basename(f))[0] + '.png'))
    print('%s (%s, %d blocks) -> %s' % (said, args.redact, kw.get('blocks', 8), args.out_dir))


def check_annotate(args):
    """--annotate and what goes with it, checked before anything is loaded."""
    if args.annotate and args.redact:
        raise ValueError('--annotate and --redact do not go together: run the script once for each')
    if args.annotate and not args.out_dir:
        raise ValueError('--annotate goes with --out-dir (the images are written back with the annotation drawn into them)')
    if not args.annotate and any(getattr(args, k) is not None for k in ANNOTATE_ONLY):
        raise ValueError('--draw, --trail and --marker-size go with --annotate')
    if args.annotate and any(getattr(args, k) is not None for k in ('blocks', 'mask', 'mask_feather', 'feather')):
        raise ValueError('--blocks, --mask, --mask-feather and --feather go with --redact')


def annotate(args, det, files):
    """--annotate: the images written back to --out-dir with landmarks, boxes, hulls and numbers drawn into them."""
    from PIL import Image
    from imm_amd.tracking import OneEuro
    kw = dict(draw=tuple(d for d in (args.draw or 'points,box').split(',') if d))
    if args.marker_size is not None:
        kw['size'] = args.marker_size
    if args.grow is not None:
        kw['grow'] = args.grow
    ims = [decode_image(osp.join(args.images_dir, f)) for f in files]
    if args.track:
        if not args.boxes:
            raise ValueError('--track needs --boxes with the faces of the first frame')
        owner, boxes = read_boxes(args.boxes, files)
        if len(owner) == 0 or (owner != 0).any():
            raise ValueError('%s: with --track every row names the first frame, %s' % (args.boxes, files[0]))
        gate = None
        if args.gate:
            from imm_amd.quality import QualityGate
            gate = QualityGate.load(args.gate, detector=det)
        ca = det.annotate_clip(ims, boxes.tolist(), trail=args.trail or 0, box_smooth=args.box_smooth, smooth=not args.no_filter,
                               one_euro=None if args.no_filter else OneEuro(), fps=args.fps, gate=gate, **kw)
        out = ca.frames
        said = '%d frames, %d faces annotated (%d lost%s)' % (len(ca), len(boxes), int(ca.track.lost.sum()),
                                                            '' if gate is None else ', %d unsure' % int(ca.track.unsure.sum()))
    else:
        if args.trail:
            raise ValueError('--trail goes with --track')
        rows = None
        if args.boxes:
            owner, boxes = read_boxes(args.boxes, files)
            rows = np.concatenate([owner[:, None], boxes], axis=1).tolist()
        out = det.annotate(ims, rows, **kw)
        said = '%d faces annotated in %d images' % (len(ims) if rows is None else len(rows), len(ims))
    os.makedirs(args.out_dir, exist_ok=True)
    for f, im in zip(files, out):
        Image.fromarray(im.cpu().numpy()).save(osp.join(args.out_dir, osp.splitext(osp.basename(f))[0] + '.png'))
    print('%s (%s) -> %s' % (said, ','.join(kw['draw']), args.out_dir))


def main(args):
    check_annotate(args)
    config = load_configs(args.configs)
    torch.cuda.set_device(0)
    files = sorted(f for f in os.listdir(args.images_dir) if f.lower().endswith(EXTENSIONS))
    if not files:
        raise ValueError('no images in %s' % args.images_dir)
    dtype = {'bf16': torch.bfloat16, 'f16': torch.float16}[args.dtype]
    det = LandmarkDetector.from_checkpoint(config.model, args.checkpoint, image_size=args.im_size, max_batch=args.batch_size,
                                           dtype=dtype, device='cuda:0')
    reg = LandmarkRegressor.load(args.regressor, detector=det) if args.regressor else None
    if args.redact:
        return redact(args, det, files)
    if args.annotate:
        return annotate(args, det, files)
    if any(getattr(args, k) is not None for k in REDACT_ONLY):
        raise ValueError('--out-dir, --blocks, --mask, --grow, --mask-feather and --feather go with --redact')
    if args.track:
        return track(args, det, reg, files)
    if args.gate or args.template:
        if not args.quality:
            raise ValueError('--gate and --template go with --quality or --track')
    gate = template = None
    if args.quality:
        from imm_amd.alignment import LandmarkTemplate
        from imm_amd.quality import QualityGate
        gate = QualityGate.load(args.gate, detector=det) if args.gate else None
        template = LandmarkTemplate.load(args.template, detector=det) if args.template else None
    quality = []
    if args.boxes and reg is None:
        raise ValueError('--boxes needs --regressor')
    owner, boxes = read_boxes(args.boxes, files) if args.boxes else (None, None)
    mus, sizes = [], []
    kps = np.zeros((0 if reg is None else (len(files) if boxes is None else len(boxes)), 0 if reg is None else reg.M, 2), np.float32)
    chunk = 4 * args.batch_size                  # images decoded and held on the host at a time
    for i in range(0, len(files), chunk):
        ims = [decode_image(osp.join(args.images_dir, f)) for f in files[i:i + chunk]]
        sizes += [im.shape[:2] for im in ims]
        mus.append(det.detect(ims).cpu().numpy())
        if args.quality:
            quality.append(det.quality(ims, template=template, gate=gate).cpu())
        if reg is not None and boxes is None:
            kps[i:i + len(ims)] = det.keypoints(ims, reg).cpu().numpy()
        elif reg is not None:
            rows = np.nonzero((owner >= i) & (owner < i + len(ims)))[0]
            if rows.size:
                local = np.concatenate([owner[rows, None] - i, boxes[rows]], axis=1)
                kps[rows] = det.keypoints(ims, reg, boxes=local.tolist()).cpu().numpy()
    mu = np.concatenate(mus)
    landmarks = ((mu + 1) / 2.0) * args.im_size
    out = dict(files=np.array(files), mu=mu, landmarks=landmarks, sizes=np.array(sizes, dtype=np.int32))
    if args.quality:
        out.update(spread=np.concatenate([q.spread.numpy() for q in quality]), score=np.concatenate([q.score.numpy() for q in quality]),
                   quality_flags=np.concatenate([q.flags.numpy() for q in quality]))
    if reg is not None:
        if boxes is None:
            owner = np.arange(len(files), dtype=np.int64)
            boxes = np.concatenate([np.zeros((len(files), 2), np.int64), np.array(sizes, dtype=np.int64).reshape(-1, 2)], axis=1)
        out.update(keypoints=kps, boxes=boxes.astype(np.int32), owner=owner.astype(np.int32))
    np.savez(args.out, **out)
    print('%d images, %d landmarks each -> %s' % (mu.shape[0], mu.shape[1], args.out))
    if args.quality:
        print('quality: mean spread %.4f .. %.4f, residual %.4f .. %.4f, %d flagged' % (
            out['score'][:, 0].min(), out['score'][:, 0].max(), out['score'][:, 1].min(), out['score'][:, 1].max(),
            int((out['quality_flags'] != 0).sum())))
    if reg is not None:
        print('%d faces, %d keypoints each (%s)' % (kps.shape[0], reg.M, ', '.join(reg.labels)))
    if args.plot and reg is not None:
        from PIL import Image
        from imm_amd.utils.plot_landmarks import plot_landmarks
        tiles = []
        for j, f in list(enumerate(files))[:args.plot_max]:
            pts = kps[owner == j].reshape(-1, 2)                   # every face of the image, in its source pixels
            h, w = sizes[j]
            with Image.open(osp.join(args.images_dir, f)) as im:
                small = np.asarray(im.convert('RGB').resize((args.im_size, args.im_size), Image.BILINEAR))
            tiles.append(np.asarray(plot_landmarks(small, pts * np.array([args.im_size / h, args.im_size / w]), scale=2)))
        save_sheet(tiles, args.plot)
    elif args.plot:
        from PIL import Image
        from imm_amd.utils.plot_landmarks import plot_landmarks
        tiles = []
        for f, lm in list(zip(files, landmarks))[:args.plot_max]:
            with Image.open(osp.join(args.images_dir, f)) as im:
                small = np.asarray(im.convert('RGB').resize((args.im_size, args.im_size), Image.BILINEAR))
            tiles.append(np.asarray(plot_landmarks(small, lm, scale=2)))
        save_sheet(tiles, args.plot)


def save_sheet(tiles, path):
    from PIL import Image
    cols = min(len(tiles), 8)
    rows = -(-len(tiles) // cols)
    h, w = tiles[0].shape[:2]
    sheet = np.full((rows * h, cols * w, 3), 255, dtype=np.uint8)
    for j, t in enumerate(tiles):
        sheet[(j // cols) * h:(j // cols + 1) * h, (j % cols) * w:(j % cols + 1) * w] = t
    Image.fromarray(sheet).save(path)
    print('plot -> %s' % path)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Detect unsupervised landmarks in a folder of images.')
    parser.add_argument('--configs', nargs='+', required=True, help='config files (paths + experiment); the `model:` block is used')
    parser.add_argument('--checkpoint', type=str, required=True, help='.pt file or TensorFlow bundle prefix')
    parser.add_argument('--images-dir', type=str, required=True)
    parser.add_argument('--out', type=str, default='landmarks.npz')
    parser.add_argument('--plot', type=str, default=None, help='also draw the landmarks of the first images onto a contact sheet')
    parser.add_argument('--plot-max', type=int, default=32)
    parser.add_argument('--im-size', type=int, default=128)
    parser.add_argument('--batch-size', type=int, default=256, help='largest batch bucket of the detector')
    parser.add_argument('--dtype', choices=('bf16', 'f16'), default='bf16')
    parser.add_argument('--regressor', type=str, default=None,
                        help='regressor .npz of scripts/test.py --save-regressor: also write the annotated points of every face')
    parser.add_argument('--boxes', type=str, default=None,
                        help='CSV or JSON face boxes, one row `file, y0, x0, y1, x1` per face (default: each whole image)')
    parser.add_argument('--track', action='store_true',
                        help='the folder is one clip (frames in sorted order): follow the faces of --boxes, given for its first frame')
    parser.add_argument('--fps', type=float, default=25.0, help='--track: the frame rate of the clip')
    parser.add_argument('--box-smooth', type=float, default=0.5, help='--track: the weight of a frame in the box filter, in (0, 1]')
    parser.add_argument('--no-filter', action='store_true', help='--track: no One-Euro filter (points_smooth equals points)')
    parser.add_argument('--quality', action='store_true', help='also write the quality scores of every image: spread, score, quality_flags')
    parser.add_argument('--template', type=str, default=None,
                        help='--quality: a landmark template .npz (scripts/test.py --save-template), the reference shape of the residual')
    parser.add_argument('--gate', type=str, default=None,
                        help='--track / --quality: a quality gate .npz (scripts/test.py --save-gate); there are no built-in thresholds')
    parser.add_argument('--redact', choices=('pixelate', 'smooth'), default=None,
                        help='with --out-dir: write every image back with the faces of --boxes made unreadable (a mosaic, or its blur); '
                             'with --track the faces of the first frame are followed through the clip')
    parser.add_argument('--out-dir', type=str, default=None, help='--redact: the folder the redacted images are written to (PNG)')
    parser.add_argument('--blocks', type=int, default=None, help='--redact: cells along the longer side of a box, in [1, 64] (default 8)')
    parser.add_argument('--mask', choices=('hull',), default=None, help='--redact: only the landmark hull (default: the whole box)')
    parser.add_argument('--grow', type=float, default=None, help='--redact --mask hull: the factor by which the hull is grown (default 1.25)')
    parser.add_argument('--mask-feather', type=float, default=None,
                        help='--redact --mask hull: the share of the box side the mask softens over (default 0.1)')
    parser.add_argument('--feather', type=float, default=None, help='--redact: the share of the box side over which the paste fades (default 0)')
    parser.add_argument('--annotate', action='store_true',
                        help='with --out-dir: write every image back with the landmarks and boxes of --boxes drawn into it; with '
                             '--track the faces of the first frame are followed and every frame shows what the tracker and --gate decided')
    parser.add_argument('--draw', type=str, default=None,
                        help='--annotate: a comma list of points, box, hull, label (default points,box); --grow sets the hull')
    parser.add_argument('--trail', type=int, default=None, help='--annotate --track: the landmarks of that many earlier frames, in [0, 15]')
    parser.add_argument('--marker-size', type=float, default=None, help='--annotate: the radius of a marker in pixels, in (0, 32] (default 2.5)')
    main(parser.parse_args())
