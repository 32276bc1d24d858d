"""Faces of a folder of photos aligned to a landmark template through LandmarkDetector.align (imm_amd/alignment.py): every face is
warped on the GPU so that its unsupervised landmarks land on the template's, sampled once from the photo's own pixels.
    python scripts/align.py --configs configs/paths/default.yaml configs/experiments/celeba-10pts.yaml \
        --checkpoint logs/celeba-10pts/model.ckpt-2000 --images-dir photos/ --boxes faces.csv \
        --template mafl_template.npz --model similarity --out-dir aligned/ [--npz aligned.npz]
The faces are the rows of --boxes, a CSV (`file, y0, x0, y1, x1` per line) or JSON file as scripts/detect.py --boxes reads it, in its
order; without --boxes, one face per photo, the whole photo.  --template is a file of scripts/test.py --save-template (or of an
earlier --fit-template run); --fit-template PATH computes the template from these faces' own landmarks (their Procrustes-refined
mean shape), saves it to PATH and aligns to it.  --model similarity | affine | tps (--lam: the spline's smoothing).
--out-dir receives one PNG per face (`<row>_<file>.png`, --out-size pixels a side, default --im-size); --npz holds `files`, `owner`
[F], `boxes` [F, 4], `mu` [F, K, 2], `coef` [F, m3, 2] (the backward maps), `geom` [F, 4], `template` [K, 2], `model`, `lam` and
`out_size`."""
from __future__ import print_function

import argparse
import os
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from imm_amd.alignment import LandmarkTemplate                # noqa: E402
from imm_amd.datasets.impair_dataset import decode_image     # noqa: E402
from imm_amd.inference import LandmarkDetector                # noqa: E402
from imm_amd.keypoints import check_boxes                      # noqa: E402
from imm_amd.utils.config import load_configs                 # noqa: E402

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
from detect import EXTENSIONS, read_boxes                      # noqa: E402


def main(args):
    from PIL import Image
    config = load_configs(args.configs)
    torch.cuda.set_device(0)
    if (args.template is None) == (args.fit_template is None):
        raise ValueError('give --template FILE or --fit-template FILE')
    files = sorted(f for f in os.listdir(args.images_dir) if f.lower().endswith(EXTENSIONS))
    if not files:
        raise ValueError('no images in %s' % args.images_dir)
    dtype = {'bf16': torch.bfloat16, 'f16': torch.float16}[args.dtype]
    det = LandmarkDetector.from_checkpoint(config.model, args.checkpoint, image_size=args.im_size, max_batch=args.batch_size,
                                           dtype=dtype, device='cuda:0')
    if args.boxes:
        owner, boxes = read_boxes(args.boxes, files)
    else:
        owner, boxes = np.arange(len(files), dtype=np.int64), None
    order = np.argsort(owner, kind='stable')                  # faces by photo, so that a chunk of photos is decoded once
    chunk = 4 * args.batch_size

    def faces():
        """(rows of the chunk, its photos, its (image, y0, x0, y1, x1) rows) over chunks of photos."""
        for i in range(0, len(files), chunk):
            rows = order[(owner[order] >= i) & (owner[order] < i + chunk)]
            if not rows.size:
                continue
            ims = [decode_image(osp.join(args.images_dir, f)) for f in files[i:i + chunk]]
            if boxes is None:
                local = [(int(o - i), 0, 0) + ims[int(o - i)].shape[:2] for o in owner[rows]]
            else:
                local = np.concatenate([owner[rows, None] - i, boxes[rows]], axis=1).tolist()
            yield rows, ims, local

    if args.fit_template:
        mu = np.zeros((len(owner), det.K, 2), np.float32)
        for rows, ims, local in faces():
            mu[rows] = det.landmarks(ims, boxes=local).cpu().numpy()
        template = LandmarkTemplate.from_landmarks(mu, det.S, dataset=args.images_dir, checkpoint=args.checkpoint)
        template.save(args.fit_template)
        print('template of %d faces -> %s' % (len(mu), args.fit_template))
    else:
        template = LandmarkTemplate.load(args.template, detector=det)
    So = args.out_size or args.im_size
    os.makedirs(args.out_dir, exist_ok=True)
    out = dict(mu=None, coef=None, geom=np.zeros((len(owner), 4), np.float32), boxes=np.zeros((len(owner), 4), np.int32))
    for rows, ims, local in faces():
        aligned, al = det.align(ims, template, boxes=local, model=args.model, lam=args.lam, out_size=So, return_transform=True)
        pix = np.clip(np.rint(aligned.cpu().numpy()), 0, 255).astype(np.uint8)
        coef, mu = al.coef.cpu().numpy(), al.mu.cpu().numpy()
        if out['mu'] is None:
            out['mu'] = np.zeros((len(owner),) + mu.shape[1:], np.float32)
            out['coef'] = np.zeros((len(owner),) + coef.shape[1:], np.float32)
        out['mu'][rows], out['coef'][rows], out['geom'][rows] = mu, coef, al.geom.cpu().numpy()
        out['boxes'][rows] = check_boxes(local, len(ims))[:, 1:]
        for r, p in zip(rows, pix):
            Image.fromarray(p).save(osp.join(args.out_dir, '%04d_%s.png' % (r, osp.splitext(files[owner[r]])[0])))
    print('%d faces aligned (%s, %d x %d) -> %s' % (len(owner), args.model, So, So, args.out_dir))
    if args.npz:
        np.savez(args.npz, files=np.array(files), owner=owner.astype(np.int32), template=template.points, model=np.array(args.model),
                 lam=np.float64(args.lam), out_size=np.int64(So), **out)
        print('coefficients -> %s' % args.npz)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Align the faces of a folder of photos to a landmark template.')
    parser.add_argument('--configs', nargs='+', required=True, help='config files (paths + experiment); the `model:` block is used')
    parser.add_argument('--checkpoint', type=str, required=True, help='.pt file or TensorFlow bundle prefix')
    parser.add_argument('--images-dir', type=str, required=True)
    parser.add_argument('--boxes', type=str, default=None,
                        help='CSV or JSON face boxes, one row `file, y0, x0, y1, x1` per face (default: each whole photo)')
    parser.add_argument('--template', type=str, default=None, help='template .npz (scripts/test.py --save-template, or --fit-template)')
    parser.add_argument('--fit-template', type=str, default=None,
                        help="compute the template from these faces' own landmarks, save it here and align to it")
    parser.add_argument('--model', choices=('similarity', 'affine', 'tps'), default='similarity')
    parser.add_argument('--lam', type=float, default=0.0, help='smoothing of the tps model')
    parser.add_argument('--out-size', type=int, default=None, help='side of the aligned images (default: --im-size)')
    parser.add_argument('--out-dir', type=str, default='aligned')
    parser.add_argument('--npz', type=str, default=None, help='also write the coefficients, landmarks and geometry')
    parser.add_argument('--im-size', type=int, default=128)
    parser.add_argument('--batch-size', type=int, default=256, help='largest batch bucket of the detector')
    parser.add_argument('--dtype', choices=('bf16', 'f16'), default='bf16')
    main(parser.parse_args())
