"""Unsupervised landmarks of a folder of images through the LandmarkDetector (imm_amd/inference.py: the pose encoder alone, batch
norm folded into its convolutions, captured HIP-graph programs per batch bucket).  Images of any size are decoded to u8 and resized
to --im-size on the GPU (TF1 bilinear, align_corners), like the data loaders do.
    python scripts/detect.py --configs configs/paths/default.yaml configs/experiments/celeba-10pts.yaml \
        --checkpoint logs/celeba-10pts/model.ckpt-2000 --images-dir faces/ --out landmarks.npz [--plot landmarks.png]
The checkpoint is a `.pt` file written by scripts/train.py or a TensorFlow bundle prefix (the authors' release).
landmarks.npz holds `files` [N], `mu` [N, K, 2] ((y, x) in [-1, 1]), `landmarks` [N, K, 2] ((y, x) pixels of the im-size x im-size
image, the convert_landmarks convention of scripts/test.py) and `sizes` [N, 2] (the decoded images' heights and widths)."""
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
from imm_amd.utils.config import load_configs               # noqa: E402

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')


def main(args):
    config = load_configs(args.configs)
    torch.cuda.set_device(0)
    files = sorted(f for f in os.listdir(args.images_dir) if f.lower().endswith(EXTENSIONS))
    if not files:
        raise ValueError('no images in %s' % args.images_dir)
    dtype = {'bf16': torch.bfloat16, 'f16': torch.float16}[args.dtype]
    det = LandmarkDetector.from_checkpoint(config.model, args.checkpoint, image_size=args.im_size, max_batch=args.batch_size,
                                           dtype=dtype, device='cuda:0')
    mus, sizes = [], []
    chunk = 4 * args.batch_size                  # images decoded and held on the host at a time
    for i in range(0, len(files), chunk):
        ims = [decode_image(osp.join(args.images_dir, f)) for f in files[i:i + chunk]]
        sizes += [im.shape[:2] for im in ims]
        mus.append(det.detect(ims).cpu().numpy())
    mu = np.concatenate(mus)
    landmarks = ((mu + 1) / 2.0) * args.im_size
    np.savez(args.out, files=np.array(files), mu=mu, landmarks=landmarks, sizes=np.array(sizes, dtype=np.int32))
    print('%d images, %d landmarks each -> %s' % (mu.shape[0], mu.shape[1], args.out))
    if args.plot:
        from PIL import Image
        from imm_amd.utils.plot_landmarks import plot_landmarks
        tiles = []
        for f, lm in list(zip(files, landmarks))[:args.plot_max]:
            with Image.open(osp.join(args.images_dir, f)) as im:
                small = np.asarray(im.convert('RGB').resize((args.im_size, args.im_size), Image.BILINEAR))
            tiles.append(np.asarray(plot_landmarks(small, lm, scale=2)))
        cols = min(len(tiles), 8)
        rows = -(-len(tiles) // cols)
        h, w = tiles[0].shape[:2]
        sheet = np.full((rows * h, cols * w, 3), 255, dtype=np.uint8)
        for j, t in enumerate(tiles):
            sheet[(j // cols) * h:(j // cols + 1) * h, (j % cols) * w:(j % cols + 1) * w] = t
        Image.fromarray(sheet).save(args.plot)
        print('plot -> %s' % args.plot)


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
    main(parser.parse_args())
