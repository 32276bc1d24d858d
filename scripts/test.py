"""Landmark-regression evaluation (reference: scripts/test.py, same flags).  The regressor's training split and the
test split come from the MAFL / AFLW loaders (imm_amd/datasets, tps=False, ordered stream) like the reference:
    python scripts/test.py --experiment-name celeba-10pts --train-dataset mafl --test-dataset mafl [--iteration N]
or, without dataset files, from .npz files with `image`, `future_image` (NHWC float32, [0,255]) and `future_landmarks`
([N,L,2] (y, x) pixels, first two points = the eyes):
    python scripts/test.py --configs a.yaml b.yaml --train-npz mafl_train.npz --test-npz mafl_test.npz --checkpoint x.pt
--save-regressor PATH also writes the regressor behind the printed error (coef, intercept, K, S, ...; imm_amd/keypoints.py), which
scripts/detect.py --regressor applies to photos.  --save-template PATH writes the mean landmark shape of the regressor's training
split (imm_amd/alignment.py: LandmarkTemplate, Procrustes-refined), which scripts/align.py --template aligns photos to.
--save-gate PATH --gate-quantile Q --gate-margin M (all three together) fits a quality gate (imm_amd/quality.py: QualityGate.fit) on the
faces of the test split: thresholds of M times the Q-quantile of their mean landmark spread and, with --template FILE (a template
written earlier by --save-template), of their shape residual against it; scripts/detect.py --track --gate applies it.  Q and M have no
defaults: nobody has measured which values suit footage."""
from __future__ import print_function

import argparse
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from imm_amd import ops                               # noqa: E402
from imm_amd.eval import eval_imm                     # noqa: E402
from imm_amd.models.imm_model import IMMModel        # noqa: E402
from imm_amd.utils.config import load_configs        # noqa: E402
from imm_amd.utils.dataset_import import import_dataset   # noqa: E402


def npz_batches(path, batch_size, device):
    d = np.load(path)
    n = d['image'].shape[0]
    for i in range(0, n, batch_size):
        sl = slice(i, min(i + batch_size, n))
        yield {'image': ops.to_device_pinned(d['image'][sl], device, torch.float32),
               'future_image': ops.to_device_pinned(d['future_image'][sl], device, torch.float32),
               'future_landmarks': d['future_landmarks'][sl]}


def landmark_dataset(name, datadir, subset, im_size, max_samples=None):
    """scripts/test.py:88-116 of the reference."""
    if name == 'mafl':
        return import_dataset('celeba')(datadir, dataset='mafl', subset=subset, order_stream=True, max_samples=max_samples,
                                        tps=False, image_size=[im_size, im_size])
    if name == 'aflw':
        return import_dataset('aflw')(datadir, subset=subset, order_stream=True, max_samples=max_samples, tps=False,
                                      image_size=[im_size, im_size])
    raise ValueError('Dataset %s not supported.' % name)


def fit_gate(args, net, detector, test_it):
    """--save-gate: the quality scores of the test split's faces (the pose encoder's input, `future_image`) -> a fitted QualityGate."""
    from imm_amd.alignment import LandmarkTemplate
    from imm_amd.quality import QualityGate
    det = detector if detector is not None else net.landmark_detector(args.im_size, max_batch=args.batch_size)
    template = LandmarkTemplate.load(args.template, detector=det) if args.template else None
    scores = []
    for batch in test_it:
        scores.append(det.quality(batch['future_image'], template=template).cpu().score.numpy())
    score = np.concatenate(scores).astype(np.float64)
    gate = QualityGate.fit((score[:, 0], score[:, 1]), args.gate_quantile, args.gate_margin)
    gate.K, gate.S, gate.heatmap = det.K, det.S, det.He
    gate.save(args.save_gate)
    print('quality gate of %d faces (quantile %g, margin %g): max_spread %s, max_residual %s -> %s' % (
        len(score), args.gate_quantile, args.gate_margin, gate.max_spread, gate.max_residual, args.save_gate))


def main(args):
    given = [args.save_gate is not None, args.gate_quantile is not None, args.gate_margin is not None]
    if any(given) and not all(given):
        raise ValueError('--save-gate, --gate-quantile and --gate-margin go together (the quantile and the margin have no defaults)')
    if args.template and not args.save_gate:
        raise ValueError('--template goes with --save-gate')
    config = load_configs([args.paths_config, osp.join('configs', 'experiments', args.experiment_name + '.yaml')]
                          if args.configs is None else args.configs)
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    net = IMMModel(config.model, device=dev)
    ckpt = args.checkpoint
    if ckpt is None:
        ckpt = osp.join(config.training.logdir, 'model.ckpt' + ('-%d' % args.iteration if args.iteration is not None else ''))
        if not osp.isfile(ckpt + '.index'):
            ckpt += '.pt'
    is_tf = osp.isfile(ckpt + '.index')       # a TensorFlow bundle prefix (the authors' released checkpoints)
    if not is_tf and not osp.isfile(ckpt):
        raise ValueError('Checkpoint file %s not found.' % ckpt)
    if args.train_npz is not None:
        first = min(args.batch_size, np.load(args.train_npz)['image'].shape[0])
        train_it = npz_batches(args.train_npz, args.batch_size, dev)
        test_it = npz_batches(args.test_npz, args.batch_size, dev)
    else:
        train_dset = landmark_dataset(args.train_dataset, config.training.datadir, 'train', args.im_size)
        test_dset = landmark_dataset(args.test_dataset, config.training.datadir, args.test_split, args.im_size)
        first = min(args.batch_size, train_dset.num_samples())
        train_it = train_dset.get_dataset(args.batch_size, repeat=False, shuffle=False, device=dev)
        test_it = test_dset.get_dataset(args.batch_size, repeat=False, shuffle=False, device=dev)
    eng = net._get_engine(first, args.im_size)
    if is_tf:
        from imm_amd.utils.tf_checkpoint import load_tf_checkpoint
        load_tf_checkpoint(eng, ckpt)
    else:
        ck = torch.load(ckpt, map_location='cpu')
        eng.load_parameters(ck['params'], ck.get('state'))
    detector = net.landmark_detector(args.im_size, max_batch=args.batch_size) if args.detector else None
    train_name = args.train_dataset if args.train_npz is None else args.train_npz
    landmarks = {} if args.save_template else None
    if args.save_regressor:
        err, reg = eval_imm.fit_regression(net, train_it, test_it, [args.im_size, args.im_size], batch_size=args.batch_size,
                                           bias=args.bias, detector=detector, dataset=train_name, checkpoint=ckpt,
                                           landmarks_out=landmarks)
        reg.save(args.save_regressor)
    else:
        err = eval_imm.evaluate_regression(net, train_it, test_it, [args.im_size, args.im_size], batch_size=args.batch_size,
                                           bias=args.bias, detector=detector, landmarks_out=landmarks)
    if args.save_template:
        from imm_amd.alignment import LandmarkTemplate
        LandmarkTemplate.from_landmarks(landmarks['gauss_yx'], args.im_size, dataset=train_name, checkpoint=ckpt).save(args.save_template)
    if args.save_gate:                                     # a fresh pass over the test split: the evaluation used its iterator up
        if args.train_npz is not None:
            again = npz_batches(args.test_npz, args.batch_size, dev)
        else:
            again = test_dset.get_dataset(args.batch_size, repeat=False, shuffle=False, device=dev)
        fit_gate(args, net, detector, again)
    model_dataset = config.training.train_dset_params.dataset if hasattr(config.training, 'train_dset_params') and \
        'dataset' in config.training.train_dset_params else getattr(config.training, 'dset', '?')
    print('')
    print('========================= RESULTS =========================')
    print('model trained in unsupervised way on %s dataset' % model_dataset)
    print('regressor trained on %s training set' % args.train_dataset)
    print('error on %s datset %s set: %.5f (%.3f percent)' % (args.test_dataset, args.test_split, err, err * 100.0))
    print('===========================================================')


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Test model on face datasets.')
    parser.add_argument('--experiment-name', type=str, required=False, default=None, help='Name of the experiment to evaluate.')
    parser.add_argument('--train-dataset', type=str, default='mafl', help='Training dataset for regressor (mafl|aflw).')
    parser.add_argument('--test-dataset', type=str, default='mafl', help='Testing dataset for regressed landmarks (mafl|aflw).')
    parser.add_argument('--paths-config', type=str, default='configs/paths/default.yaml', required=False)
    parser.add_argument('--iteration', type=int, default=None, help='Checkpoint iteration to evaluate.')
    parser.add_argument('--test-split', type=str, default='test', help='Test split (val|test).')
    parser.add_argument('--buffer-name', type=str, default=None)
    parser.add_argument('--im-size', type=int, default=128)
    parser.add_argument('--bias', action='store_true', required=False, help='Use bias in the regression.')
    parser.add_argument('--batch-size', type=int, default=100, required=False)
    # additions of this build
    parser.add_argument('--configs', nargs='+', default=None, help='explicit config files (instead of --experiment-name)')
    parser.add_argument('--checkpoint', type=str, default=None, help='explicit checkpoint file (default: <logdir>/model.ckpt[-N].pt)')
    parser.add_argument('--train-npz', type=str, default=None)
    parser.add_argument('--test-npz', type=str, default=None)
    parser.add_argument('--detector', action='store_true',
                        help='landmarks through the LandmarkDetector (pose encoder only, batch norm folded) instead of the full eval model')
    parser.add_argument('--save-regressor', type=str, default=None,
                        help='also write the fitted regressor behind the printed error to this .npz (imm_amd/keypoints.py; for '
                             'scripts/detect.py --regressor)')
    parser.add_argument('--save-template', type=str, default=None,
                        help="also write the mean landmark shape of the regressor's training split to this .npz "
                             '(imm_amd/alignment.py; for scripts/align.py --template)')
    parser.add_argument('--save-gate', type=str, default=None,
                        help='also fit a quality gate on the faces of the test split and write it to this .npz (imm_amd/quality.py; for '
                             'scripts/detect.py --track --gate); needs --gate-quantile and --gate-margin')
    parser.add_argument('--gate-quantile', type=float, default=None, help='--save-gate: the quantile of the scores, in (0, 1]; no default')
    parser.add_argument('--gate-margin', type=float, default=None, help='--save-gate: the factor on that quantile, >= 1; no default')
    parser.add_argument('--template', type=str, default=None,
                        help='--save-gate: a landmark template .npz, the reference shape of the residual (default: the spread alone)')
    main(parser.parse_args())
