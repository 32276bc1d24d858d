"""LandmarkDetector host side (imm_amd/inference.py): the batch-norm fold, the batch-bucket planner, checkpoint reading, argument
checks, and the product rule that the module never touches the oracle.  No GPU needed."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conv_f64(x, w, b, stride):
    """TF SAME convolution in f64 (oracle restatement, double precision): x NHWC, w HWIO."""
    return O.conv2d_same(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride).numpy()


@pytest.mark.parametrize('k,ci,co,stride,H', [(3, 8, 16, 1, 9), (3, 16, 24, 2, 10), (7, 3, 8, 1, 12), (1, 32, 10, 1, 4)],
                         ids=['3x3', '3x3_stride2', '7x7_rgb', '1x1'])
def test_fold_equals_eval_batch_norm(k, ci, co, stride, H):
    from imm_amd.inference import fold_batch_norm
    from imm_amd.engine import BN_EPS
    rng = np.random.default_rng(k * 100 + ci)
    x = rng.standard_normal((2, H, H, ci))
    w = rng.standard_normal((k, k, ci, co)) * 0.2
    b = rng.standard_normal(co)
    gamma = rng.uniform(-2.0, 2.0, co)                 # negative scales too: the ReLU comes after the fold
    beta = rng.standard_normal(co)
    mean = rng.standard_normal(co) * 3.0
    var = rng.uniform(1e-4, 5.0, co)
    wf, bf = fold_batch_norm(w, b, gamma, beta, mean, var)
    got = np.maximum(conv_f64(x, wf, bf, stride), 0.0)
    z = conv_f64(x, w, b, stride)
    ref = np.maximum((z - mean) / np.sqrt(var + BN_EPS) * gamma + beta, 0.0)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()
    # the oracle's own eval-mode batch norm (f64 here) agrees too
    bn, _ = O.batch_norm(torch.from_numpy(z), torch.from_numpy(gamma), torch.from_numpy(beta), torch.from_numpy(mean),
                         torch.from_numpy(var), training=False)
    assert np.abs(got - torch.relu(bn).numpy()).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize('max_batch', [256, 100, 64, 1])
@pytest.mark.parametrize('n', [1, 7, 100, 257, 1000])
def test_bucket_planner_covers_every_image_once(n, max_batch):
    from imm_amd.inference import bucket_sizes, plan_buckets
    plan = plan_buckets(n, max_batch)
    seen = np.zeros(n, dtype=np.int64)
    sizes = bucket_sizes(max_batch)
    for start, count, bucket in plan:
        assert 1 <= count <= bucket <= max_batch and bucket in sizes
        seen[start:start + count] += 1
    assert (seen == 1).all()
    assert [s for s, _c, _b in plan] == sorted(s for s, _c, _b in plan)
    assert len(plan) == -(-n // max_batch)                      # full buckets first, one tail bucket
    assert plan_buckets(0, max_batch) == []


def test_bucket_sizes_are_powers_of_two_up_to_max_batch():
    from imm_amd.inference import bucket_sizes
    assert bucket_sizes(256) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert bucket_sizes(100) == [1, 2, 4, 8, 16, 32, 64, 100]
    assert bucket_sizes(1) == [1]
    with pytest.raises(ValueError):
        bucket_sizes(0)


def test_inference_module_never_imports_the_oracle():
    src = open(os.path.join(ROOT, 'imm_amd', 'inference.py')).read()
    assert not re.search(r'^\s*(import|from)\s+oracle', src, flags=re.M)
    assert 'imm_oracle' not in src and 'np_ref' not in src
    code = 'import sys; import imm_amd.inference; print(any(m == "oracle" or m.startswith("oracle.") for m in sys.modules))'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    assert out.stdout.decode().split()[-1] == 'False'


def _fake_model(dtype, n_maps=10):
    return types.SimpleNamespace(engine=types.SimpleNamespace(dev=torch.device('cpu')), _config=O.default_model_config(n_maps),
                                 dtype=dtype)


def test_detector_limits():
    from imm_amd.inference import LandmarkDetector
    with pytest.raises(NotImplementedError):
        LandmarkDetector(_fake_model(torch.float32))                 # the f32 witness engine has no detector
    with pytest.raises(NotImplementedError):
        LandmarkDetector(_fake_model(torch.bfloat16, n_maps=65))     # soft-argmax limit
    with pytest.raises(ValueError):
        LandmarkDetector(_fake_model(torch.bfloat16), image_size=72)
    with pytest.raises(ValueError):
        LandmarkDetector(_fake_model(torch.bfloat16), image_size=48)
    with pytest.raises(RuntimeError):
        LandmarkDetector(types.SimpleNamespace(engine=None, _config=O.default_model_config(), dtype=torch.bfloat16))


def test_read_checkpoint_pt_and_tf_bundle(tmp_path):
    """The detector's variables from a scripts/train.py `.pt` file and from a TensorFlow bundle (reference naming) are the same
    f32 values; a bundle without them is refused."""
    from imm_amd.inference import pose_encoder_names, read_checkpoint
    from imm_amd.utils.tf_checkpoint import tf_variable_name, write_bundle
    cfg = O.default_model_config(10)
    P, St = O.init_params(cfg, 128, seed=3)
    g = torch.Generator().manual_seed(5)
    St = type(St)((k, v + torch.rand(v.shape, generator=g) if k.endswith('moving_variance') else v) for k, v in St.items())
    torch.save({'params': P, 'state': St}, str(tmp_path / 'model.pt'))
    write_bundle(str(tmp_path / 'tf' / 'model.ckpt'),
                 {tf_variable_name(k): v.numpy() for d in (P, St) for k, v in d.items() if not k.startswith('vgg16/')})
    a = read_checkpoint(str(tmp_path / 'model.pt'), 32)
    b = read_checkpoint(str(tmp_path / 'tf' / 'model.ckpt'), 32)
    pn, sn = pose_encoder_names(32)
    assert sorted(a[0]) == sorted(pn) and sorted(a[1]) == sorted(sn) and len(pn) == 8 * 4 + 2
    for i in (0, 1):
        for k in a[i]:
            assert a[i][k].dtype == torch.float32 and torch.equal(a[i][k], b[i][k]), k
            assert torch.equal(a[i][k], (P if i == 0 else St)[k]), k
    write_bundle(str(tmp_path / 'bad' / 'model.ckpt'), {'global_step': np.float32(1)})
    with pytest.raises(KeyError):
        read_checkpoint(str(tmp_path / 'bad' / 'model.ckpt'), 32)
    with pytest.raises(FileNotFoundError):
        read_checkpoint(str(tmp_path / 'missing'), 32)


def test_scripts_expose_the_detector():
    """scripts/test.py --detector (off by default) and scripts/detect.py parse their flags without a GPU."""
    for script, flag in (('test.py', '--detector'), ('detect.py', '--images-dir')):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=300)
        assert out.returncode == 0, out.stderr.decode()[-1500:]
        assert flag in out.stdout.decode()


def test_local_rows_renumbers_into_the_photos_used():
    from imm_amd.inference import local_rows
    part = np.array([(5, 1, 2, 30, 40), (2, -3, 0, 9, 8), (5, 7, 7, 20, 21), (9, 0, 0, 4, 4)], dtype=np.int32)
    used, local = local_rows(part)
    assert used.tolist() == [2, 5, 9] and local[:, 0].tolist() == [1, 0, 1, 2]
    assert local.dtype == np.int32 and np.array_equal(local[:, 1:], part[:, 1:])
    used, local = local_rows(part[3:])
    assert used.tolist() == [9] and local.dtype == np.int32 and np.array_equal(local, [(0, 0, 0, 4, 4)])
    already = np.array([(0, 1, 1, 5, 5), (1, 0, 0, 3, 3), (1, 2, 2, 6, 6), (2, 0, 1, 2, 3)], dtype=np.int32)
    used, local = local_rows(already)
    assert used.tolist() == [0, 1, 2] and local.dtype == np.int32 and np.array_equal(local, already)


def test_photo_rows_resolves_photos_and_boxes():
    from imm_amd.inference import photo_rows
    from imm_amd.keypoints import box_geometry, check_boxes
    rng = np.random.RandomState(0)
    photos = [rng.randint(0, 256, size=(20, 30, 3)).astype(np.uint8), rng.randint(0, 256, size=(17, 9)).astype(np.uint8),
              rng.randint(0, 256, size=(8, 12, 1)).astype(np.uint8)]
    images, u8, rows, geom = photo_rows(photos, None, 64)
    whole = check_boxes([(0, 0, 20, 30), (0, 0, 17, 9), (0, 0, 8, 12)], 3)
    assert u8 and np.array_equal(rows, whole) and rows.dtype == whole.dtype and np.array_equal(geom, box_geometry(whole, 64))
    assert [a.shape for a in images] == [(20, 30, 3), (17, 9, 3), (8, 12, 3)] and all(a.dtype == np.uint8 for a in images)
    assert np.array_equal(images[0], photos[0])
    for c in range(3):
        assert np.array_equal(images[1][:, :, c], photos[1]) and np.array_equal(images[2][:, :, c], photos[2][:, :, 0])
    boxes = [(2, 1, 1, 7, 9), (0, -4, 3, 10, 40)]
    images, u8, rows, geom = photo_rows(photos, boxes, 64)
    assert u8 and np.array_equal(rows, check_boxes(boxes, 3)) and np.array_equal(geom, box_geometry(rows, 64))
    batch = torch.zeros(5, 64, 64, 3)
    images, u8, rows, geom = photo_rows(batch, None, 64)
    assert not u8 and rows is None and images.shape == (5, 64, 64, 3)
    assert geom.dtype == np.float32 and np.array_equal(geom, np.tile(np.float32([0, 0, 1, 1]), (5, 1)))
    with pytest.raises(ValueError, match=re.escape('boxes need the images as a list of u8 arrays (a tensor batch is already S x S)')):
        photo_rows(batch, [(0, 0, 10, 10)] * 5, 64)
