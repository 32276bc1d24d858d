"""LandmarkDetector on the MI355X (imm_amd/inference.py): the ReLU epilogues of conv_s2f / conv_first bit for bit, landmark parity
with the oracle and with the existing eval path on a model whose batch-norm state is not the initial one, batch independence, the
launch program, read-only use of the model, the u8 input path, checkpoints and the scripts."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dataset_fixtures import make_celeba_tree     # noqa: E402
import guarded                                    # noqa: E402
from guarded import close                         # noqa: E402  (|got - ref| <= atol_frac * max|ref| + rtol * |ref|, NaN / inf fail)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE = 'model/pose_encoder'


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def rnd(shape, seed, scale=1.0, dt=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def dev(x):
    """A host (or device) tensor as a guarded operand on the device."""
    return guarded.inp(x, DEV, depth=2)


@pytest.fixture(autouse=True)
def _guards_intact():
    """After every test: no kernel wrote outside a tensor it was handed (tests/guarded.py)."""
    guarded.reset()
    yield
    guarded.check_guards()


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the two new epilogues
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('B', [1, 32, 100])
@pytest.mark.parametrize('H,ci,co', [(64, 64, 128), (32, 128, 256)], ids=['conv5_64to32', 'conv7_32to16'])
def test_s2f_relu_epilogue_bit_exact(ops, H, ci, co, B, dt):
    """The pose encoder's stride-2 descriptors with BIAS | RELU run conv_s2f (they fell to another family before), and the output
    is max(the same kernel's BIAS output, 0) bit for bit (ReLU on the f32 accumulator before the 16-bit store); with STATS the sums
    are those of the stored values; against the oracle within test_kernels_gpu.py's conv-forward tolerances."""
    from imm_amd import _lib as L
    x = dev(rnd((B, H, H, ci), 301, 1.0, dt))
    w = rnd((3, 3, ci, co), 302, 0.05, dt)
    b = rnd((co,), 303, 0.5, torch.float32).to(DEV)
    d_b = ops.fwd_desc(B, H, H, ci, ci, co, co, 3, 2, L.CONV_BIAS)
    d_r = ops.fwd_desc(B, H, H, ci, ci, co, co, 3, 2, L.CONV_BIAS | L.CONV_RELU)
    d_rs = ops.fwd_desc(B, H, H, ci, ci, co, co, 3, 2, L.CONV_BIAS | L.CONV_RELU | L.CONV_STATS)
    assert ops.conv2d_variant(d_r, dt)[0] == 's2f' and ops.conv2d_variant(d_r, dt) == ops.conv2d_variant(d_b, dt)
    assert ops.conv2d_variant(d_rs, dt) == ops.conv2d_variant(d_b, dt)
    rows = ops.round_up(co, 128)
    wt = guarded.out((rows, d_b.kpad), dt, DEV, fill=0)
    ops.pack_weights(w.float().to(DEV).contiguous(), wt, 0, 3, 3, ci, co, ci, rows, d_b.kpad)
    ys = [guarded.out((B, H // 2, H // 2, co), dt, DEV) for _ in range(3)]
    stats = guarded.out((ops.conv_stats_blocks(d_rs), 2, co), torch.float32, DEV)
    ops.conv2d(d_b, x, wt, b, ys[0])
    ops.conv2d(d_r, x, wt, b, ys[1])
    ops.conv2d(d_rs, x, wt, b, ys[2], stats)
    torch.cuda.synchronize()
    y_b, y_r, y_rs = (y.float().cpu() for y in ys)
    assert torch.equal(y_r, torch.clamp(y_b, min=0.0)), 's2f: ReLU epilogue != max(BIAS output, 0)'
    assert torch.equal(y_rs, y_r), 'the stats flag must not change the output'
    assert float(y_r.min()) >= 0.0 and bool((y_r > 0).any())
    st = stats.sum(0).cpu().double()
    close(st[0], y_r.double().sum((0, 1, 2)), 1e-2, 1e-3, 's2f relu sums')
    if B <= 32:
        ref = torch.relu(O.conv2d_same(x.float().cpu(), w.float(), b.cpu(), 2))
        close(ys[1], ref, 1e-2 if dt == torch.bfloat16 else 2e-3, 2e-3, 's2f relu vs oracle')


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('B,S', [(1, 128), (32, 128), (100, 128), (1, 256), (8, 256)])
def test_conv_first_relu_epilogue_bit_exact(ops, B, S, dt):
    """imm_conv_first with BIAS | RELU (conv_1 of the detector, straight from the f32 image) == max(its BIAS output, 0) bit for
    bit; with STATS too; against the oracle conv + ReLU of the 16-bit-rounded image."""
    from imm_amd import _lib as L
    co = 32
    g = torch.Generator().manual_seed(S + B)
    src = torch.rand(B, S, S, 3, generator=g) * 255
    w = rnd((7, 7, 3, co), 311, 0.01, torch.float32)
    bias = rnd((co,), 312, 0.5, torch.float32).to(DEV)
    srcd = dev(src)
    assert ops.conv_first_supported(B, S, co, co)
    wt = guarded.out((128, 224), dt, DEV, fill=0)
    ops.pack_weights(w.to(DEV).contiguous(), wt, 0, 7, 1, 21, co, 32, 128, 224)
    ys = [guarded.out((B, S, S, co), dt, DEV) for _ in range(3)]
    stats = guarded.out((ops.conv_first_stats_blocks(B, S), 2, co), torch.float32, DEV)
    ops.conv_first(srcd, wt, bias, ys[0], co, None, B, S, co, L.CONV_BIAS)
    ops.conv_first(srcd, wt, bias, ys[1], co, None, B, S, co, L.CONV_BIAS | L.CONV_RELU)
    ops.conv_first(srcd, wt, bias, ys[2], co, stats, B, S, co, L.CONV_BIAS | L.CONV_RELU | L.CONV_STATS)
    torch.cuda.synchronize()
    y_b, y_r, y_rs = (y.float().cpu() for y in ys)
    assert torch.equal(y_r, torch.clamp(y_b, min=0.0)), 'conv_first: ReLU epilogue != max(BIAS output, 0)'
    assert torch.equal(y_rs, y_r)
    assert float(y_r.min()) >= 0.0 and bool((y_r == 0).any()) and bool((y_r > 0).any())
    close(stats.sum(0)[0].cpu().double(), y_r.double().sum((0, 1, 2)), 1e-2, 1e-3, 'conv_first relu sums')
    if B <= 8:
        ref = torch.relu(O.conv2d_same(src.to(dt).float(), w.to(dt).float(), bias.cpu(), 1))
        close(ys[1], ref, 1e-2, 2e-3, 'conv_first relu vs oracle')


def test_unchanged_refusals(ops):
    """conv_first still refuses MASK (the new flag reaches s2f and conv_first only)."""
    from imm_amd import _lib as L
    img = guarded.out((2, 64, 64, 3), torch.float32, DEV, fill=0)
    wt = guarded.out((128, 224), torch.bfloat16, DEV, fill=0)
    y = guarded.out((2, 64, 64, 32), torch.bfloat16, DEV, fill=0)
    with pytest.raises(L.ImmHipError):
        ops.conv_first(img, wt, None, y, 32, None, 2, 64, 32, L.CONV_MASK)


# ----------------------------------------------------------------------------------------------------------------------------
# a model whose batch-norm state is not the initial one
# ----------------------------------------------------------------------------------------------------------------------------
def perturbed_variables(cfg, S, seed=11):
    """Oracle variables (seed 1, the engine's own initialisation) with every batch norm moved off its initial state: gamma in
    [0.5, 1.5], beta ~ N(0, 0.2), conv biases ~ N(0, 0.05), and moving statistics near the batch statistics of a calibration batch (mean + N(0, 0.1) std,
    variance x [0.7, 1.4]) so that the eval-mode activations keep a sane scale through the eight layers."""
    P, St = O.init_params(cfg, S, seed=1)
    rng = np.random.default_rng(seed)
    bn_scopes = [k[:-len('/gamma')] for k in P if k.endswith('/gamma')]
    for sc in bn_scopes:
        c = P[sc + '/gamma'].numel()
        P[sc + '/gamma'] = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
        P[sc + '/beta'] = torch.from_numpy((rng.standard_normal(c) * 0.2).astype(np.float32))
        P[sc + '/b'] = torch.from_numpy((rng.standard_normal(c) * 0.05).astype(np.float32))
    calib = O.synthetic_inputs(4, S, seed=seed)['future_image']
    for enc in ('model/pose_encoder', 'model/image_encoder'):
        ctx = O._Ctx(P, St, True)
        with torch.no_grad():
            O.encoder(ctx, calib, enc, cfg)
        for i in range(len(O.encoder_spec(cfg.n_filters))):
            sc = '%s/encoder/conv_%d' % (enc, i + 1)
            z = ctx.acts[sc + ':conv'].double()
            mean, var = z.mean((0, 1, 2)).numpy(), z.var((0, 1, 2), unbiased=False).numpy()
            c = mean.size
            St[sc + '/moving_mean'] = torch.from_numpy((mean + 0.1 * np.sqrt(var) * rng.standard_normal(c)).astype(np.float32))
            St[sc + '/moving_variance'] = torch.from_numpy((var * rng.uniform(0.7, 1.4, c)).astype(np.float32))
    return P, St


def make_model(K=10, S=128, B=4, dt=torch.bfloat16):
    from imm_amd.models.imm_model import IMMModel
    from imm_amd.utils.box import Box
    cfg = O.default_model_config(K)
    model = IMMModel(Box(dict(cfg)), dtype=dt, device=DEV)
    P, St = perturbed_variables(cfg, S)
    eng = model._get_engine(B, S)
    eng.load_parameters(P, {k: v for k, v in St.items() if '/moving_' in k})
    return cfg, model, eng, P, St


def images(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, S, S, 3, generator=g) * 255.0


# ----------------------------------------------------------------------------------------------------------------------------
# 2. parity
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,S,B,dt', [(10, 128, 32, torch.bfloat16), (10, 128, 32, torch.float16), (50, 128, 32, torch.bfloat16),
                                      (30, 256, 4, torch.bfloat16)], ids=['configs1_k10_bf16', 'k10_f16', 'k50', 's256_k30'])
def test_detect_matches_oracle_and_eval_path(ops, K, S, B, dt):
    cfg, model, eng, P, St = make_model(K, S, B, dt)
    x = images(B, S, 21)
    inputs = {'image': x, 'future_image': x}
    _, _, _, t = model.build(inputs, training_pl=False, output_tensors=True, build_loss=False)
    mu_eval = t['gauss_yx'].clone()
    heat_eval = t['heatmaps'].clone()
    det = model.landmark_detector(S)
    mu, heat = det.detect(x.to(DEV), heatmaps=True)
    mu_host = det.detect(x)                                   # host input: same bits
    torch.cuda.synchronize()
    assert mu.shape == (B, K, 2) and heat.shape == (B, S // 8, S // 8, K) and mu.dtype == torch.float32
    assert torch.equal(mu, mu_host)
    d_eval = float((mu - mu_eval).abs().max())
    n_or = min(B, 8)                                          # eval-mode batch norm is per sample: a subset is the same check
    with torch.no_grad():
        out = O.forward(P, St, {'image': x[:n_or], 'future_image': x[:n_or]}, cfg, training=False, build_loss=False)
    d_or = float((mu[:n_or].cpu() - out['gauss_yx']).abs().max())
    d_or_eval = float((mu_eval[:n_or].cpu() - out['gauss_yx']).abs().max())
    print('\nDETECT K=%d S=%d B=%d %s: max|mu - eval| %.2e  max|mu - oracle| %.2e  (eval vs oracle %.2e)  mu spread %.3f' % (
        K, S, B, dt, d_eval, d_or, d_or_eval, float(mu.std())))
    assert d_eval < 1e-3 and d_or < 1e-3
    assert float(mu.std()) > 1e-3                            # the landmarks are not a constant (the BN state matters)
    close(heat, heat_eval, 3e-2, 3e-2, 'heat maps vs eval path')
    close(heat[:n_or], out['heatmaps'], 3e-2, 3e-2, 'heat maps vs oracle')


# ----------------------------------------------------------------------------------------------------------------------------
# 3. batch independence, 4. program shape
# ----------------------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_repeatability(ops):
    """Eval-mode batch norm is per sample: within one bucket an image's landmarks do not depend on its position or its batchmates
    (bit for bit), and two calls with the same input are bit-identical.  ACROSS bucket sizes imm_conv2d picks the kernel by grid
    size (conv_6 / conv_8 at S = 128: igemm64 / igemm64 at batch 1, conv_hdeep / igemm64 at 8, conv_hdeep6 at 128 and 256), and
    those kernels sum the 3 x 3 x C products in different orders: the f32 accumulators differ in their last bits, an occasional
    16-bit rounding flips, and mu moves by a few 1e-6 (measured 3.9e-6 at bucket 8, 7.1e-6 at 128 and 256)."""
    cfg, model, eng, P, St = make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=256)
    one = images(1, 128, 5)
    got = {}
    for n, pos in ((1, 0), (7, 3), (100, 57), (256, 255)):
        x = images(n, 128, 100 + n)
        x[pos] = one[0]
        got[n] = det.detect(x)[pos]
    # same bucket, other position and other batchmates: bit-identical
    x = images(7, 128, 999)
    x[6] = one[0]
    assert torch.equal(det.detect(x)[6], got[7])
    dev = {n: float((got[n] - got[1]).abs().max()) for n in got}
    print('\nBATCH INDEPENDENCE max|mu(n) - mu(1)|: %s' % dev)
    assert max(dev.values()) < 5e-5, dev
    # same bucket size (max_batch 256: 100 images run as bucket 128), other batchmates: bit-identical
    x = images(120, 128, 1234)
    x[57] = one[0]
    assert torch.equal(det.detect(x)[57], got[100])
    x = images(100, 128, 7)
    a, b = det.detect(x), det.detect(x)
    assert torch.equal(a, b)


def test_program_shape(ops):
    """One bucket = 8 convolution launches + the pose head (+ the resize for u8 input); no batch-norm launch; conv_1 from the f32
    image, the stride-2 layers on conv_s2f, and every layer on the kernel family the training engine's BIAS-only (eval)
    descriptor of the same shape takes (the ReLU diverts none of them)."""
    from imm_amd import _lib as L
    cfg, model, eng, P, St = make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=32)
    prog = det.program(32)
    assert [l.tag for l in prog] == ['conv'] * 8 + ['pose_head']
    assert [l.tag for l in det.program(32, u8=True)] == ['resize'] + ['conv'] * 8 + ['pose_head']
    assert not any(l.tag.startswith('bn') for l in prog)
    fams = [l.family for l in prog[:8]]
    assert fams[0] == 'first' and fams[4] == 's2f' and fams[6] == 's2f', fams
    H = 128
    for i, (k, ci, co, st) in enumerate(O.encoder_spec(32)):
        if i:
            d = ops.fwd_desc(32, H, H, ci, ci, co, co, k, st, L.CONV_BIAS)
            if st == 2 and ci % 64 == 0:
                assert ops.conv2d_variant(d, torch.bfloat16)[0] == 's2f'
            else:
                assert ops.conv2d_variant(d, torch.bfloat16)[0] == fams[i], (i, fams)
        H = -(-H // st)
    print('\nDETECTOR PROGRAM B=32: %s' % [(l.name.rsplit('/', 1)[-1], l.family) for l in prog])


# ----------------------------------------------------------------------------------------------------------------------------
# 5. read-only
# ----------------------------------------------------------------------------------------------------------------------------
def test_detector_leaves_the_model_untouched(ops):
    cfg, model, eng, P, St = make_model(10, 128, 2)
    inputs = O.synthetic_inputs(2, 128, seed=3)
    before = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone(), eng.adam_m.clone(),
              eng.adam_v.clone(), eng.grads.clone())
    det = model.landmark_detector(128, max_batch=8)
    det.detect(images(11, 128, 1))
    det.detect([np.zeros((50, 60, 3), np.uint8)])
    det.refresh()
    torch.cuda.synchronize()
    after = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone(), eng.adam_m.clone(),
             eng.adam_v.clone(), eng.grads.clone())
    for a, b in zip(before[:2], after[:2]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    for a, b in zip(before[2:], after[2:]):
        assert torch.equal(a, b)
    # a training step after detection == the same step without it, bit for bit
    snap = eng.snapshot()
    model.build(inputs, True); eng.backward(); eng.optimizer_step()
    loss_a = eng.loss.clone()
    torch.cuda.synchronize()
    eng.restore(snap)
    det.detect(images(3, 128, 2))
    model.build(inputs, True); eng.backward(); eng.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.loss, loss_a)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. u8 input, 7. checkpoints
# ----------------------------------------------------------------------------------------------------------------------------
def test_u8_images_of_any_size(ops):
    cfg, model, eng, P, St = make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=4)
    rng = np.random.RandomState(0)
    sizes = [(218, 178), (128, 128), (300, 250), (90, 200), (64, 64)]
    ims = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    mu = det.detect(ims)                                      # buckets 4 + 1
    offs, total = [], 0
    for im in ims:
        offs.append(total)
        total += (im.size + 15) & ~15
    buf = np.zeros(total, np.uint8)
    for im, o in zip(ims, offs):
        buf[o:o + im.size] = im.reshape(-1)
    f32 = guarded.out((len(ims), 128, 128, 3), torch.float32, DEV)
    ops.resize_crop_u8(ops.to_device_pinned(buf, DEV), ops.to_device_pinned(np.array(offs, np.int64), DEV),
                       ops.to_device_pinned(np.array(sizes, np.int32), DEV), 3, (128, 128), (0, 0), (128, 128), f32)
    assert torch.equal(mu, det.detect(f32))
    grey = det.detect([ims[0][:, :, 0]])
    assert grey.shape == (1, 10, 2)
    with pytest.raises(TypeError):
        det.detect([ims[0].astype(np.float32)])


def test_detector_from_checkpoints(ops, tmp_path):
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.tf_checkpoint import save_tf_checkpoint
    cfg, model, eng, P, St = make_model(10, 128, 2, torch.float16)
    x = images(9, 128, 4)
    live = model.landmark_detector(128).detect(x)
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, str(tmp_path / 'model.pt'))
    save_tf_checkpoint(eng, str(tmp_path / 'tf' / 'model.ckpt'), with_optimizer=False)
    for path in (str(tmp_path / 'model.pt'), str(tmp_path / 'tf' / 'model.ckpt')):
        det = LandmarkDetector.from_checkpoint(model._config, path, image_size=128, dtype=torch.float16, device=DEV)
        assert torch.equal(det.detect(x), live), path


# ----------------------------------------------------------------------------------------------------------------------------
# 8. scripts
# ----------------------------------------------------------------------------------------------------------------------------
def _run_script(path, argv):
    import runpy
    old = sys.argv
    sys.argv = [path] + argv
    try:
        runpy.run_path(path, run_name='__main__')
    finally:
        sys.argv = old


def _write_config(tmp_path, datadir, logdir, n_maps=10):
    import yaml
    base = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'experiments', 'celeba-10pts.yaml')))
    base['training'].update({'datadir': datadir, 'logdir': logdir})
    base['model']['n_maps'] = n_maps
    base['model']['perceptual']['net_file'] = 'synthetic'
    cfg = str(tmp_path / 'exp.yaml')
    with open(cfg, 'w') as f:
        yaml.safe_dump(base, f)
    return cfg


def test_detect_script(ops, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = make_model(10, 128, 2)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    imdir = tmp_path / 'faces'
    imdir.mkdir()
    rng = np.random.RandomState(1)
    ims = []
    for i, (h, w) in enumerate([(218, 178), (128, 128), (300, 250), (100, 90), (218, 178)]):
        im = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        Image.fromarray(im).save(imdir / ('%02d.png' % i))
        ims.append(im)
    conf = _write_config(tmp_path, str(tmp_path), str(tmp_path / 'logs'))
    out = str(tmp_path / 'lm.npz')
    _run_script(os.path.join(ROOT, 'scripts', 'detect.py'), ['--configs', conf, '--checkpoint', ckpt, '--images-dir', str(imdir),
                                                             '--out', out, '--plot', str(tmp_path / 'sheet.png'), '--batch-size', '4'])
    assert '5 images' in capsys.readouterr().out
    r = np.load(out)
    assert list(r['files']) == ['%02d.png' % i for i in range(5)]
    assert r['mu'].shape == (5, 10, 2) and r['landmarks'].shape == (5, 10, 2) and r['sizes'].tolist()[2] == [300, 250]
    np.testing.assert_array_equal(r['landmarks'], (r['mu'] + 1) / 2.0 * 128)
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    np.testing.assert_array_equal(r['mu'], det.detect(ims).cpu().numpy())
    assert os.path.exists(str(tmp_path / 'sheet.png'))


def test_test_script_with_detector(ops, tmp_path, capsys):
    """scripts/test.py --detector on the fixture CelebA / MAFL tree reports the inter-ocular error of the full eval path.  The
    tree's MAFL training split has 10 images: with K = 3 landmarks (6 regressors) the unregularised Ridge fit is a least-squares
    problem rather than an under-determined one.  It is still ill-conditioned: an untrained model's landmarks spread over ~1 pixel
    between images, so the ~1e-4 landmark differences of two roundings of one model move the error by about a percent (measured:
    1.92533 vs 1.94010, 0.8 %); the bound is 2 % relative."""
    root = str(tmp_path / 'celeba')
    make_celeba_tree(root, n=40)
    cfg, model, eng, P, St = make_model(3, 128, 4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'), n_maps=3)
    errs = []
    for extra in ([], ['--detector']):
        _run_script(os.path.join(ROOT, 'scripts', 'test.py'), ['--configs', conf, '--train-dataset', 'mafl', '--test-dataset',
                                                               'mafl', '--checkpoint', ckpt, '--batch-size', '4'] + extra)
        m = re.search(r'error on mafl datset test set: ([0-9.]+)', capsys.readouterr().out)
        assert m is not None
        errs.append(float(m.group(1)))
    print('\nTEST.PY inter-ocular error: eval path %.5f, detector %.5f' % tuple(errs))
    assert abs(errs[0] - errs[1]) <= 2e-2 * errs[0], errs
