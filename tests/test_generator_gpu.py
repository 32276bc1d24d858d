"""ImageGenerator on the MI355X (imm_amd/generation.py): the render-only mode of imm_softargmax_gauss_fwd bit for bit, the ReLU
epilogues of every renderer layer, reconstruction parity with the oracle and the eval path on a model whose batch-norm state is not
the initial one, agreement of reconstruct / render / transfer, batch independence, read-only use, checkpoints and the script."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_detector_gpu import images, perturbed_variables      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. render-only mode
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('B', [1, 256])
@pytest.mark.parametrize('K', [10, 30, 50])
@pytest.mark.parametrize('mode', ['rot', 'flat', 'ankush'])
def test_render_only_mode_bit_exact(ops, mode, K, B, dt):
    """heat == NULL: the maps of the input mu, written into a strided wider buffer, equal bit for bit what the soft-argmax and the
    pose-head kernels write for the mu they computed; every byte outside the K channels keeps its sentinel; within one 16-bit ulp
    of O.gaussian_maps."""
    s, inv_std, C, off = 16, 1.0 / 0.1, 64, 8
    ldg = K + off + 24                                  # the maps start at channel `off` of a wider pixel row
    ldh = ops.round_up(K, 4)
    g = torch.Generator().manual_seed(K * 1000 + B)
    feat = (torch.randn(B, 16, 16, C, generator=g)).to(dt).to(DEV)
    w = (torch.randn(1, 1, C, K, generator=g) * 0.3).to(DEV)
    bias = (torch.randn(K, generator=g) * 0.5).to(DEV)
    wt = torch.zeros(ops.round_up(K, 128), C, dtype=dt, device=DEV)
    ops.pack_weights(w, wt, 0, 1, 1, C, K, C, wt.shape[0], C)
    heat = torch.zeros(B, 16, 16, ldh, device=DEV)
    mu = torch.zeros(B, K, 2, device=DEV)
    py, px = torch.zeros(B, 16, K, device=DEV), torch.zeros(B, 16, K, device=DEV)
    sentinel = torch.full((B, s, s, ldg), -1234.5, dtype=dt, device=DEV)
    g_head, g_sa, g_r1, g_r2 = (sentinel.clone() for _ in range(4))
    ops.pose_head_fwd(feat, C, C, wt, bias, B, 16, 16, K, inv_std, s, heat, ldh, mu, py, px, g_head[..., off:], ldg, dt, mode)
    mu_head = mu.clone()
    ops.gauss_render_fwd(mu_head, B, K, inv_std, s, g_r1[..., off:], ldg, dt, mode)
    ops.softargmax_gauss_fwd(heat, ldh, B, 16, 16, K, inv_std, s, mu, py, px, g_sa[..., off:], ldg, dt, mode)
    ops.gauss_render_fwd(mu, B, K, inv_std, s, g_r2[..., off:], ldg, dt, mode)
    torch.cuda.synchronize()
    assert torch.equal(bits(g_r2), bits(g_sa)), 'render-only != soft-argmax maps'
    if mode != 'rot':
        assert torch.equal(bits(g_r1), bits(g_head)), 'render-only != pose head maps'
    else:
        # the pose head compiles its 'rot' render as a specialisation of its own (GM = IMM_GAUSS_ROT) and its f32 value differs from
        # the runtime-mode writers' in the last bit now and then: the soft-argmax kernel and the pose head disagree with each other
        # for the same mu (measured at B = 256, K = 10: 31 of 2.75 M bf16 values, 6 f16), so no third writer can equal both;
        # this one equals the soft-argmax kernel, and is within one 16-bit ulp of the pose head
        diff = bits(g_r1) != bits(g_head)
        a, h = g_r1.float().cpu(), g_head.float().cpu()
        ulp = 2.0 ** (-7 if dt == torch.bfloat16 else -10)
        assert bool(((a - h).abs() <= ulp * h.abs() + 1e-7).all())
        assert int(diff.sum()) <= 1e-4 * diff.numel(), int(diff.sum())
    outside = torch.ones(ldg, dtype=torch.bool)
    outside[off:off + K] = False
    assert torch.equal(bits(g_r1[..., outside]), bits(sentinel[..., outside])), 'bytes outside the K channels changed'
    ref = O.gaussian_maps(mu.cpu(), [s, s], inv_std, mode=mode)
    got = g_r2[..., off:off + K].float().cpu()
    ulp = 2.0 ** (-7 if dt == torch.bfloat16 else -10)
    err = (got - ref).abs()
    assert bool((err <= ulp * ref.abs() + 1e-7).all()), 'render vs O.gaussian_maps: max err %.3g' % float(err.max())


def test_render_only_mode_refusals(ops):
    from imm_amd import _lib as L
    mu = torch.zeros(2, 10, 2, device=DEV)
    with pytest.raises(L.ImmHipError, match='softargmax_fwd: null'):
        ops.gauss_render_fwd(mu, 2, 10, 10.0, 16, None, 16, torch.bfloat16)
    with pytest.raises(L.ImmHipError, match='softargmax_fwd: null'):
        ops.gauss_render_fwd(None, 2, 10, 10.0, 16, torch.zeros(2, 16, 16, 16, dtype=torch.bfloat16, device=DEV), 16, torch.bfloat16)


# ----------------------------------------------------------------------------------------------------------------------------
# 2. ReLU epilogues of every renderer layer
# ----------------------------------------------------------------------------------------------------------------------------
def renderer_layers(K, S):
    """(H, ci_real, ci_pad, co) of every conv + BN + ReLU block of renderer_spec (the final f32 layer excluded)."""
    from imm_amd.engine import n_renderer_out, renderer_spec
    cfg = O.default_model_config(K)
    out, H = [], 16
    ci_pad = ops_round_up(8 * cfg.n_filters + K, 64)
    for (_k, ci, co, bn, up) in renderer_spec(cfg, S, n_renderer_out(cfg)):
        if bn:
            out.append((H, ci, ci_pad, co))
        ci_pad = co
        if up:
            H *= 2
    return out


def ops_round_up(x, m):
    return (x + m - 1) // m * m


@pytest.mark.parametrize('B', [1, 8, 32, 128])
@pytest.mark.parametrize('K,S', [(10, 128), (50, 128), (30, 256)], ids=['s128_k10', 's128_k50', 's256_k30'])
def test_renderer_relu_epilogues_bit_exact(ops, K, S, B):
    from imm_amd import _lib as L
    dt = torch.bfloat16
    fams = []
    for li, (H, ci, ci_pad, co) in enumerate(renderer_layers(K, S)):
        g = torch.Generator(device=DEV).manual_seed(li * 7 + B)
        x = torch.zeros(B, H, H, ci_pad, dtype=dt, device=DEV)
        x[..., :ci] = (torch.rand(B, H, H, ci, generator=g, device=DEV) * 2.0).to(dt)
        w = torch.randn(3, 3, ci, co, generator=g, device=DEV) * (1.0 / (3 * ci ** 0.5))
        b = torch.randn(co, generator=g, device=DEV) * 0.3
        d_b = ops.fwd_desc(B, H, H, ci_pad, ci_pad, co, co, 3, 1, L.CONV_BIAS)
        d_r = ops.fwd_desc(B, H, H, ci_pad, ci_pad, co, co, 3, 1, L.CONV_BIAS | L.CONV_RELU)
        fam = ops.conv2d_variant(d_r, dt)
        assert fam == ops.conv2d_variant(d_b, dt), 'the ReLU diverts layer %d to another kernel' % li
        wt = torch.zeros(ops.round_up(co, 128), d_b.kpad, dtype=dt, device=DEV)
        ops.pack_weights(w, wt, 0, 3, 3, ci, co, ci_pad, wt.shape[0], d_b.kpad)
        y_b = torch.full((B, H, H, co), float('nan'), dtype=dt, device=DEV)
        y_r = y_b.clone()
        ops.conv2d(d_b, x, wt, b, y_b)
        ops.conv2d(d_r, x, wt, b, y_r)
        torch.cuda.synchronize()
        y_b, y_r = y_b.float(), y_r.float()
        assert torch.equal(y_r, torch.clamp(y_b, min=0.0)), 'layer %d (%dx%d %d->%d, %s): ReLU != max(BIAS, 0)' % (li, H, H, ci, co, fam)
        assert bool((y_r == 0).any()) and bool((y_r > 0).any())
        fams.append(fam[0])
    print('\nRENDERER RELU FAMILIES K=%d S=%d B=%d: %s' % (K, S, B, fams))


# ----------------------------------------------------------------------------------------------------------------------------
# a model whose batch-norm state (renderer included) is not the initial one
# ----------------------------------------------------------------------------------------------------------------------------
MAP_GAIN = 100.0


def perturbed_all(cfg, S, seed=11):
    """test_detector_gpu.perturbed_variables (both encoders) extended to the renderer: the renderer's moving statistics near the
    batch statistics of a calibration joint run through O.renderer in training mode, its final bias moved off zero like the other
    biases (N(0, 0.05)).  At its initial weights the renderer barely looks at the K map channels of its 8f + K inputs, so their
    filter rows in conv_1 are scaled by MAP_GAIN: the rendered image then depends on the landmarks strongly enough that wrong maps
    (axis order, width, mode) move it by several times the parity bound (test_render_at_shifted_landmarks_matches_oracle checks
    that on the oracle itself)."""
    P, St = perturbed_variables(cfg, S, seed)
    rng = np.random.default_rng(seed + 1)
    n = len(O.renderer_spec(cfg, S, O.n_renderer_out(cfg)))
    sc_last = 'model/renderer/conv_%d' % n
    P[sc_last + '/b'] = torch.from_numpy((rng.standard_normal(P[sc_last + '/b'].numel()) * 0.05).astype(np.float32))
    w1 = P['model/renderer/conv_1/w'].clone()
    w1[:, :, 8 * cfg.n_filters:, :] *= MAP_GAIN
    P['model/renderer/conv_1/w'] = w1
    calib = O.synthetic_inputs(4, S, seed=seed)
    ctx = O._Ctx(P, St, True)
    with torch.no_grad():
        O.model_forward(ctx, calib['image'], calib['future_image'], cfg)
    for i in range(n - 1):
        sc = 'model/renderer/conv_%d' % (i + 1)
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
    P, St = perturbed_all(cfg, S)
    eng = model._get_engine(B, S)
    eng.load_parameters(P, {k: v for k, v in St.items() if '/moving_' in k})
    return cfg, model, eng, P, St


@pytest.fixture(scope='module')
def m128(ops):
    return make_model(10, 128, 4)


def rel_l2(a, ref):
    """|a - ref| / |ref - its per-image, per-channel mean|: relative to the image content, not to a constant offset."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / (ref - ref.mean((-3, -2), keepdim=True)).norm())


def check_content(pred):
    """Every image of every channel varies over the image (not a constant, not bias alone)."""
    std = pred.detach().double().cpu().std((-3, -2))
    assert float(std.min()) > 1e-2, std


def check_joint_maps(gen, mu):
    """The maps the render stage wrote into joint channels [8f, 8f + K) of its last bucket == O.gaussian_maps of the landmarks it
    was given (16 x 16, 1 / gauss_std, the configured mode, (y, x) order) within one 16-bit ulp."""
    n = mu.shape[0]
    got = gen._joint[:n, ..., gen.C8:gen.C8 + gen.K].float().cpu()
    ref = O.gaussian_maps(mu.detach().float().cpu(), [16, 16], 1.0 / float(gen.cfg.gauss_std), mode=gen.cfg.gauss_mode)
    ulp = 2.0 ** (-7 if gen.dt == torch.bfloat16 else -10)
    err = (got - ref).abs()
    assert bool((err <= ulp * ref.abs() + 1e-7).all()), 'joint maps vs O.gaussian_maps: max err %.3g' % float(err.max())
    assert float(ref.max()) > 0.3                                      # the maps are not all ~0 (grid spacing 2/15)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. parity
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,S,B,dt', [(10, 128, 32, torch.bfloat16), (10, 128, 8, torch.float16), (50, 128, 8, torch.bfloat16),
                                      (30, 256, 4, torch.bfloat16)], ids=['k10_bf16_b32', 'k10_f16', 'k50', 's256_k30'])
def test_reconstruct_matches_oracle_and_eval_path(ops, K, S, B, dt):
    cfg, model, eng, P, St = make_model(K, S, B, dt)
    x, y = images(B, S, 21), images(B, S, 22)
    _, _, _, t = model.build({'image': x, 'future_image': y}, training_pl=False, output_tensors=True, build_loss=False)
    pred_eval = t['future_im_pred'].clone()
    gen = model.image_generator(S, max_batch=B)
    pred = gen.reconstruct(x.to(DEV), y.to(DEV))
    mu = gen.detector.detect(y)
    torch.cuda.synchronize()
    assert pred.shape == (B, S, S, 3) and pred.dtype == torch.float32
    assert torch.equal(pred, gen.reconstruct(x, y))                    # host input: same bits
    n_or = min(B, 4)                                                    # eval-mode batch norm is per sample: a subset is the same check
    with torch.no_grad():
        out = O.forward(P, St, {'image': x[:n_or], 'future_image': y[:n_or]}, cfg, training=False, build_loss=False)
    e_gen = rel_l2(pred[:n_or], out['future_im_pred'])
    e_eval = rel_l2(pred_eval[:n_or], out['future_im_pred'])
    e_ge = rel_l2(pred, pred_eval)
    bound = 1.25 * e_eval + 1e-3
    print('\nRECONSTRUCT K=%d S=%d B=%d %s: rel L2 (of the image content) gen-oracle %.3e  eval-oracle %.3e  gen-eval %.3e  '
          '(bound %.3e)  min per-channel std %.3f' % (K, S, B, dt, e_gen, e_eval, e_ge, bound,
                                                     float(pred.double().std((1, 2)).min())))
    assert e_gen <= bound and e_ge <= bound
    check_content(pred)
    check_content(out['future_im_pred'])
    check_joint_maps(gen, mu)
    assert float((mu[:n_or].cpu() - out['gauss_yx']).abs().max()) < 1e-3
    if gen.Cj > gen.C8 + gen.K:
        assert float(gen._joint[..., gen.C8 + gen.K:].float().abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# 4. the three calls, 5. landmarks nobody detected
# ----------------------------------------------------------------------------------------------------------------------------
def test_render_transfer_and_reconstruct_agree(m128):
    cfg, model, eng, P, St = m128
    gen = model.image_generator(128, max_batch=4)
    A, Pz = images(4, 128, 31), images(4, 128, 32)
    rec = gen.reconstruct(A, Pz)
    assert torch.equal(gen.render(A, gen.detector.detect(Pz)), rec)
    # every stage runs at bucket 4 here: transfer == reconstruct of the 16 pairs, bit for bit
    runs, det_runs = [], []
    run0, det_run0 = gen._run, gen.detector._run
    gen._run = lambda stage, b: (runs.append(stage), run0(stage, b))
    gen.detector._run = lambda b: (det_runs.append(b), det_run0(b))
    try:
        tr, mu_p = gen.transfer(A, Pz, return_landmarks=True)
    finally:
        del gen._run, gen.detector._run
    assert tr.shape == (4, 4, 128, 128, 3)
    assert runs.count('appearance') == 1 and det_runs == [4]              # each encoder once per bucket, not per pair
    assert runs.count('render') == 4
    assert torch.equal(mu_p, gen.detector.detect(Pz))
    a_idx, p_idx = (torch.from_numpy(i) for i in np.divmod(np.arange(16), 4))
    pairs = gen.reconstruct(A[a_idx], Pz[p_idx]).view(4, 4, 128, 128, 3)
    assert torch.equal(tr, pairs)
    for a in range(4):
        assert torch.equal(tr[a, a], rec[a])
    # other bucket sizes: within the cross-bucket bound
    gen2 = model.image_generator(128, max_batch=128)
    tr2 = gen2.transfer(A[:3], Pz)
    d = rel_l2(tr2, tr[:3])
    print('\nTRANSFER cross-bucket rel L2 %.2e' % d)
    assert d < 1e-2


def test_render_at_shifted_landmarks_matches_oracle(m128):
    cfg, model, eng, P, St = m128
    B = 4
    x, y = images(B, 128, 41), images(B, 128, 42)
    gen = model.image_generator(128, max_batch=B)
    mu0 = gen.detector.detect(y).clone()
    mu = mu0.clone()
    mu[..., 1] += 0.1
    got = gen.render(x, mu)
    check_joint_maps(gen, mu)                      # offset, pixel stride, width, mode and (y, x) order of the render stage's maps
    ctx = O._Ctx(P, St, False)
    inv_std = 1.0 / cfg.gauss_std

    def oracle_render(emb, m, mode=cfg.gauss_mode, inv=inv_std):
        return O.renderer(ctx, torch.cat([emb, O.gaussian_maps(m.cpu(), [16, 16], inv, mode=mode)], dim=-1), cfg, 128)[..., :3]
    with torch.no_grad():
        emb = O.encoder(ctx, x, 'model/image_encoder', cfg)[-1]
        ref = oracle_render(emb, mu)
        ref0 = oracle_render(emb, mu0)
        wrong = {'unshifted': ref0, 'y/x swapped': oracle_render(emb, mu.flip(-1)), 'gauss_std +10 %': oracle_render(emb, mu, inv=inv_std / 1.1),
                 'other mode': oracle_render(emb, mu, mode='flat' if cfg.gauss_mode != 'flat' else 'rot')}
        out = O.forward(P, St, {'image': x, 'future_image': y}, cfg, training=False, build_loss=False)
    _, _, _, t = model.build({'image': x, 'future_image': y}, training_pl=False, output_tensors=True, build_loss=False)
    e_eval = rel_l2(t['future_im_pred'], out['future_im_pred'])
    bound = 1.25 * e_eval + 1e-3
    e = rel_l2(got, ref)
    moves = {k: rel_l2(v, ref) for k, v in wrong.items()}
    print('\nRENDER shifted landmarks: rel L2 gen-oracle %.3e (bound %.3e; eval path on reconstruct %.3e); wrong maps move the '
          'oracle by %s' % (e, bound, e_eval, ', '.join('%s %.3e' % kv for kv in moves.items())))
    assert e <= bound
    # the test can tell: the shift, and each way of getting the maps wrong, moves the oracle's own image by several bounds
    for k, v in moves.items():
        assert v > 3 * bound, (k, v, bound)
    check_content(got)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. batch independence and padding, 7. read-only
# ----------------------------------------------------------------------------------------------------------------------------
def test_batch_independence_padding_and_repeatability(m128):
    cfg, model, eng, P, St = m128
    gen = model.image_generator(128, max_batch=8)
    one_x, one_y = images(1, 128, 5), images(1, 128, 6)
    x, y = images(7, 128, 51), images(7, 128, 52)          # bucket 8, one padded row
    x[3], y[3] = one_x[0], one_y[0]
    a = gen.reconstruct(x, y)
    x2, y2 = images(6, 128, 53), images(6, 128, 54)        # bucket 8, other batchmates, other position
    x2[5], y2[5] = one_x[0], one_y[0]
    assert torch.equal(gen.reconstruct(x2, y2)[5], a[3])
    x8, y8 = torch.cat([x, images(1, 128, 55)]), torch.cat([y, images(1, 128, 56)])    # exact bucket 8
    assert torch.equal(gen.reconstruct(x8, y8)[:7], a)
    assert torch.equal(gen.reconstruct(x, y), a)
    torch.cuda.synchronize()
    assert gen.Cj > gen.C8 + gen.K and float(gen._joint[..., gen.C8 + gen.K:].float().abs().max()) == 0.0


def test_generator_leaves_the_model_untouched(m128):
    cfg, model, eng, P, St = m128
    before = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone())
    gen = model.image_generator(128, max_batch=4)
    x, y = images(5, 128, 61), images(3, 128, 62)
    gen.reconstruct(x[:3], y)
    gen.render(x, torch.zeros(5, 10, 2))
    gen.transfer(x[:2], y)
    gen.transfer([np.zeros((50, 60, 3), np.uint8)], [np.zeros((70, 40, 3), np.uint8)])
    gen.refresh()
    torch.cuda.synchronize()
    after = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone())
    for a, b in zip(before[:2], after[:2]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    for a, b in zip(before[2:], after[2:]):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------------
# 8. checkpoints, 9. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_generator_from_checkpoints(m128, tmp_path):
    from imm_amd.generation import ImageGenerator
    from imm_amd.utils.tf_checkpoint import save_tf_checkpoint
    cfg, model, eng, P, St = m128
    x, y = images(5, 128, 71), images(5, 128, 72)
    live = model.image_generator(128, max_batch=8).reconstruct(x, y)
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, str(tmp_path / 'model.pt'))
    save_tf_checkpoint(eng, str(tmp_path / 'tf' / 'model.ckpt'), with_optimizer=False)
    for path in (str(tmp_path / 'model.pt'), str(tmp_path / 'tf' / 'model.ckpt')):
        gen = ImageGenerator.from_checkpoint(model._config, path, image_size=128, max_batch=8, dtype=torch.bfloat16, device=DEV)
        assert torch.equal(gen.reconstruct(x, y), live), path


def _run_script(path, argv):
    import runpy
    old = sys.argv
    sys.argv = [path] + argv
    try:
        runpy.run_path(path, run_name='__main__')
    finally:
        sys.argv = old


def test_generate_script(m128, tmp_path):
    import yaml
    from PIL import Image
    from imm_amd.generation import ImageGenerator
    cfg, model, eng, P, St = m128
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    base = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'experiments', 'celeba-10pts.yaml')))
    base['training'].update({'datadir': str(tmp_path), 'logdir': str(tmp_path / 'logs')})
    base['model']['perceptual']['net_file'] = 'synthetic'
    conf = str(tmp_path / 'exp.yaml')
    with open(conf, 'w') as f:
        yaml.safe_dump(base, f)
    rng = np.random.RandomState(3)
    dirs = {}
    for name, sizes in (('app', [(218, 178), (128, 128)]), ('pose', [(150, 120), (128, 128), (90, 100)])):
        d = tmp_path / name
        d.mkdir()
        dirs[name] = []
        for i, (h, w) in enumerate(sizes):
            im = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
            Image.fromarray(im).save(d / ('%02d.png' % i))
            dirs[name].append(im)
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    out, npz = str(tmp_path / 'grid.png'), str(tmp_path / 'out.npz')
    _run_script(script, ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', str(tmp_path / 'app'), '--pose-dir',
                         str(tmp_path / 'pose'), '--out', out, '--npz', npz, '--batch-size', '4'])
    from imm_amd.utils.config import load_configs
    gen = ImageGenerator.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    r = np.load(npz)
    assert r['images'].shape == (2, 3, 128, 128, 3)
    np.testing.assert_array_equal(r['images'], gen.transfer(dirs['app'], dirs['pose']).cpu().numpy())
    np.testing.assert_array_equal(r['landmarks'], gen.detector.detect(dirs['pose']).cpu().numpy())
    with Image.open(out) as im:
        assert im.size == (4 * 128, 3 * 128)
    lm = np.stack([np.zeros((10, 2), np.float32), np.full((10, 2), 0.25, np.float32)])
    np.savez(str(tmp_path / 'lm.npz'), landmarks=lm)
    _run_script(script, ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', str(tmp_path / 'app'), '--landmarks',
                         str(tmp_path / 'lm.npz'), '--out', str(tmp_path / 'r.png'), '--npz', npz, '--batch-size', '4'])
    np.testing.assert_array_equal(np.load(npz)['images'], gen.render(dirs['app'], torch.from_numpy(lm)).cpu().numpy())
    assert os.path.exists(str(tmp_path / 'r.png'))
