"""ImageGenerator host side (imm_amd/generation.py): the variable name list, the batch-norm fold through the whole renderer, the
pair-bucket planner, checkpoint reading, argument checks, the script surface and the product rule that the module never touches the
oracle.  No GPU needed."""
import os
import re
import subprocess
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('bug_fix', [True, False], ids=['channels_bug_fix', 'no_bug_fix'])
@pytest.mark.parametrize('S', [128, 256])
def test_generator_name_list(S, bug_fix):
    from imm_amd.engine import trainable_spec
    from imm_amd.generation import generator_names
    cfg = O.default_model_config(10)
    cfg['channels_bug_fix'] = bug_fix
    params, state = generator_names(cfg, S)
    assert params == [n for n, _s, _w in trainable_spec(cfg, S)]
    P, St = O.init_params(cfg, S, seed=1)
    assert sorted(params) == sorted(k for k in P if not k.startswith('vgg16/'))
    assert sorted(state) == sorted(k for k in St if k.endswith(('/moving_mean', '/moving_variance')))
    assert len(state) == 2 * sum(1 for n in params if n.endswith('/gamma'))
    assert any(n.startswith('model/renderer/') for n in state) and any(n.startswith('model/image_encoder/') for n in state)


def _to64(d):
    return OrderedDict((k, v.double()) for k, v in d.items())


@pytest.mark.parametrize('S,K', [(128, 10), (256, 30)])
def test_folded_renderer_equals_eval_renderer(S, K):
    """In f64: the oracle's renderer in eval mode == the same renderer with every batch norm folded into its convolution and the
    batch norm made the identity (gamma 1, beta 0, moving mean 0, moving variance 1 - eps), within 1e-9 relative.  This pins the
    order fold -> ReLU -> up-sample and the unfolded final layer."""
    from imm_amd.engine import BN_EPS
    from imm_amd.inference import fold_batch_norm
    cfg = O.default_model_config(K)
    cfg['n_filters_render'] = 4                   # a narrow renderer keeps the f64 reference cheap; the order is the same
    cfg['n_filters'] = 4
    P, St = O.init_params(cfg, S, seed=2)
    P, St = _to64(P), _to64(St)
    rng = np.random.default_rng(S + K)
    spec = O.renderer_spec(cfg, S, O.n_renderer_out(cfg))
    for i, (_k, _ci, co, bn, _up) in enumerate(spec):
        sc = 'model/renderer/conv_%d' % (i + 1)
        P[sc + '/b'] = torch.from_numpy(rng.standard_normal(co) * 0.3)
        if bn:
            P[sc + '/gamma'] = torch.from_numpy(rng.uniform(-1.5, 1.5, co))     # negative scales too: the ReLU follows the fold
            P[sc + '/beta'] = torch.from_numpy(rng.standard_normal(co) * 0.3)
            St[sc + '/moving_mean'] = torch.from_numpy(rng.standard_normal(co) * 0.5)
            St[sc + '/moving_variance'] = torch.from_numpy(rng.uniform(0.2, 3.0, co))
    C = 8 * cfg.n_filters + K
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (2, 16, 16, C)))
    with torch.no_grad():
        ref = O.renderer(O._Ctx(P, St, False), x, cfg, S)
        Pf, Sf = OrderedDict(P), OrderedDict(St)
        for i, (_k, _ci, co, bn, _up) in enumerate(spec):
            sc = 'model/renderer/conv_%d' % (i + 1)
            if not bn:
                continue
            wf, bf = fold_batch_norm(P[sc + '/w'], P[sc + '/b'], P[sc + '/gamma'], P[sc + '/beta'], St[sc + '/moving_mean'],
                                     St[sc + '/moving_variance'])
            Pf[sc + '/w'], Pf[sc + '/b'] = torch.from_numpy(wf), torch.from_numpy(bf)
            Pf[sc + '/gamma'], Pf[sc + '/beta'] = torch.ones(co, dtype=torch.float64), torch.zeros(co, dtype=torch.float64)
            Sf[sc + '/moving_mean'] = torch.zeros(co, dtype=torch.float64)
            Sf[sc + '/moving_variance'] = torch.full((co,), 1.0 - BN_EPS, dtype=torch.float64)
        got = O.renderer(O._Ctx(Pf, Sf, False), x, cfg, S)
    assert got.shape == ref.shape == (2, S, S, O.n_renderer_out(cfg))
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert float(ref.std()) > 0


@pytest.mark.parametrize('max_batch', [128, 4, 1])
@pytest.mark.parametrize('A,P', [(1, 1), (3, 5), (16, 16), (7, 40)])
def test_pair_planner_covers_every_pair_once(A, P, max_batch):
    from imm_amd.generation import plan_pairs
    from imm_amd.inference import bucket_sizes
    seen = np.zeros((A, P), dtype=np.int64)
    for start, count, bucket, a_idx, p_idx in plan_pairs(A, P, max_batch):
        assert 1 <= count <= bucket <= max_batch and bucket in bucket_sizes(max_batch)
        assert len(a_idx) == len(p_idx) == count
        np.add.at(seen, (a_idx, p_idx), 1)
    assert (seen == 1).all()


def test_read_variables_pt_and_tf_bundle(tmp_path):
    """The generator's variables from a scripts/train.py `.pt` file and from a TensorFlow bundle written by save_tf_checkpoint are the
    same f32 values, the full name list; a bundle without them is refused; read_checkpoint (the detector's) is unchanged."""
    from imm_amd.generation import generator_names
    from imm_amd.inference import pose_encoder_names, read_checkpoint, read_variables
    from imm_amd.utils.tf_checkpoint import save_tf_checkpoint, write_bundle
    cfg = O.default_model_config(10)
    P, St = O.init_params(cfg, 128, seed=3)
    g = torch.Generator().manual_seed(5)
    St = OrderedDict((k, v + torch.rand(v.shape, generator=g) if k.endswith('moving_variance') else v) for k, v in St.items())
    model_p = OrderedDict((k, v) for k, v in P.items() if not k.startswith('vgg16/'))
    model_s = OrderedDict((k, v) for k, v in St.items() if '/moving_' in k)
    torch.save({'params': model_p, 'state': model_s}, str(tmp_path / 'model.pt'))
    eng = types.SimpleNamespace(named_parameters=lambda: model_p, named_state=lambda: model_s, step_count=torch.tensor(7))
    save_tf_checkpoint(eng, str(tmp_path / 'tf' / 'model.ckpt'), with_optimizer=False)
    pn, sn = generator_names(cfg, 128)
    a = read_variables(str(tmp_path / 'model.pt'), pn + sn, 'generator')
    b = read_variables(str(tmp_path / 'tf' / 'model.ckpt'), pn + sn, 'generator')
    assert list(a) == pn + sn and list(b) == pn + sn
    for k in a:
        assert a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], (P if k in P else St)[k]), k
    pp, ps = read_checkpoint(str(tmp_path / 'model.pt'), 32)
    assert sorted(pp) == sorted(pose_encoder_names(32)[0]) and sorted(ps) == sorted(pose_encoder_names(32)[1])
    write_bundle(str(tmp_path / 'bad' / 'model.ckpt'), {'global_step': np.float32(1)})
    with pytest.raises(KeyError, match='generator'):
        read_variables(str(tmp_path / 'bad' / 'model.ckpt'), pn + sn, 'generator')
    with pytest.raises(FileNotFoundError):
        read_variables(str(tmp_path / 'missing'), pn, 'generator')


def _fake_model(dtype, n_maps=10, **over):
    cfg = O.default_model_config(n_maps)
    cfg.update(over)
    return types.SimpleNamespace(engine=types.SimpleNamespace(dev=torch.device('cpu')), _config=cfg, dtype=dtype)


def test_generator_limits():
    from imm_amd.generation import ImageGenerator
    with pytest.raises(NotImplementedError):
        ImageGenerator(_fake_model(torch.float32))                   # the f32 witness engine has no generator
    with pytest.raises(NotImplementedError):
        ImageGenerator(_fake_model(torch.bfloat16, n_maps=65))       # soft-argmax limit
    with pytest.raises(ValueError):
        ImageGenerator(_fake_model(torch.bfloat16), image_size=72)
    with pytest.raises(NotImplementedError, match='16x16'):
        ImageGenerator(_fake_model(torch.bfloat16, min_res=32))       # the training engine's renderer starts at 16 x 16 only
    with pytest.raises(RuntimeError):
        ImageGenerator(types.SimpleNamespace(engine=None, _config=O.default_model_config(), dtype=torch.bfloat16))


def test_generation_module_never_imports_the_oracle():
    src = open(os.path.join(ROOT, 'imm_amd', 'generation.py')).read()
    assert not re.search(r'^\s*(import|from)\s+oracle', src, flags=re.M)
    assert 'imm_oracle' not in src and 'np_ref' not in src
    code = 'import sys; import imm_amd.generation; print(any(m == "oracle" or m.startswith("oracle.") for m in sys.modules))'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    assert out.stdout.decode().split()[-1] == 'False'


def test_generate_script_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    text = out.stdout.decode()
    for flag in ('--configs', '--checkpoint', '--appearance-dir', '--pose-dir', '--landmarks', '--out', '--npz'):
        assert flag in text, flag
