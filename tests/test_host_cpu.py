"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol (no compute
calls without a GPU), config/attr-dict behaviour, network specs against the oracle, launch-table helpers."""
import os
import re
import sys

import pytest
import torch

from oracle import imm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from imm_amd import build as B
    from imm_amd import _lib as L
    B.build()
    lib = L.load()
    header = open(os.path.join(ROOT, 'include', 'imm_hip.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|int64_t|const char\*)\s+(imm_[a-z0-9_]+)\s*\(', header, flags=re.M)))
    assert declared == L.symbols('imm_hip.h'), set(declared) ^ set(L.symbols('imm_hip.h'))
    # argument validation happens before any HIP call: exercisable without a device
    assert lib.imm_pack_image(None, None, 0, 10, None) == -1
    assert b'pack_image' in lib.imm_last_error()
    assert lib.imm_bn_bwd_blocks(1000, 24) == -2 and lib.imm_bn_bwd_blocks(1 << 20, 32) > 0
    d = L.ConvDesc(batch=1, hi=8, wi=8, ci=12, ldx=16, ho=8, wo=8, co=8, ldy=8, kh=3, kw=3, stride=1, pad_t=1, pad_l=1,
                   updiv=1, kpad=128, flags=0, ldmask=0)
    assert lib.imm_conv_stats_blocks(d) == -1 and b'multiple of 8' in lib.imm_last_error()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from imm_amd import _lib as L
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setattr(L, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(L.ImmHipError):
        L.load()


def test_product_package_never_imports_the_oracle():
    for dirpath, _d, files in os.walk(os.path.join(ROOT, 'imm_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(import|from)\s+oracle', src, flags=re.M), os.path.join(dirpath, f)
                assert 'imm_oracle' not in src and 'np_ref' not in src, os.path.join(dirpath, f)
    src = open(os.path.join(ROOT, 'scripts', 'train.py')).read() if os.path.exists(os.path.join(ROOT, 'scripts', 'train.py')) else ''
    assert 'import oracle' not in src and 'from oracle' not in src
    # tools/ and scripts/ are product-side utilities: they may not pull the checker in either
    for sub in ('tools', 'scripts'):
        for f in os.listdir(os.path.join(ROOT, sub)):
            if f.endswith('.py'):
                src = open(os.path.join(ROOT, sub, f)).read()
                assert not re.search(r'^\s*(import|from)\s+oracle', src, flags=re.M), os.path.join(sub, f)


def test_box_and_config_loader(tmp_path):
    from imm_amd.utils.box import Box
    from imm_amd.utils.config import load_configs
    b = Box({'a': {'b': 1}, 'l': [{'c': 2}]})
    assert b.a.b == 1 and b.l[0].c == 2 and hasattr(b, 'a') and not hasattr(b, 'zzz')
    b.x = {'y': 3}
    assert b.x.y == 3 and b.to_dict()['x'] == {'y': 3}
    p1, p2 = tmp_path / 'paths.yaml', tmp_path / 'exp.yaml'
    p1.write_text('logdir: data/logs\nvgg16_path: data/models/vgg16.caffemodel.h5\nnum: 7\n')
    p2.write_text('name: e1\ntraining:\n  logdir: ${logdir}/${name}\n  n: ${num}\nmodel:\n  perceptual:\n    net_file: ${vgg16_path}\n')
    c = load_configs([str(p1), str(p2)])
    assert c.training.logdir == 'data/logs/e1' and c.training.n == 7 and c.model.perceptual.net_file.endswith('.h5')


def test_shipped_reference_configs_parse_if_present():
    """The experiment files under configs/ (the reference's six experiments, same keys and values) through the loader."""
    ref = os.path.join(ROOT, 'configs')
    from imm_amd.utils.config import load_configs
    for exp in sorted(os.listdir(os.path.join(ref, 'experiments'))):
        c = load_configs([os.path.join(ref, 'paths', 'default.yaml'), os.path.join(ref, 'experiments', exp)])
        assert c.model.gauss_mode == 'rot' and c.model.n_filters == 32 and c.training.batch == 50
        assert c.training.logdir.startswith('data/logs/') and '${' not in str(c.to_dict())


def test_network_specs_match_oracle():
    from imm_amd import engine as E
    from imm_amd.utils.box import Box
    for K, S, total in ((10, 128, 4138067), (30, 128, 4189287), (50, 128, 4240507), (30, 256, 4201959)):
        cfg = O.default_model_config(K)
        spec = E.trainable_spec(Box(dict(cfg)), S)
        P, _ = O.init_params(cfg, S)
        assert [n for n, _s, _w in spec] == list(P.keys())
        assert all(tuple(P[n].shape) == tuple(s) for n, s, _w in spec)
        assert sum(int(torch.tensor(s).prod()) for _n, s, _w in spec) == total
        assert all((w == 1e-5) == n.endswith('/w') for n, _s, w in spec)
        assert E.render_sizes(Box(dict(cfg)), S) == O.render_sizes(cfg, S)
        assert E.renderer_spec(Box(dict(cfg)), S, 9) == O.renderer_spec(cfg, S, 9)
    # seeded initialisation is bit-identical to the oracle's (same generator, same draw order)
    import numpy as np
    rng = np.random.default_rng(1)
    P, _ = O.init_params(O.default_model_config(10), 128)
    first = E.truncated_normal(rng, (7, 7, 3, 32), 0.01)
    assert np.array_equal(first, P['model/image_encoder/encoder/conv_1/w'].numpy())
    w = E.synthetic_vgg_weights(2)
    _, St = O.init_params(O.default_model_config(10), 128)
    assert all(torch.equal(w[k], St[k]) for k in w)


def test_segment_and_job_tables_on_cpu():
    from imm_amd import ops
    tab = ops.SegmentTable([10, 20000, 3], [1e-5, 0.0, 0.0], 'cpu')
    assert tab.nseg == 3 and tab.total == 20013 and tab.offsets == [0, 10, 20010, 20013]
    ch = ops.SegmentTable.CHUNK
    mid = list(range(10, 20010, ch))
    assert tab.seg_first_blk.tolist() == [0, 1, 1 + len(mid), 2 + len(mid)] and tab.blk_begin.tolist() == [0] + mid + [20010]
    assert tab.blk_end.tolist() == [10] + mid[1:] + [20010, 20013] and tab.blk_seg.tolist() == [0] + [1] * len(mid) + [2]
    jt = ops.JobTable([(1, 2, 3), (4, 5, 6)], [5000, 10], 2048, 'cpu')
    assert jt.blk_first.tolist() == [0, 3, 4] and jt.n_blocks == 4 and jt.jobs.shape == (2, 12)
    assert ops.same_pad_before(128, 3, 2) == (0, 64) and ops.same_pad_before(128, 7, 1) == (3, 128)
    d = ops.dgrad_desc(2, 128, 128, 32, 32, 64, 64, 3, 2, 0)
    assert (d.hi, d.ho, d.updiv, d.stride, d.pad_t, d.ci, d.co, d.kpad) == (64, 128, 2, 1, 2, 64, 32, 576)
    d = ops.fwd_desc(2, 128, 128, 32, 32, 32, 32, 7, 1, 0, kw=1)
    assert (d.kh, d.kw, d.pad_t, d.pad_l, d.kpad) == (7, 1, 3, 0, 224)


def test_split_inputs_is_an_even_batch_split():
    from imm_amd.train.cnn_train_multi import split_inputs
    inp = O.synthetic_inputs(4, 64)
    parts = [split_inputs(inp, 2, i) for i in range(2)]
    assert all(p['image'].shape[0] == 2 for p in parts)
    assert torch.equal(torch.cat([p['future_image'] for p in parts]), inp['future_image'])
    with pytest.raises(AssertionError):
        split_inputs(O.synthetic_inputs(3, 64), 2, 0)


def test_ab_build_switches(tmp_path, monkeypatch):
    """IMM_HIPCC_FLAGS (diagnosis builds) changes the source digest, so such a build is never mistaken for the production
    library; IMM_HIP_LIB points the binding at another build of the same ABI (A/B timing on one box)."""
    import shutil
    import subprocess
    from imm_amd import build as B
    d0 = B.source_digest()
    monkeypatch.setenv('IMM_HIPCC_FLAGS', '-DIMM_HDEEP_PROFILE')
    assert B.source_digest() != d0
    monkeypatch.delenv('IMM_HIPCC_FLAGS')
    assert B.source_digest() == d0
    other = str(tmp_path / 'libimm_other.so')
    shutil.copy(B.LIB, other)
    code = "from imm_amd import _lib as L; h = L.load(); print(L.LIB_PATH); print(h.imm_abi_version())"
    env = dict(os.environ, IMM_HIP_LIB=other)
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    lines = out.stdout.decode().split()
    from imm_amd import _lib as L
    assert lines[0] == other and int(lines[1]) == L.ABI_VERSION


def test_every_entry_point_named_in_the_documents_exists():
    """INTEGRATION.md, DESIGN.md and README.md may only name `imm_*` entry points the header declares (round 3's INTEGRATION.md still
    listed two that had been removed).  A name passes when it is an exported symbol or a documented prefix / family form of one
    (`imm_graph_`, `imm_upsample2x_fwd/bwd` -> `imm_upsample2x_fwd`); names of modules, files and fixtures are listed here."""
    import re
    hdr = open(os.path.join(ROOT, 'include', 'imm_hip.h')).read()
    exported = set(re.findall(r'\b(imm_[a-z0-9_]+)\s*\(', hdr))
    types = set(re.findall(r'\b(imm_[a-z0-9_]+)\b', hdr)) - exported            # enums / structs / struct fields
    not_abi = {'imm_amd', 'imm_hip', 'imm_model', 'imm_oracle', 'imm_step_golden', 'imm_ref_cpu', 'imm_pmc_', 'imm_mi355x'}
    bad = []
    for doc in ('INTEGRATION.md', 'DESIGN.md', 'README.md'):
        text = open(os.path.join(ROOT, doc)).read()
        for name in sorted(set(re.findall(r'\bimm_[a-z0-9_]+', text))):
            if name in exported or name in types or name in not_abi or name.rstrip('_') in not_abi:
                continue
            if any(e.startswith(name) for e in exported):       # family / prefix forms
                continue
            bad.append((doc, name))
    assert not bad, bad
    assert len(exported) == 93 and ('%d entry points' % len(exported)) in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_reference_import_paths_resolve_to_the_product_modules():
    """SURVEY.md §8b / VERDICT r4: the reference's callers import `imm.models.imm_model`, `imm.train.cnn_train_multi`,
    `imm.utils.box`, `imm.utils.dataset_import`, `imm.eval.eval_imm` (scripts/train.py:13-19, scripts/test.py, eval_imm.py:14-15).
    The `imm` alias package hands out the imm_amd modules themselves (one module object, shared class state)."""
    from imm.models.imm_model import IMMModel
    import imm.train.cnn_train_multi as tru
    from imm.utils.box import Box
    from imm.utils.dataset_import import import_dataset
    from imm.eval import eval_imm
    import imm.datasets.tps_dataset as tpsd
    import imm_amd.models.imm_model as M
    import imm_amd.train.cnn_train_multi as T
    import imm_amd.datasets.tps_dataset as D
    assert IMMModel is M.IMMModel and tru is T and tpsd is D
    assert Box is __import__('imm_amd.utils.box', fromlist=['Box']).Box
    assert callable(import_dataset) and hasattr(eval_imm, 'evaluate')
    for name in ('setup_training', 'average_gradients', 'train_loop'):
        assert hasattr(tru, name), name
    n0 = M.IMMModel.num_instances
    assert IMMModel.num_instances == n0               # the class counter of base_model.py:19,31 is one counter


def test_wgrad_chunk_planner_counts_launch_slots_like_the_library():
    """a chunk of the multi-problem filter-gradient launch holds <= 64 jobs and <= 16 LAUNCH SLOTS, where every job
    of the generic kernel (variant key < 100000) is a slot of its own and every other variant group is one slot."""
    from collections import OrderedDict
    from imm_amd.engine import plan_wgrad_chunks

    def slots(chunk):
        return sum(len(m) if gk[0] // 100000 == 0 else 1 for gk, m in chunk)
    g = OrderedDict()
    g[(0, 1)] = list(range(40))                       # 40 generic jobs: 16 + 16 + 8
    g[(200064, 1)] = list(range(100, 170))            # one LDS-halo variant with 70 members
    g[(100128, 2)] = list(range(200, 203))
    chunks = plan_wgrad_chunks(g, 64, 16)
    assert all(slots(c) <= 16 and sum(len(m) for _k, m in c) <= 64 for c in chunks), [(slots(c), sum(len(m) for _k, m in c)) for c in chunks]
    flat = [j for c in chunks for _k, m in c for j in m]
    assert sorted(flat) == sorted(list(range(40)) + list(range(100, 170)) + list(range(200, 203)))      # every job exactly once
    assert len(chunks) >= 3
    # the ordinary model: 7 variants, 25 jobs -> one chunk
    g2 = OrderedDict(((100000 + i, 1), list(range(4))) for i in range(6))
    assert len(plan_wgrad_chunks(g2, 64, 16)) == 1
    # forced caps (tests/test_step_gpu.py): 5 jobs / 2 variants
    assert all(len(c) <= 2 and sum(len(m) for _k, m in c) <= 5 for c in plan_wgrad_chunks(g2, 5, 2))


def test_upload_and_download_host_side():
    """ops.upload / ops.download (pinned staging + read-back on a GPU: tests/test_kernels_gpu.py) with host destinations: plain copies
    with the same reshape / dtype rules, and a size mismatch raises instead of broadcasting."""
    import numpy as np
    from imm_amd import ops
    src = torch.arange(35.).reshape(7, 5).t()                  # non-contiguous
    dst = torch.empty(35, dtype=torch.float64)
    ops.upload(dst, src, 'x')
    assert torch.equal(dst, src.reshape(-1).double())
    ops.upload(dst, np.arange(35, dtype=np.int32).reshape(5, 7))
    assert torch.equal(dst, torch.arange(35.).double())
    back = ops.download(dst)
    assert torch.equal(back, dst) and back.data_ptr() != dst.data_ptr()
    with pytest.raises(RuntimeError):
        ops.upload(dst, torch.zeros(36))


def test_no_raw_pageable_uploads_in_scripts_and_datasets():
    """`torch.from_numpy(x).to(device)` / `(expr).to(device)` of a host temporary is the pattern behind round 5's torn
    upload (a pageable source above ~1 MB freed right after the asynchronous copy).  Scripts, datasets and the data path put host
    arrays on the device through ops.to_device_pinned / ops.upload / ops.PinnedStager or their own pinned staging ring; this test
    greps for the raw form.  (A `.to(dev, non_blocking=True)` FROM a pinned buffer guarded by an event is the staging ring itself.)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pat = re.compile(r'\.(to\((dev|device|self\.device|d)\b|cuda\(\))')
    allowed = re.compile(r'_staging\[i\]\[:need\]\.to\(dev, non_blocking=True\)')
    bad = []
    for sub in ('scripts', os.path.join('imm_amd', 'datasets'), os.path.join('imm_amd', 'data'), os.path.join('imm_amd', 'eval'),
                os.path.join('imm_amd', 'train')):
        for dirpath, _dirs, files in os.walk(os.path.join(root, sub)):
            for fn in files:
                if not fn.endswith('.py'):
                    continue
                for no, line in enumerate(open(os.path.join(dirpath, fn)), 1):
                    code = line.split('#', 1)[0]
                    if pat.search(code) and not allowed.search(code):
                        bad.append('%s:%d: %s' % (os.path.relpath(os.path.join(dirpath, fn), root), no, line.strip()))
    assert not bad, 'raw host-to-device uploads (use ops.to_device_pinned):\n' + '\n'.join(bad)


def test_pinned_stager_host_side():
    """ops.PinnedStager / ops.to_device_pinned with host destinations: plain copies (the CPU tools and this suite)."""
    import numpy as np
    from imm_amd import ops
    st = ops.PinnedStager()
    dst = torch.empty(5, 7)
    st.copy(dst, torch.arange(35.).reshape(7, 5).t(), 'x')
    assert torch.equal(dst, torch.arange(35.).reshape(7, 5).t())
    t = ops.to_device_pinned(np.arange(6, dtype=np.float64), 'cpu', torch.float32)
    assert t.dtype == torch.float32 and torch.equal(t, torch.arange(6.))


def test_convolution_host_side_has_one_definition_of_each_fact():
    """The private interface between the .hip files lives in csrc/conv_dispatch.h (no file declares an internal imm_* function it
    does not define; every file that defines or calls one of the header's functions includes it), and device properties,
    environment variables and the dynamic-LDS opt-in are each touched in runtime.hip only."""
    csrc = os.path.join(ROOT, 'imm_amd', 'csrc')
    text = {fn: open(os.path.join(csrc, fn)).read() for fn in sorted(os.listdir(csrc)) if fn.endswith(('.hip', '.h'))}
    hips = [fn for fn in text if fn.endswith('.hip')]
    assert 'conv_dispatch.h' in text and len(hips) > 30
    head = re.compile(r'^(?:extern "C" )?(?:static )?(?:inline )?(?:const )?\w+[\w \*&]*?[ \*&](imm_\w+)\(', re.M)

    def functions(src):
        """name -> set of 'decl' / 'def' for every imm_* function head at the start of a line"""
        seen = {}
        for m in head.finditer(src):
            i, depth = m.end(), 1
            while depth:
                depth += {'(': 1, ')': -1}.get(src[i], 0)
                i += 1
            seen.setdefault(m.group(1), set()).add('decl' if src[i:].lstrip()[:1] == ';' else 'def')
        return seen

    assert functions('int imm_a(int (*f)(int));\nextern "C" int imm_b(void) {\n') == {'imm_a': {'decl'}, 'imm_b': {'def'}}
    foreign = ['%s: %s' % (fn, name) for fn in hips for name, kinds in functions(text[fn]).items() if kinds == {'decl'}]
    assert not foreign, 'prototypes of functions defined elsewhere (declare them in conv_dispatch.h / common.h):\n' + '\n'.join(foreign)
    for word, home in (('hipGetDeviceProperties', ['runtime.hip']), ('getenv', ['runtime.hip']), ('hipFuncSetAttribute', ['runtime.hip'])):
        assert [fn for fn in text if word in text[fn]] == home, word
    shared = sorted(functions(text['conv_dispatch.h']))
    assert len(shared) > 40, shared
    uses = re.compile(r'\b(?:%s)\(' % '|'.join(shared))
    missing = [fn for fn in hips if uses.search(text[fn]) and '#include "conv_dispatch.h"' not in text[fn]]
    assert not missing, missing
    defined = {name for fn in hips for name, kinds in functions(text[fn]).items() if 'def' in kinds}
    assert not set(shared) - defined, sorted(set(shared) - defined)


def test_environment_switches_are_the_ones_the_readme_lists():
    """Every IMM_* variable read through os.environ in imm_amd/**/*.py or through getenv in csrc/runtime.hip (the library's only
    file that reads the environment) stands in the switch table of README.md and the table names no other; the engine reads its
    switches in IMMEngine.__init__ and nowhere below it."""
    import ast
    import glob
    read = set()
    for path in glob.glob(os.path.join(ROOT, 'imm_amd', '**', '*.py'), recursive=True):
        read |= set(re.findall(r"""os\.environ(?:\.get\(|\[|\.pop\()\s*['"](IMM_\w+)['"]""", open(path).read()))
        read |= set(re.findall(r"""['"](IMM_\w+)['"]\s+(?:not\s+)?in\s+os\.environ""", open(path).read()))
    read |= set(re.findall(r'getenv\("(IMM_\w+)"\)', open(os.path.join(ROOT, 'imm_amd', 'csrc', 'runtime.hip')).read()))
    readme = open(os.path.join(ROOT, 'README.md')).read()
    table = re.search(r'^\| Switch \|.*?\n((?:\|.*\n)+)', readme, flags=re.M).group(1)
    listed = set(re.findall(r'^\| `(IMM_\w+)`', table, flags=re.M))
    assert len(listed) > 10 and read == listed, (sorted(read - listed), sorted(listed - read))
    src = open(os.path.join(ROOT, 'imm_amd', 'engine.py')).read()
    tree = ast.parse(src)
    init = next(f for c in tree.body if isinstance(c, ast.ClassDef) and c.name == 'IMMEngine'
                for f in c.body if isinstance(f, ast.FunctionDef) and f.name == '__init__')
    lines = src.split('\n')
    outside = [i + 1 for i, l in enumerate(lines) if re.search(r'\benviron\b|\bgetenv\b', l) and not init.lineno <= i + 1 <= init.end_lineno]
    assert not outside, outside
    assert any('environ' in l for l in lines[init.lineno - 1:init.end_lineno])
