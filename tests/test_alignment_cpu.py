"""Alignment, host side (no GPU): the fit matrices F of the three models against known maps and against direct f64 least squares
(tests/alignment_reference.py), the template's Procrustes refinement, its file format and its degenerate inputs, the Alignment
object's point maps, and the ABI of the two new entry points."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as R                                             # noqa: E402

from imm_amd import alignment as AL                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (10, 30, 64)


def coef_of(tpl, mu, model, lam=0.0):
    F = tpl.fit_matrix(model, lam)
    assert F.dtype == np.float64 and F.shape == (2 * AL.n_basis(model, tpl.K), 2 * tpl.K)
    return (F @ np.asarray(mu, np.float64).reshape(-1)).reshape(-1, 2)


def random_template(K, seed):
    return AL.LandmarkTemplate(np.random.RandomState(seed).uniform(-0.8, 0.8, size=(K, 2)), 128)


@pytest.mark.parametrize('K', KS)
def test_similarity_and_affine_return_known_maps(K):
    rng = np.random.RandomState(K)
    tpl = random_template(K, K + 1)
    t = tpl.points
    # a similarity: rotation by th, scale s, shift b (complex a = s e^{i th} on y + ix)
    th, s, b = 0.7, 1.3, np.array([0.11, -0.23])
    ar, ai = s * np.cos(th), s * np.sin(th)
    want = np.array([b, [ar, ai], [-ai, ar]])
    mu = R.basis_at(t, t, False).T @ want
    for model in ('similarity', 'affine'):
        got = coef_of(tpl, mu, model)
        assert np.abs(got - want).max() < 1e-12, (model, np.abs(got - want).max())
    # a general affine map returns itself under affine; similarity gives the least-squares similarity of the reference
    want = np.array([[0.05, -0.1], [0.9, 0.3], [-0.4, 1.2]])
    mu = R.basis_at(t, t, False).T @ want
    assert np.abs(coef_of(tpl, mu, 'affine') - want).max() < 1e-12
    assert np.abs(coef_of(tpl, mu, 'similarity') - R.fit(t, mu, 'similarity')).max() < 1e-12
    # noisy landmarks: F is the least-squares fit of the restatement
    mu = mu + rng.standard_normal(mu.shape) * 0.08
    for model in ('similarity', 'affine'):
        assert np.abs(coef_of(tpl, mu, model) - R.fit(t, mu, model)).max() < 1e-11, model
    # fit() is F applied to a batch
    batch = np.stack([mu, mu[::-1]])
    assert np.allclose(tpl.fit(batch, 'affine')[1], coef_of(tpl, mu[::-1], 'affine'), atol=1e-14)


@pytest.mark.parametrize('K', KS)
def test_tps_interpolates_at_lam_zero(K):
    t = R.jittered_grid_template(K, K)
    tpl = AL.LandmarkTemplate(t, 128)
    cond = R.tps_system_cond(t)
    assert cond <= 2e3, cond
    mu = t + np.random.RandomState(K + 7).standard_normal(t.shape) * 0.08
    coef = coef_of(tpl, mu, 'tps')
    assert coef.shape == (K + 3, 2)
    err = np.abs(R.apply_map(t, coef, t) - mu).max()
    print('\ntps lam=0 K=%d: cond(L) %.3g, interpolation error %.3g' % (K, cond, err))
    assert err < 1e-9
    assert np.abs(coef - R.fit(t, mu, 'tps')).max() < 1e-9
    # the side conditions: the radial coefficients sum to zero and are orthogonal to the template
    assert np.abs(coef[:K].sum(0)).max() < 1e-9 and np.abs(t.T @ coef[:K]).max() < 1e-9
    # the template's own basis is the restatement's
    assert np.abs(tpl.basis('tps', 16) - R.basis_at(t, R.grid(16), True)).max() < 1e-13
    assert np.abs(tpl.basis('affine', 16) - R.basis_at(t, R.grid(16), False)).max() == 0
    for lam in (1e-3, 0.1):
        assert np.abs(coef_of(tpl, mu, 'tps', lam) - R.fit(t, mu, 'tps', lam)).max() < 1e-9


@pytest.mark.parametrize('K', (30, 64))
def test_tps_with_large_lam_tends_to_affine(K):
    t = R.jittered_grid_template(K, K + 100)
    tpl = AL.LandmarkTemplate(t, 128)
    mu = t + np.random.RandomState(K).standard_normal(t.shape) * 0.08
    c = coef_of(tpl, mu, 'tps', 1e6)
    a = coef_of(tpl, mu, 'affine')
    print('\ntps lam=1e6 K=%d: |affine part - affine| %.3g, |radial| %.3g' % (K, np.abs(c[K:] - a).max(), np.abs(c[:K]).max()))
    assert np.abs(c[K:] - a).max() < 1e-6
    assert np.abs(c[:K]).max() < 1e-6


def test_similarity_does_not_reflect():
    tpl = random_template(12, 3)
    t = tpl.points
    mu = t * np.array([1.0, -1.0])                     # mirrored left-right
    c = coef_of(tpl, mu, 'similarity')
    lin = c[1:3]                                       # rows q_y, q_x of (y, x)
    assert np.linalg.det(lin) >= 0, 'similarity produced a reflection'
    assert abs(lin[0, 0] - lin[1, 1]) < 1e-14 and abs(lin[0, 1] + lin[1, 0]) < 1e-14      # rotation-scale structure
    assert np.linalg.det(coef_of(tpl, mu, 'affine')[1:3]) < 0                                # affine follows the mirror


def test_from_landmarks_procrustes_recovers_the_base_shape():
    rng = np.random.RandomState(0)
    base = rng.uniform(-0.5, 0.5, size=(10, 2))
    base -= base.mean(0)
    z = base[:, 0] + 1j * base[:, 1]
    shapes = []
    for _ in range(25):                                # poses in symmetric fours: mean scale 1, mean rotation 0, mean shift 0
        s, th, b = rng.uniform(0.7, 1.0), rng.uniform(0.3, 1.0), (rng.uniform(-0.2, 0.2) + 1j * rng.uniform(-0.2, 0.2))
        for ss, tt, bb in ((s, th, b), (s, -th, b), (2 - s, th, -b), (2 - s, -th, -b)):
            shapes.append(ss * np.exp(1j * tt) * z + bb)
    mu = np.stack([np.stack([w.real, w.imag], 1) for w in shapes])
    plain = AL.LandmarkTemplate.from_landmarks(mu, 128, procrustes_iterations=0)
    assert np.abs(plain.points - mu.mean(0)).max() == 0
    refined = AL.LandmarkTemplate.from_landmarks(mu, 128, procrustes_iterations=3)
    err_plain, err_ref = np.abs(plain.points - base).max(), np.abs(refined.points - base).max()
    print('\nProcrustes: |plain mean - base| %.3g, |refined - base| %.3g' % (err_plain, err_ref))
    assert err_ref < 1e-9
    assert err_plain > 0.03                            # the plain mean of rotated copies is a shrunken shape
    with pytest.raises(ValueError):
        AL.LandmarkTemplate.from_landmarks(mu, 128, procrustes_iterations=-1)


def test_template_file_and_checks(tmp_path):
    tpl = AL.LandmarkTemplate(R.jittered_grid_template(10, 1), 128, dataset='mafl', checkpoint='model.pt')
    path = str(tmp_path / 'template.npz')
    tpl.save(path)
    back = AL.LandmarkTemplate.load(path)
    assert np.array_equal(back.points, tpl.points) and (back.K, back.S, back.dataset, back.checkpoint) == (10, 128, 'mafl', 'model.pt')
    with np.load(path) as d:
        assert str(d['format']) == AL.FORMAT and int(d['K']) == 10 and int(d['S']) == 128
    tpl.check(10, 128)
    with pytest.raises(ValueError):
        tpl.check(9, 128)
    with pytest.raises(ValueError):
        tpl.check(10, 64)

    class Det(object):
        K, S = 30, 128
    with pytest.raises(ValueError):
        AL.LandmarkTemplate.load(path, detector=Det())
    other = str(tmp_path / 'other.npz')
    np.savez(other, format=np.array('something-else'), points=tpl.points)
    with pytest.raises(ValueError):
        AL.LandmarkTemplate.load(other)
    for bad_model, lam in (('projective', 0.0), ('tps', -1.0), ('affine', 0.5), ('tps', float('nan'))):
        with pytest.raises(ValueError):
            tpl.fit_matrix(bad_model, lam)


def test_degenerate_templates_are_refused():
    pts = R.jittered_grid_template(10, 2)
    twice = pts.copy()
    twice[7] = twice[2] + 1e-8
    with pytest.raises(ValueError, match='coincide'):
        AL.LandmarkTemplate(twice, 128)
    line = np.stack([np.linspace(-0.5, 0.5, 10), 0.3 * np.linspace(-0.5, 0.5, 10) + 0.1], 1)
    with pytest.raises(ValueError, match='collinear'):
        AL.LandmarkTemplate(line, 128)
    with pytest.raises(ValueError):
        AL.LandmarkTemplate(pts[:2], 128)
    with pytest.raises(ValueError):
        AL.LandmarkTemplate(np.zeros((65, 2)), 128)
    # a large lam is no degeneracy: cond(L) is huge, the fit is the affine one
    tpl = AL.LandmarkTemplate(R.jittered_grid_template(64, 3), 128)
    assert R.tps_system_cond(tpl.points, 1e6) > 1e9
    assert np.isfinite(tpl.fit_matrix('tps', 1e6)).all()


@pytest.mark.parametrize('model', ('similarity', 'affine', 'tps'))
def test_alignment_point_maps(model):
    K, S, So = 10, 128, 96
    t = R.jittered_grid_template(K, 4)
    tpl = AL.LandmarkTemplate(t, S)
    rng = np.random.RandomState(5)
    mu = np.stack([t * 0.8 + 0.1 + rng.standard_normal(t.shape) * 0.05 for _ in range(3)])
    geom = np.array([[10, 20, 1.5, 1.2], [-5, 0, 0.7, 0.9], [0, 0, 1, 1]], np.float32)
    al = AL.Alignment(tpl.fit(mu, model).astype(np.float32), geom, mu.astype(np.float32), model, 0.0, tpl, So)
    # the template's own points, as pixels of the aligned image, land on the landmarks' source pixels (exactly for tps at lam = 0)
    pix = (t + 1) / 2 * So
    src = al.to_source(pix)
    want = geom[:, None, :2] + (mu + 1) / 2 * S * geom[:, None, 2:]
    assert src.shape == (3, K, 2)
    if model == 'tps':
        assert np.abs(src - want).max() < 1e-3                    # f32 coefficients
        with pytest.raises(NotImplementedError):
            al.to_aligned(src)
    else:
        assert np.abs(src - want).max() < 0.1 * S                 # a least-squares fit: close, not exact
        back = al.to_aligned(src)
        assert np.abs(back - pix[None]).max() < 1e-9
        pts = rng.uniform(0, So, size=(3, 7, 2))
        assert np.abs(al.to_aligned(al.to_source(pts)) - pts).max() < 1e-9
    # to_source is the restatement's map
    c = (R.apply_map(t, np.asarray(al.coef[1], np.float64), -1 + 2 * pix / So) + 1) / 2 * S
    assert np.abs(src[1] - (geom[1, :2] + c * geom[1, 2:])).max() < 1e-9


def test_abi_of_the_alignment_entry_points():
    from imm_amd import _lib as L
    main = open(os.path.join(ROOT, 'include', 'imm_hip.h')).read()
    assert re.search(r'#define IMM_ABI_VERSION (\d+)', main).group(1) == str(L.ABI_VERSION)
    assert L.ABI_VERSION >= 25 and '#include "imm_align.h"' in main
    header = open(os.path.join(ROOT, 'include', 'imm_align.h')).read()
    declared = sorted(set(re.findall(r'^int\s+(imm_[a-z0-9_]+)\s*\(', header, flags=re.M)))
    assert declared == L.symbols('imm_align.h') == ['imm_align_coeffs', 'imm_align_warp_u8']
    lib = L.load()
    for name in declared:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m is not None, name
        assert len(m.group(1).split(',')) == len(L.signature(name)[1]), name
        assert getattr(lib, name) is not None
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'align.hip')).read().lower()
    for word in ('s_' + 'store', 's_buffer_' + 'store', 's_scratch_' + 'store', 's_' + 'atomic', 's_buffer_' + 'atomic',
                 's_dcache_' + 'wb', 's_dcache_' + 'discard'):
        assert word not in src, word
