"""What the plan_* functions share, host side (no GPU): the plan base that refuses a missing or unknown field, the one check of a list of
u8 photos and its boxes with every caller's own wording, and the status bits that live in tracking.py."""
import numpy as np
import pytest
import torch

from imm_amd import annotation as AN
from imm_amd import clip as CL
from imm_amd import inference as INF
from imm_amd import morphing as MP
from imm_amd import redaction as RD
from imm_amd import reenact as RE
from imm_amd import tracking as TR
from imm_amd.generation import NEEDS_U8, plan_repose

K = 10
PLANS = [MP.MorphPlan, RD.RedactPlan, AN.AnnotatePlan, CL.ClipPlan, RD.ClipRedactPlan, AN.ClipAnnotatePlan, RE.ReenactPlan]
PHOTOS = [np.full((12, 10, 3), 7, np.uint8), np.full((8, 9), 200, np.uint8)]          # the second one grey
FLOATS = [np.zeros((8, 8, 3), np.float32)]


@pytest.mark.parametrize('cls', PLANS, ids=lambda c: c.__name__)
def test_a_plan_refuses_a_missing_and_an_unknown_field(cls):
    assert issubclass(cls, INF._Plan) and len(set(cls.FIELDS)) == len(cls.FIELDS) > 0
    fields = {name: i for i, name in enumerate(cls.FIELDS)}
    plan = cls(**fields)
    assert all(getattr(plan, name) == i for name, i in fields.items())
    with pytest.raises(AssertionError):
        cls(**{name: v for name, v in fields.items() if name != cls.FIELDS[-1]})
    with pytest.raises(AssertionError):
        cls(misspelt=0, **fields)
    with pytest.raises(AssertionError):                                      # a misspelt field is both
        cls(**{name + ('_' if name == cls.FIELDS[0] else ''): v for name, v in fields.items()})


def test_the_clip_plans_are_made_with_exactly_their_fields():
    frames, faces = [PHOTOS[0]] * 3, [(1, 1, 11, 9)]
    made = [CL.plan_clip(frames, faces, PHOTOS[:1], K=K, max_batch=4), RD.plan_redact_clip(frames, faces, K, max_batch=4),
            AN.plan_annotate_clip(frames, faces, None, K, max_batch=4), RE.plan_reenact(PHOTOS, frames, faces[0], max_batch=4)]
    for plan, cls in zip(made, (CL.ClipPlan, RD.ClipRedactPlan, AN.ClipAnnotatePlan, RE.ReenactPlan)):
        assert type(plan) is cls and set(vars(plan)) == set(cls.FIELDS)
    assert MP.MorphPlan.FIELDS[:3] == ('photos', 'rows', 'donors') and RD.RedactPlan.FIELDS[0] == AN.AnnotatePlan.FIELDS[0] == 'photos'


def test_photos_and_rows_default_is_one_whole_photo_box_per_photo():
    photos, rows = INF.photos_and_rows(PHOTOS, None)
    assert rows.dtype == np.int32 and rows.tolist() == [[0, 0, 0, 12, 10], [1, 0, 0, 8, 9]]
    assert [p.shape for p in photos] == [(12, 10, 3), (8, 9, 3)] and all(p.dtype == np.uint8 and p.flags.c_contiguous for p in photos)
    assert (photos[1] == 200).all()                                          # grey, repeated to three channels
    photos, rows = INF.photos_and_rows(PHOTOS, [(1, 2, 3, 6, 7), (0, 0, 0, 4, 4)])
    assert rows.tolist() == [[1, 2, 3, 6, 7], [0, 0, 0, 4, 4]]
    assert INF.photo_boxes(PHOTOS, None, 16)[2].tolist() == INF.photos_and_rows(PHOTOS, None)[1].tolist()


def test_photos_and_rows_refuses_in_the_callers_words():
    with pytest.raises(ValueError) as e:
        INF.photos_and_rows(torch.zeros(1, 8, 8, 3), None, 'mine: a list')
    assert str(e.value) == 'mine: a list'
    for empty, text in ((None, 'no boxes'), ('mine: none', 'mine: none')):   # without the caller's words check_boxes refuses the empty list
        with pytest.raises(ValueError) as e:
            INF.photos_and_rows([], None, 'mine: a list', empty)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        INF.photos_and_rows(PHOTOS, [(0, 0, 0, 4, 4)] * 3, limit=(2, 'at most 2 rows, got %d'))
    assert str(e.value) == 'at most 2 rows, got 3'
    INF.photos_and_rows(PHOTOS, [(0, 0, 0, 4, 4)] * 2, limit=(2, 'at most 2 rows, got %d'))
    for kind in (TypeError, ValueError):
        with pytest.raises(kind) as e:
            INF.photos_and_rows(FLOATS, None, not_u8=kind)
        assert type(e.value) is kind and str(e.value) == 'image arrays must be uint8 HWC, got float32'


def callers(photos):
    """Every caller of photos_and_rows with `photos` as its list: name -> call."""
    return {'repose': lambda: plan_repose(photos, torch.zeros(1, K, 2), None, None, 0.125, K),
            'morph': lambda: MP.plan_morph(photos, PHOTOS, None, None, 0.5, None, 0.125, K),
            'morph_donors': lambda: MP.plan_morph(PHOTOS, photos, None, None, 0.5, None, 0.125, K),
            'redact': lambda: RD.plan_redact(photos, None, K),
            'annotate': lambda: AN.plan_annotate(photos, None, K),
            'reenact': lambda: RE.plan_reenact(photos, [PHOTOS[0]], (1, 1, 11, 9)),
            'colour_stats': lambda: INF.LandmarkDetector.colour_stats(None, photos)}


def test_every_caller_keeps_its_wording_and_its_type():
    batch = torch.zeros(2, 8, 8, 3)
    no_list = dict(repose=NEEDS_U8, morph='photos: ' + NEEDS_U8, morph_donors='donors: ' + NEEDS_U8, redact='photos: ' + NEEDS_U8,
                   annotate='photos: ' + NEEDS_U8, reenact=NEEDS_U8, colour_stats='photos: ' + NEEDS_U8)
    for name, call in callers(batch).items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == no_list[name], name
    none = dict(no_list, reenact='no photos', repose='no boxes')             # repose leaves the empty list to check_boxes
    for name, call in callers([]).items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == none[name], name
    for name, call in callers(FLOATS).items():
        kind = ValueError if name == 'reenact' else TypeError
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == 'image arrays must be uint8 HWC, got float32', name


def test_check_landmarks():
    lm = INF.check_landmarks(np.zeros((2, K, 2), np.float64), (2,), K)
    assert lm.dtype == torch.float32 and tuple(lm.shape) == (2, K, 2)
    assert INF.check_landmarks(torch.full((1, K, 2), float('nan')), (2, 1), K, 'donor_landmarks').shape[0] == 1
    with pytest.raises(ValueError) as e:
        INF.check_landmarks(np.zeros((3, K, 2)), (2,), K)
    assert str(e.value) == 'landmarks must be [2, %d, 2], got (3, %d, 2)' % (K, K)
    with pytest.raises(ValueError) as e:
        INF.check_landmarks(np.zeros((K, 2)), (2, 1), K, 'donor_landmarks')
    assert str(e.value) == 'donor_landmarks must be [2 or 1, %d, 2], got (%d, 2)' % (K, K)
    for plan in (lambda lm: RD.plan_redact(PHOTOS, None, K, landmarks=lm), lambda lm: AN.plan_annotate(PHOTOS, None, K, landmarks=lm)):
        with pytest.raises(ValueError) as e:
            plan(np.zeros((2, K + 1, 2)))
        assert str(e.value) == 'landmarks must be [2, %d, 2], got (2, %d, 2)' % (K, K + 1)
        assert plan(np.full((2, K, 2), np.nan)).landmarks.dtype == torch.float32          # values that are not finite are not refused


def test_the_status_bits_live_in_tracking():
    assert (TR.FLAG_LOST, TR.FLAG_OUTSIDE, TR.FLAG_UNSURE) == (1, 2, 4)
    assert RD.FLAG_UNSURE is TR.FLAG_UNSURE
    assert AN.FLAG_LOST is TR.FLAG_LOST and AN.FLAG_OUTSIDE is TR.FLAG_OUTSIDE and AN.FLAG_UNSURE is TR.FLAG_UNSURE
    flags, q = torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([0, 2, 0, 1], dtype=torch.int32)
    assert TR.or_unsure(flags, q) is flags and flags.tolist() == [0, 5, 2, 7]
