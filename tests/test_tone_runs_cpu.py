"""No GPU: the conditions tests/test_gpu_tone_runs.py rests on, checked on the models and layouts of tests/tone_run_cases.py.

  * Every batch takes the route it names: run lengths, classes, which runs have no measured member, sparse measured subsets, and
    for the 515-image batch more slots than one head chunk with measured slots behind the chunk's end.
  * Every measured H of a batch differs from every other H of that batch and lies strictly between 1 and k.
  * The doubt band.  The existing tone-map tests allow at most 3 % of a plane's samples within 1 / 256 of a rounding step
    (tonemap_cases.DOUBT).  A 16 x 8 chroma plane has 32 samples -- one sample is 3.1 % -- so the cap cannot be applied per plane to
    these images: it is the same 3 %, pooled over all samples of one batch.  A condition on the inputs, not a measurement of the
    device.
"""
import pytest

from tests import packed_tonemap_cases as K
from tests import tone_run_cases as R
from tests import tonemap_cases as T

DOUBT_CAP = 0.03
TFS = [T.TF_HLG, T.TF_PQ, T.TF_LINEAR]
PLANES = ("vy", "vu", "vv")


@pytest.mark.parametrize("packed", [False, True], ids=["planar", "packed"])
def test_the_layout_takes_the_runs_it_names(packed):
    lay = R.layout(packed)
    assert len(lay) == R.N_LAYOUT
    got = R.runs(lay, by_gamut=not packed)
    assert got == R.LAYOUT_RUNS
    assert got[0][1] == R.CAP                                            # a run that ends at the cap, its size run going on behind it
    assert R.runs(lay, by_gamut=False) == R.LAYOUT_RUNS                  # (the shift and convertYuv: the class break splits 34 | 35, 36 too)
    assert [lay[i].aligned for i, _ in got] == [True, True, False, True, False, True]
    assert (lay[34].w, lay[34].h) == (lay[33].w, lay[33].h) == (lay[35].w, lay[35].h)   # the class break lies inside a size run
    assert packed or (lay[35].gamut != lay[33].gamut and lay[35].gamut == lay[36].gamut)
    measured = [[j for j in range(i, i + m) if not lay[j].given] for i, m in got]
    assert measured[3] == []                                             # a run with no measured member: no pass-1 launch
    assert all(0 < len(ms) < m for ms, (i, m) in zip(measured, got) if m > 2)   # sparse subsets ...
    assert measured[0][:3] == [0, 2, 3] and measured[4] == [38, 39]     # ... that do not start at, or fill, their run
    assert all(lay[i].given for i in range(R.N_LAYOUT) if i % 3 == 1)
    many = R.many(packed)
    assert len(many) == R.N_MANY > R.HEAD_CAP and R.runs(many, by_gamut=not packed) == [(32 * k, 32) for k in range(16)] + [(512, 3)]
    assert [im.given for im in many[512:]] == [False, False, True]
    # a slot shifted by a run or by a head chunk would meet another content or another kind of headroom
    for shift in (R.CAP, R.HEAD_CAP):
        assert all((many[i].content, many[i].given) != (many[i + shift].content, many[i + shift].given) for i in range(R.N_MANY - shift))


def _check_heads(wants, images, k, null):
    heads = [float(w["H"]) for w in wants]
    assert all(1.0 < h < float(k) for h in heads), (min(heads), max(heads), k)
    measured = [h for h, im in zip(heads, images) if null or not im.given]
    assert len(set(measured)) == len(measured) and (null or not set(measured) & {h for h, im in zip(heads, images) if im.given})


@pytest.mark.parametrize("tf", TFS)
def test_planar_batches_meet_the_conditions(tf):
    lay = R.layout(False)
    for null in (False, True):
        wants = [R.planar_expected(im, tf, measured=null) for im in lay]
        _check_heads(wants, lay, T.k_of(tf), null)
        share = R.pooled_doubt(wants, PLANES)
        print("tone-runs planar layout tf %d peaks %s: pooled doubt share %.4f" % (tf, "NULL" if null else "given", share))
        assert share <= DOUBT_CAP
    many = R.many(False)
    wants = [R.planar_expected(im, tf) for im in many]
    assert all(1.0 < float(w["H"]) < float(T.k_of(tf)) for w in wants)
    assert len({float(R.planar_expected(many[c], tf, measured=True)["H"]) for c in range(7)}) == 7
    assert R.pooled_doubt(wants, PLANES) <= DOUBT_CAP
    # the brightest pixel is the one set: the measured H is its, not the ramp's
    flat = T.model(*T.ramp_planes(16, 8, swing=60.0, top=300.0), T.CG_2100, tf)
    assert all(R.planar_expected(im, tf, measured=True)["m"] > flat["m"] for im in lay if (im.w, im.h, im.gamut) == (16, 8, T.CG_2100))


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
def test_packed_batches_meet_the_conditions(form):
    lay = R.layout(True)
    k = T.k_of(form[1])
    for null in (False, True):
        wants = [R.packed_expected(im, form, measured=null) for im in lay]
        _check_heads(wants, lay, k, null)
        share = R.pooled_doubt(wants, ("v",))
        print("tone-runs packed layout %r peaks %s: pooled doubt share %.4f" % (form, "NULL" if null else "given", share))
        assert share <= DOUBT_CAP
    many = R.many(True)
    wants = [R.packed_expected(im, form) for im in many]
    assert all(1.0 < float(w["H"]) < float(k) for w in wants)
    assert len({float(R.packed_expected(many[c], form, measured=True)["H"]) for c in range(7)}) == 7
    assert R.pooled_doubt(wants, ("v",)) <= DOUBT_CAP
    for im in lay:      # the pixel set is the brightest
        img = R.packed_image(form, im.w, im.h, im.content)
        assert K.values(img, form[0]).max() == K.values(img, form[0])[(3 * im.content + 1) % im.h, (5 * im.content + 3) % im.w, im.content % 3]
