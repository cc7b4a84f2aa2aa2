"""Host: the case table of the background map (tests/background_cases.py) on the reference alone, without a GPU.

1. every case's certificate holds on background_ref.background: the case reaches the path of background.hip it is there
   for.  This is what keeps the GPU parity test over the same table from passing vacuously; a claim that fails is a
   failed test.
2. background_ref.fill_plan, written from ring membership max(|di|, |dj|) == r, agrees with background_ref.layer_mesh,
   written from slices, on which cells are filled and from which values: columns 0 and 1 of every layer of every case
   are recomputed from the plan with med, bit for bit.
3. the whole table evaluates in a few seconds.
"""
import time

import numpy as np
import pytest

import background_cases as K
import background_ref as B


@pytest.mark.parametrize('name', K.NAMES)
def test_the_case_reaches_its_path_on_the_reference(name):
    claims = K.certificate(name)
    assert claims
    for claim, holds in claims:
        print('%s: %s: %s' % (name, claim, 'holds' if holds else 'FAILS'))
    assert all(holds for _, holds in claims), [claim for claim, holds in claims if not holds]


@pytest.mark.parametrize('name', K.NAMES)
def test_fill_plan_agrees_with_layer_mesh(name):
    ref, par = K.reference(name), dict(B.DEFAULTS, **K.inputs(name)['par'])
    h = (par['filter'] - 1) // 2
    for layer, mesh in enumerate(ref['mesh']):
        plan, good, radius, count = K.plan_summary(mesh, par['filter'])
        want = np.full(mesh.shape[:2] + (2,), np.nan)
        for i, row in enumerate(plan):
            for j, (r, cells) in enumerate(row):
                if cells:
                    want[i, j] = [B.med([mesh[c][2] for c in cells]), B.med([mesh[c][3] for c in cells])]
        assert want.tobytes() == np.ascontiguousarray(mesh[..., :2]).tobytes(), (name, layer)
        # a valid cell finds itself in its window; a dead layer has no plan
        assert np.all(radius[good] == h) and ((radius == -1) == (good.sum() == 0)).all()
        assert np.all(count[radius >= 0] >= 1)


def test_fill_plan_written_out_by_hand():
    good = np.zeros((3, 5), dtype=bool)
    good[0, 0] = good[2, 4] = good[2, 3] = True
    plan = B.fill_plan(good, 1)
    assert plan[0][0] == (0, [(0, 0)]) and plan[1][1] == (1, [(0, 0)]) and plan[0][2] == (2, [(0, 0), (2, 3), (2, 4)])
    assert plan[1][4] == (1, [(2, 3), (2, 4)]) and plan[0][4] == (2, [(2, 3), (2, 4)]) and plan[2][0] == (2, [(0, 0)])
    plan = B.fill_plan(good, 3)
    assert plan[1][1] == (1, [(0, 0)]) and plan[0][2] == (2, [(0, 0), (2, 3), (2, 4)])
    assert plan[1][3] == (1, [(2, 3), (2, 4)])
    assert B.fill_plan(np.zeros((2, 2), dtype=bool), 5) == [[(None, [])] * 2] * 2
    # a ring beyond the shorter side of the mesh: rmax is max(my, mx)
    far = np.zeros((1, 9), dtype=bool)
    far[0, 8] = True
    assert B.fill_plan(far, 5)[0][0] == (8, [(0, 8)]) and B.fill_plan(far, 5)[0][6] == (2, [(0, 8)])


def test_the_table_covers_every_family_and_evaluates_in_seconds():
    assert set(K.FAMILIES) == {'wide', 'cells', 'sparse', 'ties', 'sort', 'clip', 'min_frac', 'clamp'}
    K.inputs.cache_clear()
    K.reference.cache_clear()
    t0 = time.perf_counter()
    for name in K.NAMES:
        K.certificate(name)
    spent = time.perf_counter() - t0
    print('%d cases in %.2f s' % (len(K.NAMES), spent))
    assert spent < 20.0                                                  # (about a second; room for a slow host)
