"""GPU: a stamp, frame or cube call's result does not depend on what ran before it on the same context.

The fifteen entry points behind the staging buffer and the grow-only frame workspaces of stamp_calls.cpp (stage, specx,
render, find, group, framefit, cubefit; the audit is DESIGN.md "Call-order independence", the second table) follow the
protocol of tests/test_gpu_call_history.py: on one context the checked call runs once, so that the workspaces are sized
for it, then a predecessor, then the checked call again -- and every output array of that second run equals, byte for
byte, the same call on a fresh context (a NaN equals itself, -0 differs from +0).  The fresh result is computed once
per module and first held to the entry point's fp64 reference with the helper and the bounds of its own parity test.
The checked calls and the predecessors are those of tests/stamp_history_cases.py: L larger, S smaller, X the other
tenant of the workspace, T another terminal state at the same shape, N non-finite data, F a refused call.  Mixed
precision runs every pair; f64 the whole list of the stamp calls, and L, X and one T of the frame and cube calls, whose
kernels are the same fp64 ones in both modes.

R: a frame or cube call issued while device-output reconstructs are still in flight on both lanes (the wait_for_lanes
path of Staged::run and of fit_cube_psf) equals the fresh call, and the reconstructs equal theirs.

Every documented output is written, and nothing else (include/mpsfr.h, "What a call writes"): each entry point once in
its device form into buffers prefilled with the byte 0xA5 -- every element equals the host form's fresh value, none
still holds the sentinel, and the bytes behind the documented size still do.

Nothing here has a tolerance of its own: everything new is bit equality.
"""
import numpy as np
import pytest

import stamp_history_cases as C
from conftest import H

pytestmark = pytest.mark.gpu

PAIRS = ([('mixed', name, p) for name, labels in C.LABELS.items() for p in labels]
         + [('f64', name, p) for name, labels in C.F64_LABELS.items() for p in labels])


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


_FRESH = {}
_BROKEN = []


class _Gpu:
    """Around the GPU part of a test: an error of the library (a HIP error, a refused legal call) ends the GPU work of
    the module, so that nothing more is started on a device that has faulted."""
    def __enter__(self):
        if _BROKEN:
            pytest.fail('not run: an earlier test of this module ended with %s' % _BROKEN[0])

    def __exit__(self, kind, value, tb):
        if kind is not None and not issubclass(kind, (AssertionError, ValueError, TypeError, KeyError)):
            _BROKEN.append('%s: %s' % (kind.__name__, value))
        return False


def _fresh(api, prec, name):
    """The checked call on a fresh context, held to its fp64 reference (once per module)."""
    if (prec, name) not in _FRESH:
        run, hold = C.CHECKED[name]
        with _Gpu():
            ctx = C.context(api, prec)
            out = run(api, ctx)
            ctx.close()
        hold(api, out, prec)
        _FRESH[prec, name] = out
    return _FRESH[prec, name]


def test_the_labels_are_those_of_the_predecessors():
    P = C.predecessors()
    assert sorted(P) == sorted(C.CHECKED) == sorted(C.LABELS)
    for name in P:
        assert sorted(P[name]) == sorted(C.LABELS[name]), name
        kinds = {p[0] for p in P[name]}
        assert kinds >= set('LSNF') and ('X' in kinds), (name, kinds)
        assert set(C.F64_LABELS[name]) <= set(P[name])


@pytest.mark.parametrize('prec,checked,pred', PAIRS)
def test_checked_call_after_predecessor_equals_fresh(api, prec, checked, pred):
    want = _fresh(api, prec, checked)
    run = C.CHECKED[checked][0]
    with _Gpu():
        ctx = C.context(api, prec)
        run(api, ctx)
        C.predecessors()[checked][pred](api, ctx)
        got = run(api, ctx)
        ctx.close()
    differ = C.differences(checked, pred, got, want)
    assert not differ, '\n'.join(differ)


@pytest.mark.parametrize('checked', list(C.CHECKED))
def test_two_fresh_contexts_agree(api, checked):
    """The control of the comparison above: run-to-run differences that do not depend on a predecessor would show
    here, between two fresh contexts."""
    want = _fresh(api, 'mixed', checked)
    with _Gpu():
        ctx = C.context(api, 'mixed')
        got = C.CHECKED[checked][0](api, ctx)
        ctx.close()
    differ = C.differences(checked, 'nothing (a second fresh context)', got, want)
    assert not differ, '\n'.join(differ)


# ---- R: the lanes
LB = np.array([500.0, 700.0, 900.0])
_ROWS = {}


def _rows(api):
    if not _ROWS:
        see, gl, l0 = api.synthetic_rows(6)
        with _Gpu():
            ctx = C.context(api, 'mixed')
            _ROWS.update(see=see, gl=gl, l0=l0, want=ctx.reconstruct(LB, see, gl, l0, None, H))
            ctx.close()
    return _ROWS


@pytest.mark.parametrize('checked', C.FRAME_CALLS)
def test_checked_call_behind_reconstructs_in_flight(api, checked):
    import torch
    dev = torch.device('cuda:0')
    r = _rows(api)
    n, nl = r['see'].size, LB.size
    want = _fresh(api, 'mixed', checked)
    run = C.CHECKED[checked][0]
    with _Gpu():
        ctx = C.context(api, 'mixed')
        ctx.set_option('streams', 2)
        run(api, ctx)
        outs = []
        for _ in range(2):                       # one per lane, nobody waits
            t = dict(psf=torch.full((n, nl, 40, 40), float('nan'), dtype=torch.float64, device=dev),
                     psf_sum=torch.full((nl, 40, 40), float('nan'), dtype=torch.float64, device=dev),
                     fit=torch.full((n, nl, api.NFIT), float('nan'), dtype=torch.float64, device=dev))
            outs.append(t)
        torch.cuda.synchronize()
        for t in outs:
            ctx.reconstruct_device(LB, r['see'], r['gl'], r['l0'], None, H, None, 1, None, t['psf'].data_ptr(),
                                   t['psf_sum'].data_ptr(), t['fit'].data_ptr())
        got = run(api, ctx)
        ctx.sync()
        torch.cuda.synchronize()
        recs = [{key: v.cpu().numpy() for key, v in t.items()} for t in outs]
        ctx.close()
    differ = C.differences(checked, 'R two reconstructs in flight', got, want)
    for k, rec in enumerate(recs):
        differ += C.differences('reconstruct %d' % k, checked + ' issued behind it', rec, r['want'])
    assert not differ, '\n'.join(differ)


# ---- every documented output is written, and nothing else
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
@pytest.mark.parametrize('checked', list(C.DEVICE))
def test_device_form_writes_every_documented_element_and_nothing_else(api, prec, checked):
    import torch
    want = _fresh(api, prec, checked)
    with _Gpu():
        ctx = C.context(api, prec)
        got, tails = C.device_run(api, ctx, torch, checked)
        ctx.close()
    assert sorted(got) == sorted(want)
    problems = C.differences(checked + ' (device form)', 'nothing', got, want)
    for k in sorted(got):
        left = int(C.holds_sentinel(got[k]).sum())
        if left:
            problems.append('%s: %d elements of output %s still hold the sentinel' % (checked, left, k))
        if tails[k]:
            problems.append('%s: %d bytes behind output %s were written' % (checked, tails[k], k))
    assert not problems, '\n'.join(problems)
