"""CPU tests (no GPU): the cases of tests/detector_heads.py are what tests/test_gpu_detector_post.py takes them for.

Per case: every head value is a multiple of 2^-6 and exact in float32; the candidate count is the intended one; the kernel's run
length per thread lies in the intended regime; no score is closer than 1e-4 to the threshold (the float softmax is good to ~1e-7, so
no decision hangs on expf's last bit) except the class that scores exactly 0.5 under threshold 0.5; and NMS really suppresses.
Then four deliberately wrong references, each of which must differ from the true one on a listed case."""
import numpy as np
import pytest

from terran_amd import lib
from tests import detector_heads as dh

CASES = sorted(dh.CASES)
CHEAP = [c for c in CASES if max(dh.CASES[c].counts or [dh.CASES[c].at_least]) <= 4000]      # the wrong references run their own NMS


def test_the_loader_accepts_the_program():
    P = dh.program()
    lib.check_program(P)
    assert P.tensor_formats()[P.outputs[0]] == dh.pack.FMT_F32 and all(np.all(s == 0) for s in P.tensor_scales())


def test_head_matrices_hold_integers_and_powers_of_two_only():
    for s in dh.STRIDES:
        M, b = dh.head_matrix(s)
        w = np.abs(M[M != 0])
        assert np.all((w == np.rint(w)) | ((np.log2(w) == np.rint(np.log2(w))) & (w >= 2.0 ** -6))), s
        assert np.array_equal(b, np.rint(b))
        assert not M[[6, 7, 10, 11]].any() and not b[[6, 7, 10, 11]].any()           # dw = dh = 0: expf(0) in the decode
    assert len({dh.head_matrix(s)[0].tobytes() for s in dh.STRIDES}) == 3             # no level repeats another


@pytest.mark.parametrize('name', CASES)
def test_case_is_what_it_claims(name):
    case = dh.CASES[name]
    geo, ref = case.geo, dh.reference(case)
    for s in dh.STRIDES:                                   # multiples of 2^-6, exact in float32, far below 2^24
        h = ref['heads'][s]
        assert h.shape == (case.N, 32, geo.fh[s], geo.fw[s])
        assert np.array_equal(h * dh.QUANTUM, np.rint(h * dh.QUANTUM)) and np.abs(h).max() * dh.QUANTUM < 2 ** 20
        assert np.array_equal(h.astype(np.float32).astype(np.float64), h)
    ncand = [int((ref['scores'][i] >= np.float32(case.thr)).sum()) for i in range(case.N)]
    painted = [sum(1 for t, d in p.live.items() if ref['scores'][i][t] >= np.float32(case.thr)) for i, p in enumerate(case.painters())]
    assert ncand == painted                                # nothing passes that the painter did not set
    if case.counts is not None:
        assert ncand == case.counts
    else:
        assert min(ncand) >= case.at_least
    assert geo.perc == -(-geo.ncell // 1024)
    assert {'short': geo.per < 64, 'full': geo.per == 64, 'rescored': geo.per > 64}[case.regime], geo.per
    # every score at least 1e-4 from the threshold, in float64; d == 0 under 0.5 gives 0.5 on both sides
    p64 = 1.0 / (1.0 + np.exp(-ref['d']))
    near = np.abs(p64 - case.thr) < 1e-4
    assert not near.any() or (case.thr == 0.5 and np.all(ref['d'][near] == 0.0))
    assert np.array_equal(ref['scores'] >= np.float32(case.thr), p64 >= case.thr)
    kept = [len(x) for x in ref['dets']]
    for c, k in zip(ncand, kept):
        assert (1 < k < c) if c >= 64 else (k <= c and (k > 0) == (c > 0)), (c, k)
    print('%s: T %d perc %d candidates %s kept %s' % (name, geo.T, geo.perc, ncand, kept))


def test_the_straddling_classes_are_all_there():
    """Per threshold in use: anchors in each failing and each passing class next to it, and the shortcut sees both of its sides."""
    for thr, (fails, passes) in dh.STRADDLE.items():
        seen = set()
        for case in dh.CASE_LIST:
            if case.thr == thr:
                for p in case.painters():
                    seen |= set(p.live.values())
        assert set(fails) | set(passes) <= seen, (thr, sorted(seen))
        lg, m = np.log(thr / (1 - thr)), dh.margin(thr)
        assert all(d / 64.0 < lg for d in fails) and all(d / 64.0 >= lg for d in passes)
        assert fails[0] / 64.0 < m                          # skipped by the shortcut
    assert dh.STRADDLE[0.75][0][1] / 64.0 >= dh.margin(0.75)     # not skipped: the exact test fails it
    assert -1 / 64.0 < dh.margin(0.5) < 0


def test_edges_of_the_walk_are_painted():
    """Last cell of a level and first of the next, both anchors of a cell, one passing beside one failing, ties over all levels."""
    for name, first_of in (('c64', 16), ('c1023', 8), ('c8192', 8), ('c1025', 16)):
        case = dh.CASES[name]
        geo, sc = case.geo, dh.reference(case)['scores'][0] >= np.float32(case.thr)
        last32 = geo.t0[16] - 1
        assert sc[last32] and not sc[last32 - 1]
        assert sc[geo.t0[first_of]] and sc[geo.t0[first_of] + 1]
        assert sc[geo.t0[8] - 2] and not sc[geo.t0[8] - 1] and sc[geo.T - 1]
    case = dh.CASES['c1024']
    ref = dh.reference(case)
    top = ref['d'][0] == dh.TIE_CLASSES[0] / 64.0
    assert all(top[case.geo.t0[s]:].sum() >= 20 for s in dh.STRIDES) and top[:case.geo.t0[16]].sum() >= 20
    case = dh.CASES['per64_offset63']                     # nothing but offset 63 of a run passes
    ok = np.nonzero(dh.reference(case)['scores'][0] >= np.float32(case.thr))[0]
    assert case.geo.per == 64 and np.all(ok % 64 == 63) and len({int(t) // 64 for t in ok}) == len(ok)
    case = dh.CASES['per68_rescored']                     # candidates on both sides of both level hops inside one run, and past offset 63
    geo = case.geo
    for i, s in enumerate((16, 8)):                       # image i lets the pixel (0, 0) speak to level s
        ok = dh.reference(case)['scores'][i] >= np.float32(case.thr)
        b = geo.t0[s]
        k = b // geo.per
        assert k * geo.per < b < (k + 1) * geo.per and ok[k * geo.per:b].any() and ok[b:(k + 1) * geo.per].any() and ok[b:b + 2].any()
        assert (ok & (np.arange(geo.T) % geo.per >= 64)).sum() >= 100


def test_select_of_this_module_is_the_oracle_without_a_mistake():
    for name in ('c65', 'batch3', 'odd_101x150'):
        case = dh.CASES[name]
        assert dh.same_detections(dh.reference(case, 'none')['dets'], dh.reference(case)['dets'])


@pytest.mark.parametrize('mistake', dh.MISTAKES)
def test_wrong_reference_is_caught(mistake):
    caught = [name for name in CHEAP if not dh.same_detections(dh.reference(dh.CASES[name], mistake)['dets'], dh.reference(dh.CASES[name])['dets'])]
    print(mistake, 'differs on', caught)
    assert caught
    if mistake == 'offset63_dropped':
        assert 'per64_offset63' in caught
    if mistake == 'level_hop_late':
        assert 'per68_rescored' in caught
