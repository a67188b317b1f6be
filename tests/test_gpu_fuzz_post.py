"""-m gpu: fixed seeds of tests/fuzz_post.py, device against oracle, exact (counts, order, integer outputs, scores).

The seeds were chosen on the CPU from the generators' parameters (fuzz_post.rf_inputs / op_inputs draw them without a GPU);
the tests assert from the returned `info` what the lists are there for, so that an edit cannot empty them: for RetinaFace the
densities 0.0 and 1.0 and all three thresholds, for OpenPose two plateaus (more than 1 024 peaks of one part: the global-memory
re-run) and a frame without people."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RF_SEEDS = (1, 4, 8, 17, 25, 41, 43)
OP_SEEDS = (0, 4, 5, 9, 28, 29, 34)


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def test_retinaface_seeds(ctx):
    from tests import fuzz_post
    infos = []
    for seed in RF_SEEDS:
        ok, info = fuzz_post.rf_case(ctx, np.random.default_rng(seed))
        assert ok, ('retinaface', seed, info)
        infos.append(info)
    assert {0.0, 1.0} <= {i['dens'] for i in infos} and {i['thr'] for i in infos} == {0.5, 0.3, 0.75}
    assert any(i['kept'] == 0 for i in infos) and max(i['kept'] for i in infos) > 100


def test_openpose_seeds(ctx):
    from tests import fuzz_post
    infos = []
    for seed in OP_SEEDS:
        ok, info = fuzz_post.op_case(ctx, np.random.default_rng(seed))
        assert ok, ('openpose', seed, info)
        infos.append(info)
    assert sum('plateau' in i for i in infos) >= 2 and any(i['P'] == 0 for i in infos) and any(i.get('humans', 0) > 0 for i in infos)
