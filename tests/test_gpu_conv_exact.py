"""-m gpu: the output stage of the dense conv kernels, bit for bit, one pinned kernel at a time.

The four copies of that stage -- conv_epilogue (the generic kernel's direct drain), conv_epilogue_drain (the LDS-staged drain of
the pipe / split-role / window kernels), conv_drain_fast (the lean drain on pre-split tensors) and splitk_reduce_kernel (behind a
K-split launch) -- each apply bias or the border-class biases of in_affine, the per-channel un-scale, ReLU / PReLU, the shortcut
through its own channel offset and format (optionally at (y >> 1, x >> 1)), the store into a channel slice and the second affine
output with its own offset.  The programs of tests/exact_programs.py (epilogue_net, up2_net, ksplit_net) hold integers only, so
every tensor is np.array_equal to the float64 reference (tests/test_exact_programs_cpu.py holds that reference against torch, shows
that one wrong offset, slope, class, K range or shift changes it, and that the un-scale is not 1 throughout).  `conv_counts()` says
which kernel ran each conv and whether the lean drain did.  Maps have 45, 132 and 270 pixels, on two cases also 1 and 128 (ep.case_sizes): the
edges of a 128- or 256-pixel tile.  DESIGN.md section 4 maps each drain and argument to the test ids of this file.
"""
import numpy as np
import pytest

from tests import exact_programs as ep
from tests.util import run_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


_refs = {}              # (program key, size) -> the reference: the weights depend on the key alone, not on variant, io or precision


def check(ctx, net, key, sizes, stride, what):
    """One forward per size: the counts are net.counts, every named tensor equals the reference.  -> {size: (out, out2)}."""
    outs = {}
    for size in sizes:
        fr = ep.frames(ep.frame_seed(size), *ep.frame_size(size, stride))
        ctx.conv_counts(reset=True)
        _refs[key, size] = run_exact(ctx, net, fr, net.names, what, ref=_refs.get((key, size)))
        assert ctx.conv_counts() == net.counts, (what, size, ctx.conv_counts(), net.counts)
        outs[size] = tuple(net.model.read(k) for k in ('out', 'out2') if k in net.tid)
    net.model.free()
    return outs


# (case, variant, precision) wherever csrc/conv_igemm.hip: variant_eligible accepts the variant (ep.variant_eligible mirrors it)
EPI_ITEMS = [(case, v, p) for case in ep.CONV_CASES for v in ep.VARIANTS for p in ep.PRECISIONS if ep.conv_programs(case, v, p)]
UP2_ITEMS = [(case, v, p) for case in ep.UP2_CASES for v in ep.VARIANTS for p in ep.PRECISIONS if ep.up2_programs(case, v, p)]


@pytest.mark.parametrize('case,variant,precision', EPI_ITEMS, ids=['%s-%s-%s' % i for i in EPI_ITEMS])
def test_epilogue(ctx, case, variant, precision):
    """Every epilogue of the case on the pinned kernel, with float32 and with pre-split shortcut / outputs, at every size."""
    for epi, io, sizes in ep.conv_programs(case, variant, precision):
        net = ep.epilogue_net(precision, case, variant, epi, io)
        check(ctx, net, ('epilogue', case, epi), sizes, ep.CONV_CASES[case].get('stride', 1), '%s %s %s %s %s' % (case, variant, precision, epi, io))


@pytest.mark.parametrize('case,variant,precision', UP2_ITEMS, ids=['%s-%s-%s' % i for i in UP2_ITEMS])
def test_shortcut_upsampled_x2(ctx, case, variant, precision):
    """res_up2: the shortcut is ceil(h / 2) x ceil(w / 2) and read at (y >> 1, x >> 1), on odd and even maps."""
    for epi, io, sizes in ep.up2_programs(case, variant, precision):
        net = ep.up2_net(precision, case, variant, epi, io)
        check(ctx, net, ('up2', case, epi), sizes, 1, 'up2 %s %s %s %s %s' % (case, variant, precision, epi, io))


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('variant', ep.KSPLIT_VARIANTS)
@pytest.mark.parametrize('case', sorted(ep.KSPLIT_CASES))
def test_k_split(ctx, case, variant, precision):
    """K in 2 and 4 ranges: splitk_reduce_kernel runs ReLU, PReLU, shortcut, shortcut + second output and the border-class biases."""
    for epi, ks, io in ep.ksplit_programs(case, precision):
        net = ep.ksplit_net(precision, case, variant, epi, ks, io)
        sizes = ep.KSPLIT_SIZES + ((ep.AFFINE_SIZE,) if ep.KSPLIT_EPILOGUES[epi].get('affine') else ())
        check(ctx, net, ('ksplit', case, epi, ks), sizes, 1, 'k_split %d %s %s %s %s %s' % (ks, case, variant, precision, epi, io))


AGREE_SIZES = ((3, 5, 3), (3, 9, 10))


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('case', [c for c in ep.CONV_CASES if len({i[1] for i in EPI_ITEMS if i[0] == c}) > 1])
def test_variants_agree(ctx, case, precision):
    """'out' and 'out2' of every kernel that can run the case are the same bits (pre-split tensors where the precision has them): if
    test_epilogue fails, this says whether one kernel or the reference is the odd one out."""
    stride = ep.CONV_CASES[case].get('stride', 1)
    for epi in ep.CONV_CASES[case]['epi']:
        got = {}
        for v in ep.VARIANTS:
            listed = [(io, sizes) for e, io, sizes in ep.conv_programs(case, v, precision) if e == epi]
            if listed:
                io, sizes = listed[-1]
                net = ep.epilogue_net(precision, case, v, epi, io)
                got[v] = check(ctx, net, ('epilogue', case, epi), [s for s in AGREE_SIZES if s in sizes], stride, 'agree %s %s %s %s' % (case, v, precision, epi))
        first = next(iter(got))
        assert len(got) > 1
        for v, outs in got.items():
            for size, tensors in outs.items():
                assert all(np.array_equal(a, b) for a, b in zip(tensors, got[first][size])), (case, epi, precision, v, 'differs from', first, size)
