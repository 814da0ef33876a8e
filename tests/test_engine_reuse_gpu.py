"""One Engine driven through every host entry point, at changing sizes and in changing order.

The host calls take their device buffers from the context's staging slots: the i-th buffer a call asks for is slot i,
whatever stage asked for it last and however large it was then; the work-list triangulation keeps six buffers of its own
on the context.  What can go wrong there -- two operands of one call in one slot, a slot that did not grow, a counter, flag
or partial sum that nothing in this call wrote, a result read from the stale tail of a larger earlier call -- shows only
when different stages and sizes share a context.  So every result of the shared engine must equal, bit for bit and NaN for
NaN, the result of the identical call on a fresh Engine that has run nothing else.

What an earlier call leaves behind is usually friendly: zeros, or plausible numbers of the same kind.  With
P2S_TUNE_POISON_STAGING the shared engine fills every one of these buffers, over its whole capacity, before the call that
asked for it touches it: with 0xFF (every double and float a NaN, every integer -1, every flag set) and with 0x3F (every
double 4.77e-4, every float 0.747: finite garbage for the kernels that skip NaN).  The stage list is
tests/engine_reuse_cases.py."""
import numpy as np
import pytest

from engine_reuse_cases import LARGE, SMALL, new_engine, stages

pytestmark = pytest.mark.gpu


def differences(got, want):
    """The indices of the arrays of `got` that are not `want`'s in dtype, shape, bits or NaN positions; [-1]: another number of them."""
    if len(got) != len(want):
        return [-1]
    return [i for i, (g, w) in enumerate(zip(got, want))
            if not (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == 'f'))]


@pytest.fixture(scope='module')
def fresh():
    """{(size, name): (first, second)}: every call on an Engine of its own that has run nothing else, and once more on it."""
    out = {}
    for size in (SMALL, LARGE):
        for name, call in stages(size):
            eng = new_engine()
            out[size, name] = (tuple(call(eng)), tuple(call(eng)))
            eng.close()
    return out


def test_every_stage_repeats_itself_on_a_fresh_engine(fresh):
    """The premise of the comparison below: the same call twice on a fresh engine gives the same bits."""
    differing = [key + (differences(first, second),) for key, (first, second) in fresh.items() if differences(first, second)]
    assert differing == []


def test_the_poison_byte_is_checked():
    from pose2sim_amd import _lib
    from pose2sim_amd.engine import Engine
    eng = new_engine()
    for value in (-2, 256):
        with pytest.raises(_lib.P2sError, match='poison byte'):
            eng.set_tuning(Engine.TUNE_POISON_STAGING, value)
    for value in (0, 255, -1):
        eng.set_tuning(Engine.TUNE_POISON_STAGING, value)
    eng.close()


@pytest.mark.parametrize('poison', [None, 0xFF, 0x3F])
def test_one_engine_through_every_stage_and_size(fresh, poison):
    """Small shapes, the same calls at three times the frames (every slot grows), the small shapes again in reverse
    order (every slot now holds the stale tail of a larger call of another stage) -- as the calls left the buffers, and with
    every buffer poisoned before each call."""
    from pose2sim_amd.engine import Engine
    eng = new_engine()
    if poison is not None:
        eng.set_tuning(Engine.TUNE_POISON_STAGING, poison)
    differing = []
    for rnd, (size, order) in enumerate(((SMALL, 1), (LARGE, 1), (SMALL, -1))):
        for name, call in stages(size)[::order]:
            for index in differences(tuple(call(eng)), fresh[size, name][0]):
                differing.append((poison, rnd, name, index))
                print('differs (poison, round, stage, array):', differing[-1])
    eng.close()
    assert differing == []
