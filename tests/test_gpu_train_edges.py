"""apd_trainer on the GPU against the literal checker over the case table of tests/_train_cases.py: the defined sigmoid at a few
thousand arguments per call site (every edge of train_exp to the last ulp, every binary exponent), subnormal products, an overflow
inside a dot product, huge frames, zero and subnormal weights, signed zeros at rate 0, Mat::norm where it rescales, rates and
starting weights that are not finite, a weight that is inf a step before any is NaN, run lengths around the prefetch blocks of 8
(shared and per-model orders, continuations), and 512 / 1500 models in one launch.  Every comparison is the one of
tests/test_gpu_train.py: the four matrices, total_err, steps and first_nonfinite, bit for bit through canonical_bits, after every
run of a case.  tests/test_train_cases.py shows on the checker alone that each case reaches what it is named after."""
import numpy as np
import pytest

import _train_cases as cases
from test_gpu_train import assert_equals_checker, autoencoder_bits, ctx, trainer_for  # noqa: F401  (ctx: the module's fixture)

pytestmark = pytest.mark.gpu


def run_case(ctx, name):
    case = cases.get(name)
    with trainer_for(ctx, case.models) as t:
        for r, ((order, alpha), want) in enumerate(zip(case.runs, case.trained())):
            t.run(case.frames, order, alpha)
            assert_equals_checker(t, want, "%s, run %d of %d" % (name, r + 1, len(case.runs)))
        return [(autoencoder_bits(t.weights(m)).tobytes(), repr(t.totals()[m])) for m in case.info.get("alone", ())]


@pytest.mark.parametrize("name", [n for n in cases.names() if " models " not in n])
def test_case_is_the_checkers_bits(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", [n for n in cases.names() if " models " in n])
def test_many_models_in_one_launch(ctx, name):
    """Every model against the checker; the first, the middle and the last one also against themselves trained alone."""
    case = cases.get(name)
    side_by_side = run_case(ctx, name)
    order, alpha = case.runs[0]
    for m, got in zip(case.info["alone"], side_by_side):
        with trainer_for(ctx, [case.models[m]]) as one:
            one.run(case.frames, order[m], alpha[m])
            assert (autoencoder_bits(one.weights(0)).tobytes(), repr(one.totals()[0])) == got, "%s: model %d alone" % (name, m)


def test_a_case_run_twice_leaves_the_same_bytes(ctx):
    """Nothing in a launch depends on what ran before it: the non-finite sigmoid probes and the rates, twice each, on fresh trainers."""
    for name in ("sigmoid la non-finite", "rates"):
        case = cases.get(name)
        images = []
        for _ in range(2):
            with trainer_for(ctx, case.models) as t:
                t.run(case.frames, *case.runs[0])
                images.append([autoencoder_bits(t.weights(m)).tobytes() + repr(t.totals()[m]).encode() for m in range(len(case.models))])
        assert images[0] == images[1], name
