"""The case table of the trainer's edge tests ("Tests"): models, frames and runs at which train_kernel could
leave the checker's bits without tests/test_gpu_train.py noticing -- the defined sigmoid over the whole f32 range, arithmetic that
leaves the normal range, Mat::norm where it rescales, rates and starting weights that are not finite, run lengths around the
prefetch blocks of 8, and many models in one launch.  tests/test_train_cases.py shows on the checker alone that every case does
what its name says; tests/test_gpu_train_edges.py runs every case on the device.  Pure numpy over tests/_train_reference.py: the
library is not imported here, and a case is built (and its checker run) only when it is asked for."""
import numpy as np

import _train_reference as ref

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
FLT_MAX = np.finfo(F).max


class Case:
    """Models side by side, one frame array, and runs [(order, alpha)] that follow each other on one trainer.  order: [steps] shared
    by all models or [n_models][steps]; alpha: one value or one per model."""

    def __init__(self, models, frames, runs, labels=None, **info):
        self.models = list(models)
        self.frames = np.ascontiguousarray(frames, F)
        self.runs = [(np.ascontiguousarray(o, np.uint32), np.broadcast_to(np.asarray(a, F), (len(self.models),)).copy()) for o, a in runs]
        self.labels = labels or ["model %d" % m for m in range(len(self.models))]
        self.info = info
        self._trained = None

    def trained(self):
        """The checker's models after each run: [run][model].  Computed once."""
        if self._trained is None:
            now, out = [m.copy() for m in self.models], []
            for order, alpha in self.runs:
                for m, model in enumerate(now):
                    model.run(self.frames, order[m] if order.ndim == 2 else order, alpha[m])
                out.append([m.copy() for m in now])
            self._trained = out
        return self._trained


def ulps(x, n):
    """x and its n f32 neighbours on either side (finite ones)."""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(n):
        with np.errstate(over="ignore"):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        out += [lo, hi]
    return [v for v in out if np.isfinite(v)]


def ordinary(rng, n, d, sd=2.0):
    return (rng.standard_normal((n, d)) * sd).astype(F)


# ---- 1. the defined sigmoid, probed through one-step models at 64 -> 64 -------------------------------------------------------------
def first_where(pred, lo, hi):
    """The f32 closest to lo between lo and hi at which pred holds; pred is false at lo, true at hi and changes once."""
    lo, hi = F(lo), F(hi)
    while np.nextafter(lo, hi) != hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = np.nextafter(lo, hi)
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def sigmoid_edges():
    """Arguments at which train_exp / train_sigmoid change their behaviour, each with its neighbours to the last ulp."""
    sig = lambda v: ref.sigmoid_defined(np.array([v], F))[0]
    one = first_where(lambda v: sig(v) == F(1.0), 10.0, 20.0)                # ~ 16.64: exactly 1.0 from here on
    zero = first_where(lambda v: sig(v) == F(0.0), -80.0, -95.0)             # ~ -88.72: exactly +0.0 from here on
    sub = first_where(lambda v: sig(v) < np.finfo(F).tiny, -80.0, -95.0)     # ~ -87.34: the quotient 1 / (1 + e) turns subnormal
    esub = first_where(lambda v: ref.exp_defined(np.array([-v], F))[0] < np.finfo(F).tiny, 80.0, 95.0)   # e = exp(-v) turns subnormal
    out = []
    tiny, denorm_max = np.finfo(F).tiny, np.array([0x007FFFFF], np.uint32).view(F)[0]
    for p in (F(0.0), F(1e-45), denorm_max, tiny):
        for s in (F(1.0), F(-1.0)):
            out += ulps(s * p, 3)
    out += [F(-0.0)]
    for p in (one, zero, sub, esub, -esub, -one):
        out += ulps(p, 8)
    for p in (100.0, 104.0, -100.0, -104.0, 88.0, -88.0, 16.0, -16.0, 1.0, -1.0):
        out += ulps(p, 3)
    out += [FLT_MAX, -FLT_MAX, np.nextafter(FLT_MAX, F(0)), np.nextafter(-FLT_MAX, F(0)), F(1e30), F(-1e30), F(105.0), F(-105.0), F(1000.0), F(-1000.0)]
    out += list(np.linspace(-88.8, -87.3, 200).astype(F)) + list(np.linspace(87.3, 88.8, 200).astype(F))
    # t = -v with t * 1.44269504 within an ulp of k + 1/2: the round-to-nearest-even of kf, for every k the clamp allows
    for k in range(-150, 145):
        t = F((k + 0.5) / np.float64(F(1.44269504)))
        out += [-u for u in ulps(t, 2)]
    return np.array(out, F)


def sigmoid_sweep(rng):
    """Every binary exponent up to 2^7 with random mantissas and both signs, uniform draws in [-105, -86] and [-30, 30]."""
    exps = np.repeat(np.arange(0, 135, dtype=np.uint32), 2)                   # exponent fields 0 (subnormal) .. 134 (2^7)
    mant = rng.integers(0, 1 << 23, exps.size, dtype=np.uint32)
    sign = (np.arange(exps.size, dtype=np.uint32) & np.uint32(1)) << np.uint32(31)
    by_exponent = (sign | (exps << np.uint32(23)) | mant).view(F)
    return np.concatenate([by_exponent, rng.uniform(-105.0, -86.0, 1465).astype(F), rng.uniform(-30.0, 30.0, 1465).astype(F)])


# frame values a lane may carry when the edge list is probed: an argument that is not observed at one of them is given another
ACT_FRAME_VALUES = np.array([1.0, 2.0, 0.75, 0.25, 1.5, 0.625, 3.0, 0.375, 0.0, -1.0, 0.5, 5.0, 0.1, 1.25, 7.0, -0.3], F)
LA_SCALE = F(2.0 ** -7)              # W_dec = LA_SCALE * I at the `la` site: act = sigmoid(v / 128) stays away from 0 and 1
LA_FRAME_SCALE = F(2.0 ** 20)        # and frames of this size make delta_out . W_dec^T larger than 1: subnormal la values keep their bits


def probe_models(site, args):
    """One 64 -> 64 model per 64 arguments.  `act`: W_enc = 0, b_enc = 1 (latent = 1), W_dec = 0, b_dec = u: act = sigmoid(u) and the
    updated W_dec column is -delta_out.  `la`: W_enc = 0, b_enc = v (latent = v), W_dec = LA_SCALE * I, b_dec = 0: the updated W_enc
    column is -x * delta_dec."""
    args = np.asarray(args, F).reshape(-1, 64)
    zero = np.zeros((64, 64), F)
    if site == "act":
        return [ref.Model(zero, zero, np.ones(64, F), u) for u in args]
    return [ref.Model(zero, np.eye(64, dtype=F) * LA_SCALE, v, np.zeros(64, F)) for v in args]


def probe_frame(site, part):
    """63 ones and a 2 for the sweeps; for the edge list every value of ACT_FRAME_VALUES in four lanes."""
    x = np.tile(ACT_FRAME_VALUES, 64 // len(ACT_FRAME_VALUES)) if part == "edges" else np.array([1.0] * 63 + [2.0], F)
    return (x if site == "act" else x * LA_FRAME_SCALE).reshape(1, 64)


def observed(site, models, frame):
    """[model][lane]: replacing the checker's sigmoid value at the lane's argument by its upper f32 neighbour, and by its lower one,
    each changes a bit of the lane's column of the updated weights (W_dec, b_dec for `act`; W_enc, b_enc for `la`)."""
    call = {"la": 0, "act": 1}[site]
    out = np.empty((len(models), 64), bool)

    def column(model):
        w, b = (model.wd, model.bd) if site == "act" else (model.we, model.be)
        return ref.canonical_bits(np.concatenate([w, b[None, :]]).T).reshape(64, -1)

    for n, model in enumerate(models):
        columns = []
        for towards in (None, INF, -INF):
            calls = []

            def sigmoid(v, towards=towards, calls=calls):
                calls.append(0)
                s = ref.sigmoid_defined(v)
                return s if towards is None or len(calls) - 1 != call else np.nextafter(s, towards)

            m = ref.Model(model.we, model.wd, model.be, model.bd, F, sigmoid)
            m.step(frame, 1.0)
            columns.append(column(m))
        out[n] = (columns[0] != columns[1]).any(1) & (columns[0] != columns[2]).any(1)
    return out


def sigmoid_case(site, part):
    """part `edges`: the edge list; `sweep`: the seeded sweep.  info: args [model][64] and used [model][64] (False: a filler lane)."""
    frame = probe_frame(site, part)
    if part == "sweep" or site == "la":
        values = sigmoid_sweep(np.random.default_rng(181)) if part == "sweep" else sigmoid_edges()
        args = np.concatenate([values, np.zeros(-values.size % 64, F)]).reshape(-1, 64)
        used = (np.arange(args.size) < values.size).reshape(-1, 64)
    else:
        # Whether an argument is observed depends on the frame value of its lane alone (the probe's weights are zero).  Try every edge
        # argument under each of the frame's values (the frame rolled by c lanes), then give it a lane of the first value, counted from
        # the one its position would have had, at which it is observed.
        edges, n_values = sigmoid_edges(), len(ACT_FRAME_VALUES)
        flat = np.concatenate([edges, np.zeros(-edges.size % 64, F)])
        seen = np.stack([observed(site, probe_models(site, flat), np.roll(frame[0], c)).ravel() for c in range(n_values)])
        queues = [[] for _ in range(n_values)]
        for q, u in enumerate(edges):
            values = [(q + c) % n_values for c in range(n_values) if seen[(-c) % n_values, q]]   # rolled by r, lane q carries value q - r
            if not values:
                raise AssertionError("%r is not observed at any frame value" % u)
            queues[values[0]].append(u)
        per_model = 64 // n_values
        n_models = max(-(-len(queue) // per_model) for queue in queues)
        args, used = np.zeros((n_models * per_model, n_values), F), np.zeros((n_models * per_model, n_values), bool)
        for value, queue in enumerate(queues):
            args[:len(queue), value] = queue
            used[:len(queue), value] = True
        args, used = args.reshape(-1, 64), used.reshape(-1, 64)
    return Case(probe_models(site, args), frame, [([0], 1.0)], site=site, args=args, used=used)


def sigmoid_nonfinite_case(site):
    """+inf, -inf and NaN arguments, one model each, in lane 0, lane 63 and lane 31."""
    args = np.zeros((3, 64), F)
    for m, (v, lane) in enumerate(((INF, 0), (-INF, 63), (NAN, 31))):
        args[m, lane] = v
    return Case(probe_models(site, args), probe_frame(site, "edges"), [([0], 1.0)], labels=["+inf", "-inf", "nan"], site=site)


# ---- 2. arithmetic that leaves the normal range -----------------------------------------------------------------------------------
def subnormal_products_case(d, l, steps):
    """Frames ~ 1e-28 with one component 1 (no rescale) against W_enc ~ 1e-12: products ~ 1e-40.  The W_enc row under the 1 and b_enc
    start as zero and W_dec is ~ 1e-38, so they grow by ~ 1e-39 per step: the latent stays a sum of subnormals for the whole run, and
    what it adds to W_dec stays in the compared bits.  A third of every array is zero."""
    rng = np.random.default_rng(2000 + d)
    def weights(scale, *shape):
        w = (rng.standard_normal(shape) * scale).astype(F)
        w[rng.random(shape) < 1 / 3] = 0.0
        return w
    one = d // 2
    we, wd = weights(1e-12, d, l), weights(1e-38, l, d)
    we[one] = 0.0
    frames = (rng.standard_normal((steps, d)) * 1e-28).astype(F)
    frames[:, one] = 1.0
    return Case([ref.Model(we, wd, np.zeros(l, F), weights(1e-12, d))], frames, [(np.arange(steps), 0.5)])


def dot_overflow_case():
    """5 -> 3.  Step 4 meets a frame whose products with column 0 of W_enc are 2e38, 2e38 (their sum is +inf), then -inf: NaN, because
    k ascends -- from the last term down the sum would be -inf.  info: frame, column."""
    rng = np.random.default_rng(2100)
    model = ref.seeded(rng, 5, 3)
    model.we[:, 0] = [2e19, 2e19, 1e20, 0.25, -0.5]
    frames = ordinary(rng, 10, 5)
    frames[9] = [1e19, 1e19, -1e20, 1.0, 0.5]
    order = np.array([0, 1, 2, 3, 9, 4, 5, 6, 7, 8, 0], np.uint32)
    # the steps before must leave the column large: a rate of zero keeps it (and every other weight) as it is
    return Case([model], frames, [(order, 0.0)], frame=frames[9].copy(), column=model.we[:, 0].copy(), step=4)


def huge_frames_case(d, l, steps):
    rng = np.random.default_rng(2200 + d)
    model = ref.seeded(rng, d, l)
    model.we *= F(1e-30)
    model.wd *= F(1e-30)
    frames = ordinary(rng, steps, d) * F(1e30)
    return Case([model, model.copy()], frames, [(np.arange(steps), [1e-35, 1e-3])], labels=["rate 1e-35", "rate 1e-3"])


def tiny_weights_case(d, l, steps):
    """Weights and biases that start as +0, -0 and subnormals of either sign; ordinary frames."""
    rng = np.random.default_rng(2300 + d)
    def weights(*shape):
        sub = rng.integers(1, 1 << 23, shape, dtype=np.uint32) | (rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31))
        pick = rng.integers(0, 3, shape)
        return np.where(pick == 0, F(0.0), np.where(pick == 1, F(-0.0), sub.view(F))).astype(F)
    return Case([ref.Model(weights(d, l), weights(l, d), weights(l), weights(d))], ordinary(rng, steps, d), [(np.arange(steps), 0.1)])


def signed_zero_case(d, l, steps):
    """Rate 0 with -0 in frames and weights.  Model 0: seeded weights with a third set to -0; model 1: every weight and bias -0."""
    rng = np.random.default_rng(2400 + d)
    a = ref.seeded(rng, d, l)
    for w in (a.we, a.wd, a.be, a.bd):
        w[rng.random(w.shape) < 1 / 3] = -0.0
    z = lambda *shape: np.full(shape, -0.0, F)
    frames = ordinary(rng, steps, d)
    frames[rng.random(frames.shape) < 0.25] = -0.0
    frames[rng.random(frames.shape) < 0.1] = 0.0
    return Case([a, ref.Model(z(d, l), z(l, d), z(l), z(d))], frames, [(np.arange(steps), 0.0)], labels=["a third -0", "all -0"])


# ---- 3. Mat::norm where it normalises ---------------------------------------------------------------------------------------------
def tile(values, d):
    return np.resize(np.asarray(values, F), d)


def norm_frames(d):
    """name -> (frame, rescales, model stays finite); None where the outcome is not the point of the frame."""
    rng = np.random.default_rng(3000 + d)
    near = np.nextafter(F(0.05), INF)
    s = np.nextafter(F(1e-8), F(0))
    shuffled = lambda v: rng.permutation(tile(v, d)).astype(F)
    out = {
        "spread below 1e-8": (tile([0, 3e-9, 7e-9, 9e-9, 1e-9], d), True, True),
        "one ulp apart at 0.05": (tile([0.05, near, near, 0.05, near], d), True, True),
        "spread just under 1e-8": (tile([0, s, s / F(2), s / F(4), s], d), True, True),
        "spread exactly 1e-8": (tile([0, F(1e-8), F(5e-9), F(2.5e-9), F(1e-8)], d), False, True),
        "subnormal spread": (tile([0, 1e-45, 3e-45, 0, 2e-45], d), True, True),
        "inf and a spread below 1e-8": (np.concatenate([[INF], tile([1e-9, 2e-9, 3e-9, 4e-9], d - 1)]).astype(F), True, False),
        "all non-finite": (tile([INF, -INF, NAN, INF, NAN], d), False, False),
        # minimum and maximum both repeated, in the first and the last component (the 64th at D = 64); a -0 after the +0 that is kept
        "repeated ends, min first": (np.concatenate([[0.0, 4e-9], shuffled([2e-9, -0.0, 4e-9, 1e-9])[:d - 4], [4e-9, -0.0]]).astype(F), True, None),
        "repeated ends, max first": (np.concatenate([[4e-9, -0.0], shuffled([2e-9, 0.0, 4e-9, 3e-9])[:d - 4], [0.0, 4e-9]]).astype(F), True, None),
        "repeated ends, wide": (np.concatenate([[-1.5, 2.5], shuffled([2.5, -1.5, 0.5, 1.0])[:d - 4], [2.5, -1.5]]).astype(F), False, True),
    }
    assert all(v[0].shape == (d,) and v[0].dtype == F for v in out.values())
    return out


NORM_ORDER_STEPS = 20
NORM_PLACES = (0, 7, 11)             # step 0, the last step of a block of 8, a step inside


def norm_case(d, l):
    """Per frame of norm_frames(d) three models, which meet it at step 0, 7 or 11 of 20; the first and the last model stay on ordinary
    frames.  info: at [model] = (name, step) or None."""
    rng = np.random.default_rng(3100 + d)
    special = norm_frames(d)
    n_plain = 30
    frames = np.concatenate([ordinary(rng, n_plain, d), np.stack([v[0] for v in special.values()])])
    at = [None] + [(name, p) for name in special for p in NORM_PLACES] + [None]
    models = [ref.seeded(rng, d, l) for _ in at]
    orders = rng.integers(0, n_plain, (len(at), NORM_ORDER_STEPS)).astype(np.uint32)
    for m, a in enumerate(at):
        if a is not None:
            orders[m, a[1]] = n_plain + list(special).index(a[0])
    labels = ["neighbour" if a is None else "%s at step %d" % a for a in at]
    return Case(models, frames, [(orders, 0.1)], labels=labels, at=at)


# ---- 4. rates, starting weights, the first non-finite step ------------------------------------------------------------------------
RATES = [0.0, -0.1, 1e-42, 1e30, np.inf, np.nan]
RATES_FIRST_NONFINITE = [None, None, None, 1, 0, 0]


def rates_case():
    rng = np.random.default_rng(4001)
    model = ref.seeded(rng, 5, 3)
    frames = ordinary(rng, 12, 5)
    return Case([model.copy() for _ in RATES], frames, [(rng.integers(0, 12, 17), RATES)], labels=["rate %r" % r for r in RATES])


def nonfinite_start_case(d, l, steps):
    """One model per place of a single non-finite starting value: +-inf in the first and the last entry of each array, a NaN inside
    each array.  One fresh run of `steps`."""
    rng = np.random.default_rng(4100 + 100 * d + l)
    base = ref.seeded(rng, d, l)
    places = [("we", (0, 0), INF), ("we", (d - 1, l - 1), -INF), ("wd", (0, 0), INF), ("wd", (l - 1, d - 1), -INF),
              ("be", (0,), INF), ("be", (l - 1,), -INF), ("bd", (0,), INF), ("bd", (d - 1,), -INF),
              ("we", (d // 2, l // 2), NAN), ("wd", (l // 2, d // 2), NAN), ("be", (l // 2,), NAN), ("bd", (d // 2,), NAN)]
    models = []
    for name, index, value in places:
        m = base.copy()
        getattr(m, name)[index] = value
        models.append(m)
    frames = ordinary(rng, 10, d)
    order = rng.integers(0, 10, 9)[:steps]
    return Case(models, frames, [(order, 0.1)], labels=["%s in %s%r" % (v, n, list(i)) for n, i, v in places])


DIVERGE_RATE = 1e38


def diverge_parts():
    """5 -> 3 at a rate of 1e38.  The first three frames are so large (~ 1e6) that every output saturates at exactly 0 or 1: delta_out
    is zero and the model stays as it is.  The fourth (~ 30) does not saturate, and its update overflows."""
    rng = np.random.default_rng(4200)
    model = ref.seeded(rng, 5, 3)
    frames = ordinary(rng, 12, 5, 30.0)
    frames[:3] *= F(1e6 / 30.0)
    return model, frames, np.arange(12, dtype=np.uint32)


def diverge_history():
    """Per step of the whole run: (some weight is inf, some weight is NaN)."""
    model, frames, order = diverge_parts()
    model, out = model.copy(), []
    for i in order:
        model.step(frames[i], DIVERGE_RATE)
        w = np.concatenate([a.ravel() for a in (model.we, model.wd, model.be, model.bd)])
        out.append((bool(np.isinf(w).any()), bool(np.isnan(w).any())))
    return out


def diverge_inf_step():
    """s: the first step after which a weight is inf and none is NaN."""
    return [i for i, (inf, nan) in enumerate(diverge_history()) if inf and not nan][0]


def diverge_case(split):
    """`whole`; `last`: s is the last step of the first run; `first`: s is the first step of the second run."""
    model, frames, order = diverge_parts()
    s = diverge_inf_step()
    cut = {"whole": None, "last": s + 1, "first": s}[split]
    runs = [(order, DIVERGE_RATE)] if cut is None else [(order[:cut], DIVERGE_RATE), (order[cut:], DIVERGE_RATE)]
    return Case([model], frames, runs)


# ---- 5. step counts around the prefetch blocks of 8 -------------------------------------------------------------------------------
RUN_LENGTHS = (7, 8, 9, 15, 16, 17, 24, 25, 64)
CONTINUATIONS = ((8, 8), (8, 1), (7, 9), (16, 0, 8))


def block_order(rng, n_frames, rows, steps):
    """Indices that include 0 and n_frames - 1; the last step of every row uses the last frame of the array."""
    order = rng.integers(0, n_frames, (rows, steps)).astype(np.uint32)
    order[:, 0] = 0
    order[:, steps // 2] = n_frames - 1
    order[:, -1] = n_frames - 1
    return order


def block_case(d, l, lengths, per_model):
    rng = np.random.default_rng(5000 + 100 * d + sum(lengths) * 7 + len(lengths) + per_model)
    n_models, n_frames = (3, 11) if per_model else (2, 11)
    models = [ref.seeded(rng, d, l) for _ in range(n_models)]
    frames = ordinary(rng, n_frames, d)
    runs = []
    for n in lengths:
        order = block_order(rng, n_frames, n_models if per_model else 1, n) if n else np.zeros((n_models if per_model else 1, 0), np.uint32)
        runs.append((order if per_model else order[0], np.linspace(0.05, 0.2, n_models)))
    return Case(models, frames, runs)


# ---- 6. many models in one launch -------------------------------------------------------------------------------------------------
def many_case(d, l, n_models):
    rng = np.random.default_rng(6000 + d)
    models = [ref.seeded(np.random.default_rng(6100 + 7 * m + d), d, l) for m in range(n_models)]
    frames = ordinary(rng, 40, d)
    orders = rng.integers(0, 40, (n_models, 9)).astype(np.uint32)
    alphas = rng.uniform(0.01, 0.3, n_models).astype(F)
    return Case(models, frames, [(orders, alphas)], alone=(0, n_models // 2, n_models - 1))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
BUILDERS = {}


def _add(name, builder, *args):
    BUILDERS[name] = (builder, args)


for _site in ("act", "la"):
    _add("sigmoid %s edges" % _site, sigmoid_case, _site, "edges")
    _add("sigmoid %s sweep" % _site, sigmoid_case, _site, "sweep")
    _add("sigmoid %s non-finite" % _site, sigmoid_nonfinite_case, _site)
for _d, _l, _n in ((5, 3, 9), (13, 8, 17)):
    _add("subnormal products %d->%d" % (_d, _l), subnormal_products_case, _d, _l, _n)
    _add("huge frames %d->%d" % (_d, _l), huge_frames_case, _d, _l, _n)
    _add("tiny weights %d->%d" % (_d, _l), tiny_weights_case, _d, _l, _n)
    _add("signed zeros %d->%d" % (_d, _l), signed_zero_case, _d, _l, _n)
_add("dot overflow", dot_overflow_case)
_add("norm 5->3", norm_case, 5, 3)
_add("norm 64->7", norm_case, 64, 7)
_add("rates", rates_case)
for _d, _l in ((64, 64), (33, 5), (5, 33)):
    for _n in (1, 8, 9):
        _add("non-finite start %d->%d, %d steps" % (_d, _l, _n), nonfinite_start_case, _d, _l, _n)
for _split in ("whole", "last", "first"):
    _add("diverge %s" % _split, diverge_case, _split)
for _d, _l in ((3, 2), (13, 8)):
    for _n in RUN_LENGTHS:
        _add("%d steps %d->%d shared" % (_n, _d, _l), block_case, _d, _l, (_n,), False)
        _add("%d steps %d->%d per model" % (_n, _d, _l), block_case, _d, _l, (_n,), True)
    for _parts in CONTINUATIONS:
        _add("%s steps %d->%d shared" % (" + ".join(map(str, _parts)), _d, _l), block_case, _d, _l, _parts, False)
        _add("%s steps %d->%d per model" % (" + ".join(map(str, _parts)), _d, _l), block_case, _d, _l, _parts, True)
_add("512 models 64->64", many_case, 64, 64, 512)
_add("1500 models 3->2", many_case, 3, 2, 1500)

_BUILT = {}


def names():
    return list(BUILDERS)


def get(name):
    if name not in _BUILT:
        builder, args = BUILDERS[name]
        _BUILT[name] = builder(*args)
    return _BUILT[name]
