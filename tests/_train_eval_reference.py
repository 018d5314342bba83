"""The checker of apd_trainer_evaluate: the forward half of Model.step (tests/_train_reference.py) restated
literally in f32 scalars and rows -- x.norm(), the two Mat::mul rows, the defined sigmoid, 0.5 * euclidean -- with nothing of the
update in it, and main.rs:130's running total under frozen weights.  The device must equal it bit for bit (canonical_bits).  The
sigmoid probe the GPU test uses and the lemma it rests on live here too, so that the CPU and the GPU test build the same models.
Nothing here imports the library."""
import numpy as np

import _train_reference as ref
from _train_reference import canonical_bits, mul_row, norm, sigmoid_defined

F = np.float32
NONE = None


def error_of(model, x):
    """What AutoEncoder::take_step (neural.rs:74-94) returns for the frame x under the model's weights, which are only read."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        y = norm(x)
        latent = mul_row(x, model.we) + model.be
        output = mul_row(latent, model.wd) + model.bd          # the pre-activation latent (neural.rs:78)
        act = sigmoid_defined(output)
        dist = F(0.0)
        for i in range(x.size):
            diff = F(act[i] - y[i])
            sq = F(diff * diff)
            dist = F(dist + sq)
        return F(F(0.5) * np.sqrt(dist))


def evaluate(model, frames, order=None):
    """(errors [n_eval] f32, total f32, first non-finite position or None): order None is every frame in order.  The total starts
    from +0.0 and takes one f32 add per position, in position order."""
    frames = np.asarray(frames, F)
    order = range(len(frames)) if order is None else order
    errors, total, first = [], F(0.0), NONE
    for e, i in enumerate(order):
        err = error_of(model, frames[int(i)])
        errors.append(err)
        with np.errstate(all="ignore"):
            total = F(total + err)
        if first is NONE and not np.isfinite(err):
            first = e
    return np.array(errors, F), total, first


def errors_batch(model, x):
    """error_of for every row of x at once: the same f32 operations in the same order, carried out on columns of positions instead of
    scalars (an elementwise numpy operation rounds each element as the scalar one does).  Rows that Mat::norm rescales go through
    the literal norm().  tests/test_train_eval_reference.py holds it to error_of's bits; the GPU tests use it where they evaluate
    tens of thousands of positions."""
    x = np.asarray(x, F).reshape(-1, model.bd.size)
    with np.errstate(all="ignore"):
        finite = np.isfinite(x)
        mn, mx = np.where(finite, x, F(np.inf)).min(axis=1), np.where(finite, x, F(-np.inf)).max(axis=1)
        y = x.copy()
        for r in np.nonzero(np.abs(mn - mx) < F(1e-8))[0]:
            y[r] = norm(x[r])
        latent = np.zeros((x.shape[0], model.be.size), F)
        for k in range(model.we.shape[0]):
            latent = latent + x[:, k:k + 1] * model.we[k][None, :]
        latent = latent + model.be[None, :]
        output = np.zeros_like(x)
        for j in range(model.wd.shape[0]):
            output = output + latent[:, j:j + 1] * model.wd[j][None, :]
        act = sigmoid_defined(output + model.bd[None, :]).reshape(x.shape)
        dist = np.zeros(x.shape[0], F)
        for i in range(x.shape[1]):
            diff = act[:, i] - y[:, i]
            dist = dist + diff * diff
        return (F(0.5) * np.sqrt(dist)).astype(F)


def totals_of(errors):
    """(total, first non-finite position or None) of one model's errors: from +0.0, one f32 add per position in position order."""
    total = F(0.0)
    with np.errstate(all="ignore"):
        for err in errors:
            total = F(total + err)
    bad = np.nonzero(~np.isfinite(errors))[0]
    return total, (int(bad[0]) if bad.size else NONE)


def evaluate_many(models, frames, order=None):
    """evaluate per model through errors_batch; order None, [n_eval] or [n_models][n_eval].  Returns (errors [n_models][n_eval],
    totals [n_models], firsts).  The errors of each frame are computed once per model and gathered through the order."""
    frames = np.asarray(frames, F)
    order = None if order is None else np.asarray(order, np.int64)
    errors, totals, firsts = [], [], []
    for k, m in enumerate(models):
        per_frame = errors_batch(m, frames) if len(frames) else np.zeros(0, F)
        e = per_frame if order is None else per_frame[order[k] if order.ndim == 2 else order]
        total, first = totals_of(e)
        errors.append(e)
        totals.append(total)
        firsts.append(first)
    return np.stack(errors), np.array(totals, F), firsts


# ---- the sigmoid probe.  D = 2, L = 1, W_enc = 0, W_dec = 0, b_dec = [u, 40], frame [0, 1]: output = [u, 40] whatever the latent is,
# act_1 = sigmoid(40) = 1 exactly and y = x (|0 - 1| is not below 1e-8), so diff = [sigmoid(u) - 0, 1 - 1] and
#   error = 0.5 * sqrt(s * s + 0) = 0.5 * s        with s = sigmoid_defined(u)
# EXACTLY wherever s * s is a normal f32: the square is then one rounding of s^2, its correctly rounded root is s again (the root of
# fl(s^2) lies within a quarter ulp of s), and the halving is exact.  The error then shows every bit of s.  Where s * s is subnormal
# or zero (s below ~1.1e-19) bits of s are lost; those arguments are compared all the same, and counted.
PROBE_FRAME = np.array([[0.0, 1.0]], F)


def probe_model(u):
    return ref.Model(np.zeros((2, 1), F), np.zeros((1, 2), F), np.zeros(1, F), np.array([u, 40.0], F))


def probe_arguments():
    """The edge list and the seeded sweep of tests/_train_cases.py's `act` site, +-inf and NaN; padded with zeros to whole launches
    of 64 models (b_dec belongs to the model: an argument is a model).  Those lists dwell where the sigmoid underflows (753 of
    their 5314 finite arguments lie below about -43.7, where sigmoid^2 is subnormal and the lemma is silent): on their own the lemma
    covers 85.8 % of them.  So 3000 seeded draws from the normal range [-40, 20] are appended, which brings the share to 90.9 %.
    Returns (args [launch][64], count of real arguments)."""
    import _train_cases as cases
    extra = np.random.default_rng(182).uniform(-40.0, 20.0, 3000).astype(F)
    values = np.concatenate([cases.sigmoid_edges(), cases.sigmoid_sweep(np.random.default_rng(181)), np.array([np.inf, -np.inf, np.nan], F), extra]).astype(F)
    padded = np.concatenate([values, np.zeros(-values.size % 64, F)])
    return padded.reshape(-1, 64), values.size


def probe_lemma_holds(u):
    """[...] bool: the checker's error at argument u is exactly 0.5 * sigmoid_defined(u) (NaN counts as equal to NaN)."""
    u = np.asarray(u, F)
    with np.errstate(all="ignore"):
        want = (F(0.5) * sigmoid_defined(u.ravel())).astype(F)
    got = np.array([error_of(probe_model(v), PROBE_FRAME[0]) for v in u.ravel()], F)
    return (canonical_bits(got) == canonical_bits(want)).reshape(u.shape)
