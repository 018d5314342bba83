"""The checker of the autoencoder trainer: a literal numpy restatement of AutoEncoder::take_step
(neural.rs:74-94) with every intermediate rounded to f32 and the project's DEFINED sigmoid (csrc/train_math.h), which the device
must equal bit for bit; its float64 twin with the true exp, against which the f32 form means something on short horizons only; and
apd_train_order's counter-based generator.  Nothing here is fast, and nothing here imports the library."""
import numpy as np

F = np.float32
NONE = None


def canonical_bits(a):
    """The bit patterns of f32 values with every NaN as 0x7FC00000.  "Bit for bit" means this everywhere in the trainer's tests: which
    NaN an operation returns (sign, payload) is left to the implementation by IEEE 754 -- x86 divides 0 / 0 into 0xFFC00000, and a
    compiler may turn the reference's `* -1.0` into a sign flip -- and no later result depends on it."""
    bits = np.ascontiguousarray(a, F).ravel().view(np.uint32).copy()
    bits[np.isnan(np.ascontiguousarray(a, F).ravel())] = 0x7FC00000
    return bits


# ---- the defined exponential and sigmoid (train_math.h, operation for operation)
def exp_defined(t):
    """e ~ exp(t) for an f32 array t: clamp to [-104, 100], k = rne(t log2 e) by the 1.5 * 2^23 trick, two-part reduction,
    Cephes' degree-5 polynomial by Horner, two exact power-of-two scalings."""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        tc = np.where(t > F(100.0), F(100.0), t)
        tc = np.where(tc < F(-104.0), F(-104.0), tc)
        z = tc * F(1.44269504)
        kf = (z + F(12582912.0)) - F(12582912.0)
        r = (tc - kf * F(0.693359375)) - kf * F(-2.12194440e-4)
        p = F(1.9875691500e-4)
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = p * r + F(c)
        rr = r * r
        p = p * rr
        p = p + r
        p = p + F(1.0)
        k = np.where(tc == tc, kf, F(0.0)).astype(np.int32)
        k1 = k >> 1
        k2 = k - k1
        p = (p * np.ldexp(F(1.0), k1).astype(F)) * np.ldexp(F(1.0), k2).astype(F)
        return np.where(tc == tc, p, t).astype(F)


def sigmoid_defined(v):
    with np.errstate(all="ignore"):
        return (F(1.0) / (F(1.0) + exp_defined(-np.asarray(v, F)))).astype(F)


def sigmoid_libm(v):
    """numerics.rs:233 with numpy's f32 exp: what a platform libm would give."""
    with np.errstate(all="ignore"):
        return (F(1.0) / (F(1.0) + np.exp(-np.asarray(v, F)))).astype(F)


# ---- Mat::norm (numerics.rs:192-208), in any float type
def norm(x):
    ft = x.dtype.type
    mn, mx = ft(np.inf), ft(-np.inf)
    for v in x:
        if v < mn and np.isfinite(v):
            mn = v
        if v > mx and np.isfinite(v):
            mx = v
    with np.errstate(all="ignore"):
        scaler = mx - mn
        if abs(mn - mx) < ft(F(1e-8)):
            return ((x - mn) / scaler).astype(x.dtype)
    return x.copy()


def mul_row(x, w):
    """Mat::mul of a 1 x K row by a K x N matrix (numerics.rs:305-319): from 0.0, k ascending, a multiply then an add."""
    acc = np.zeros(w.shape[1], w.dtype)
    for k in range(w.shape[0]):
        acc = acc + x[k] * w[k]
    return acc


class Model:
    """One autoencoder and the trainer's counters.  dtype float32 (the checker) or float64 (the twin)."""

    def __init__(self, w_encode, w_decode, b_encode, b_decode, dtype=F, sigmoid=None):
        self.dt = np.dtype(dtype).type
        self.we = np.array(w_encode, dtype).copy()            # [D][L]
        self.wd = np.array(w_decode, dtype).copy()            # [L][D]
        self.be = np.array(b_encode, dtype).ravel().copy()
        self.bd = np.array(b_decode, dtype).ravel().copy()
        d, l = self.bd.size, self.be.size
        self.we, self.wd = self.we.reshape(d, l), self.wd.reshape(l, d)
        if sigmoid is None:
            sigmoid = sigmoid_defined if self.dt is F else (lambda v: 1.0 / (1.0 + np.exp(-v)))
        self.sigmoid = sigmoid
        self.total_err, self.steps, self.lifetime, self.first_nonfinite = self.dt(0.0), 0, 0, NONE

    def copy(self):
        m = Model(self.we, self.wd, self.be, self.bd, self.dt, self.sigmoid)
        m.total_err, m.steps, m.lifetime, m.first_nonfinite = self.total_err, self.steps, self.lifetime, self.first_nonfinite
        return m

    def finite(self):
        return all(np.isfinite(a).all() for a in (self.we, self.wd, self.be, self.bd))

    def step(self, x, alpha):
        dt = self.dt
        x, alpha = np.asarray(x, dt), dt(alpha)
        with np.errstate(all="ignore"):
            y = norm(x)
            latent = mul_row(x, self.we) + self.be
            la = self.sigmoid(latent)
            output = mul_row(latent, self.wd) + self.bd        # the pre-activation latent (neural.rs:78)
            act = self.sigmoid(output)
            delta_out = ((y - act) * dt(-1.0)) * (act * (dt(1.0) - act))
            delta_dec = mul_row(delta_out, self.wd.T) * (la * (dt(1.0) - la))
            grad_dec = (dt(0.0) + latent[:, None] * delta_out[None, :]) * alpha
            grad_enc = (dt(0.0) + x[:, None] * delta_dec[None, :]) * alpha
            self.we = self.we - grad_enc
            self.wd = self.wd - grad_dec
            self.be = self.be - delta_dec * alpha
            self.bd = self.bd - delta_out * alpha
            diff = act - y
            sq = diff * diff
            dist = dt(0.0)
            for v in sq:
                dist = dist + v
            err = dt(0.5) * np.sqrt(dist)
            self.total_err = self.total_err + err
        if self.first_nonfinite is NONE and not self.finite():
            self.first_nonfinite = self.lifetime
        self.steps += 1
        self.lifetime += 1
        return err

    def run(self, frames, order, alpha):
        for i in order:
            self.step(frames[int(i)], alpha)
        return self

    def reset_totals(self):
        self.total_err, self.steps = self.dt(0.0), 0

    def bits(self):
        """The four matrices as one array of canonical bit patterns (f32 models only)."""
        return canonical_bits(np.concatenate([a.astype(F).ravel() for a in (self.we, self.wd, self.be, self.bd)]))


def seeded(rng, d, l, dtype=F):
    """AutoEncoder::new (neural.rs:46-53): Mat::seeded for w_encode, w_decode, b_encode, b_decode, in that order."""
    def mat(rows, cols):
        return ((rng.random(rows * cols, dtype=F) - F(0.5)) / F(cols)).reshape(rows, cols)
    we, wd, be, bd = mat(d, l), mat(l, d), mat(1, l), mat(1, d)
    return Model(we, wd, be, bd, dtype)


def max_weight_difference(a, b):
    return max(float(np.max(np.abs(p.astype(np.float64) - q.astype(np.float64))))
               for p, q in ((a.we, b.we), (a.wd, b.wd), (a.be, b.be), (a.bd, b.bd)))


# ---- apd_train_order's generator (train_math.h)
M64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def order_key(seed, epoch, signal):
    key = mix64((seed + 0x9E3779B97F4A7C15) & M64)
    key = mix64(key ^ (((epoch + 1) * 0xD1B54A32D192ED03) & M64))
    return mix64(key ^ (((signal + 1) * 0x8CB92BA72F3D8DD7) & M64))


def train_order(seed, epoch, offsets):
    out = []
    for s in range(len(offsets) - 1):
        first, n = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        block = list(range(first, first + n))
        key = order_key(seed, epoch, s)
        for i in range(n - 1, 0, -1):
            u = mix64((key + i * 0x9E3779B97F4A7C15) & M64)
            j = ((u >> 32) * (i + 1)) >> 32
            block[i], block[j] = block[j], block[i]
        out += block
    return np.array(out, np.uint32)


def step_decay(learning_rate, drop, epoch_drop, epoch):
    """neural.rs:26-28 in f32.  The power is exact when drop is a power of two (the shipped 0.5); otherwise numpy's powf stands in."""
    with np.errstate(all="ignore"):
        return F(learning_rate) * np.power(F(drop), np.floor((F(1.0) + F(epoch)) / F(epoch_drop)), dtype=F)


def f32_count(n):
    """main.rs:117,131 literally: total = 0.0; total += 1.0 per step.  Only for small n; the closed form is neural.epoch_count."""
    total = F(0.0)
    for _ in range(n):
        total = total + F(1.0)
    return total


def train_loop(frames, offsets, discovery, models, seed):
    """main.rs:115-135 on checker models (changed in place): per epoch the decayed rate, the epoch's order, a step per frame and the
    mean total_err / total.  Returns the means [epochs][models]."""
    means = np.empty((discovery.epochs, len(models)), F)
    for epoch in range(discovery.epochs):
        lr = step_decay(discovery.learning_rate, discovery.drop, discovery.epoch_drop, epoch)
        order = train_order(seed, epoch, offsets)
        total = F(min(len(order), 1 << 24))
        for m, model in enumerate(models):
            model.reset_totals()
            model.run(frames, order, lr)
            with np.errstate(all="ignore"):
                means[epoch, m] = model.total_err / total
    return means
