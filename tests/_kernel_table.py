"""The DTW kernel table as the tests see it: parsed from the text of csrc/apd_internal.h, the single source of what is instantiated.

The five APD_*_GEOMS(X) lists and kKernelDims are read from the header (continuation lines joined first); the two per-dimension
clamps have a literal Python mirror here, which tests/test_kernel_table.py compares with the header's expressions.  A geometry
added to a list becomes a new test case of tests/test_gpu_kernel_matrix.py without an edit to the tests.  Also here: the reader
of the APD_DEBUG_PLAN lines (which geometry took how many tiles), the only report of which kernel ran, the header's fast-path
feature range (kFeatureFloor, kFeatureBound) and the mixed-magnitude corpus that the CPU and the GPU range tests share.  For the
spotting kernels: kSpotRegisterRows, a mirror of kernel_dim / spot_rows_per_lane / spot_row_class, the list of instantiations
<RT, D> the header implies, and the reader of their own APD_DEBUG_PLAN lines.
"""
import contextlib
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio_pattern_discovery_amd", "csrc", "apd_internal.h")

# family -> (macro of its list, base of its integer code): KernelGeom::encode, base + first * 100 + second
FAMILIES = {
    "systolic": ("APD_SYSTOLIC_GEOMS", 0),
    "wide": ("APD_WIDE_GEOMS", 10000),
    "strip": ("APD_STRIP_GEOMS", 20000),
    "banded": ("APD_BANDED_STRIP_GEOMS", 30000),
    "shared": ("APD_SHARED_COLUMN_GEOMS", 40000),
}
CLAMPS = ("max_cells_per_lane", "max_strip_columns")


def header_text(path=HEADER):
    """The header with its backslash-newline continuations joined, as the preprocessor sees the macro bodies."""
    with open(path) as f:
        return re.sub(r"\\[ \t]*\r?\n", " ", f.read())


def parse_geoms(text, macro):
    """[(first, second)] of one '#define MACRO(X) X(a, b) X(c, d) ...' line."""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s\(X\)[ \t]+(.*)$" % re.escape(macro), text, re.M)
    if m is None:
        raise ValueError("no '#define %s(X) ...' in %s" % (macro, HEADER))
    body = m.group(1).split("//")[0]
    geoms = [(int(a), int(b)) for a, b in re.findall(r"\bX\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]
    left = re.sub(r"\bX\(\s*\d+\s*,\s*\d+\s*\)", "", body).strip()
    if left:
        raise ValueError("%s: not a list of X(a, b) entries: %r" % (macro, left))
    return geoms


def parse_dims(text):
    m = re.search(r"\bkKernelDims\[\]\s*=\s*\{([^}]*)\}", text)
    if m is None:
        raise ValueError("no 'kKernelDims[] = {...}' in %s" % HEADER)
    return [int(v) for v in m.group(1).split(",") if v.strip()]


def parse_table(text=None):
    """({family: [(first, second)]}, [kernel dims]) of the header."""
    text = header_text() if text is None else text
    return {fam: parse_geoms(text, macro) for fam, (macro, _) in FAMILIES.items()}, parse_dims(text)


# ---- literal mirror of the header's per-dimension clamps (compared with the header text by tests/test_kernel_table.py)
def max_cells_per_lane(d):
    return 9 if d <= 13 else (7 if d <= 16 else 5)


def max_strip_columns(d):
    return 13 if d <= 10 else (11 if d <= 13 else max_cells_per_lane(d))


def encode(family, first, second):
    return FAMILIES[family][1] + first * 100 + second


def decode(code):
    """KernelGeom::decode: (family, first, second), or None for the codes that name the generic kernel."""
    for fam, (_, base) in FAMILIES.items():
        lo = 100 if fam == "systolic" else base
        if lo <= code < base + 10000:
            return fam, (code % 10000) // 100, code % 100
    return None


def instantiated(family, first, second, dim):
    """geom_instantiated for a listed geometry at a kernel dimension: within the dimension's clamp."""
    return second <= (max_strip_columns(dim) if family == "strip" else max_cells_per_lane(dim))


def capacity(family, first, second):
    """KernelGeom::capacity: band offsets one pair covers (band form); for the strips, columns per pass G * CW."""
    if family in ("strip", "banded"):
        return (64 // first) * second
    return (64 if family == "wide" else 1) * first * second


def default_tau(text=None):
    """The hybrid form's recomputation threshold a fresh context holds: 'float tau = <a>f / <b>f;' of the header's context."""
    text = header_text() if text is None else text
    m = re.search(r"\bfloat\s+tau\s*=\s*([0-9.]+)f\s*/\s*([0-9.]+)f\s*;", text)
    if m is None:
        raise ValueError("no 'float tau = <a>f / <b>f;' in %s" % HEADER)
    return float(np.float32(m.group(1)) / np.float32(m.group(2)))


# literal mirror of launch_align's "part.hybrid = ..." (csrc/dtw_generic.hip) and of what admits the families that it asks for unit
# penalties: launch_systolic's "unit && L.hybrid", the wide and strip kernels' "L.band.mat == 1.0f" under equal penalties
def hybrid_live(family, dim, pens=(1.0, 1.0, 1.0), strict=False):
    """True if hybrid mode launches the norm-expansion form (the one with the tau gate) of `family` at kernel dimension dim."""
    if strict or tuple(float(p) for p in pens) != (1.0, 1.0, 1.0):
        return False
    return dim >= (8 if family in ("systolic", "shared") else 10)


def pairs(table=None):
    """([(family, first, second, dim)] that exist, [...] that the dimension's clamp drops), in header order."""
    geoms, dims = parse_table() if table is None else table
    have, dropped = [], []
    for fam in FAMILIES:
        for a, b in geoms[fam]:
            for d in dims:
                (have if instantiated(fam, a, b, d) else dropped).append((fam, a, b, d))
    return have, dropped


# ---- the header's own clamp expressions, evaluated: integers, the parameter, <=, <, ?:, parentheses, calls of the other clamp
def clamp_source(text, name):
    """(parameter name, expression text, 1-based line number) of 'constexpr int NAME(uint32_t d) { return EXPR; }'."""
    m = re.search(r"constexpr\s+int\s+%s\s*\(\s*uint32_t\s+(\w+)\s*\)\s*\{\s*return\s+([^;]*);\s*\}" % re.escape(name), text)
    if m is None:
        raise ValueError("no 'constexpr int %s(uint32_t d) { return ...; }' in %s" % (name, HEADER))
    return m.group(1), m.group(2).strip(), text.count("\n", 0, m.start()) + 1


def eval_clamp(text, name, d):
    """The value of the header's clamp `name` at dimension d."""
    param, expr, line = clamp_source(text, name)
    toks = re.findall(r"\d+|\w+|<=|<|[?:()]", expr)
    if "".join(toks) != re.sub(r"\s+", "", expr):
        raise ValueError("%s:%d: %s: cannot read %r" % (HEADER, line, name, expr))
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else None

    def take(want=None):
        t = peek()
        if t is None or (want is not None and t != want):
            raise ValueError("%s:%d: %s: cannot read %r (at token %d)" % (HEADER, line, name, expr, pos[0]))
        pos[0] += 1
        return t

    def primary():
        t = take()
        if t == "(":
            v = ternary()
            take(")")
            return v
        if t.isdigit():
            return int(t)
        if t == param:
            return d
        if t in CLAMPS and t != name and peek() == "(":
            take("(")
            arg = ternary()
            take(")")
            return eval_clamp(text, t, arg)
        raise ValueError("%s:%d: %s: unknown name %r in %r" % (HEADER, line, name, t, expr))

    def compare():
        v = primary()
        while peek() in ("<=", "<"):
            op, rhs = take(), primary()
            v = int(v <= rhs if op == "<=" else v < rhs)
        return v

    def ternary():
        c = compare()
        if peek() == "?":
            take("?")
            a = ternary()
            take(":")
            b = ternary()
            return a if c else b
        return c

    v = ternary()
    if peek() is not None:
        raise ValueError("%s:%d: %s: trailing %r in %r" % (HEADER, line, name, peek(), expr))
    return v


def read_plan(stderr_text):
    """{geometry code: tiles} of the '[apd] rank r/w: geometry <code>: <n> tiles, ...' lines APD_DEBUG_PLAN=1 prints per tile plan."""
    plan = {}
    for code, tiles in re.findall(r"geometry (\d+): (\d+) tiles", stderr_text):
        plan[int(code)] = plan.get(int(code), 0) + int(tiles)
    return plan


# ---- the spotting kernels: spot_kernel<SpotSweep, RT, D> and spot_kernel<SpotRecordSweep, RT, D> (csrc/dtw_spot.hip, csrc/dtw_spot_path.hip)
SPOT_KINDS = ("sweep", "record")


def parse_spot_register_rows(text=None):
    """kSpotRegisterRows of the header: the most query rows per lane the spotting kernels hold in registers."""
    text = header_text() if text is None else text
    m = re.search(r"constexpr\s+uint32_t\s+kSpotRegisterRows\s*=\s*(\d+)\s*;", text)
    if m is None:
        raise ValueError("no 'constexpr uint32_t kSpotRegisterRows = <n>;' in %s" % HEADER)
    return int(m.group(1))


# literal mirror of the header's kernel_dim, spot_rows_per_lane and spot_row_class (hand values: tests/test_kernel_table.py)
def kernel_dim(d, dims=None):
    """The resident frame dimension of a batch of dimension d: the first kernel dimension >= d, else d itself."""
    for k in parse_dims(header_text()) if dims is None else dims:
        if k >= d:
            return k
    return d


def spot_rows_per_lane(n):
    return (n + 63) // 64


def spot_row_class(dim, n, dims=None, register_rows=None):
    """The RT a query of n frames runs with at RESIDENT dimension dim: its rows per lane in registers, or 0 (lane columns in LDS)."""
    dims = parse_dims(header_text()) if dims is None else dims
    register_rows = parse_spot_register_rows() if register_rows is None else register_rows
    r = spot_rows_per_lane(n)
    return r if dim in dims and r <= register_rows else 0


def spot_row_n(n):
    """(lane, row of the lane) that hold query row n: spot_sweep's lane_n and r_n."""
    r = spot_rows_per_lane(n)
    return (n - 1) // r, (n - 1) % r


def spot_kernels(text=None):
    """[(RT, D)] of every instantiation the header implies, for the sweep and for the recording sweep alike: RT = 1 ..
    kSpotRegisterRows and 0 at every kernel dimension, and <0, 0> for any other dimension."""
    text = header_text() if text is None else text
    rows = parse_spot_register_rows(text)
    return [(rt, d) for d in parse_dims(text) for rt in list(range(1, rows + 1)) + [0]] + [(0, 0)]


_SPOT_LINE = re.compile(r"\[apd\] spot (\w+) kernel <(\d+), (\d+)>: (\d+) pairs(?:, r_max (\d+), lds (\d+) bytes)?")


def read_spot_launches(stderr_text):
    """One dict per '[apd] spot <kind> kernel <RT, D>: <n> pairs[, r_max <r>, lds <b> bytes]' line of APD_DEBUG_PLAN=1, in order:
    kind, rt, d, pairs, and for the LDS class r_max and lds (None for the register classes)."""
    out = []
    for kind, rt, d, pairs, r_max, lds in _SPOT_LINE.findall(stderr_text):
        out.append(dict(kind=kind, rt=int(rt), d=int(d), pairs=int(pairs), r_max=int(r_max) if r_max else None,
                        lds=int(lds) if lds else None))
    return out


def read_spot_plan(stderr_text):
    """{(kind, RT, D): pairs} of the spotting kernels' APD_DEBUG_PLAN lines: which instantiation took how many pairs."""
    plan = {}
    for launch in read_spot_launches(stderr_text):
        key = (launch["kind"], launch["rt"], launch["d"])
        plan[key] = plan.get(key, 0) + launch["pairs"]
    return plan


@contextlib.contextmanager
def debug_plan(capfd):
    """The body runs under APD_DEBUG_PLAN=1; the yielded list holds the stderr it wrote once the body has ended."""
    captured = []
    os.environ["APD_DEBUG_PLAN"] = "1"
    capfd.readouterr()
    try:
        yield captured
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
        captured.append(capfd.readouterr().err)


# ---- the fast kernels' feature range, and the corpus that leaves it at both ends
def feature_range(text=None):
    """(kFeatureFloor, kFeatureBound) of the header: a batch is flagged for the literal kernel when a non-zero feature has a
    magnitude outside [floor, bound)."""
    text = header_text() if text is None else text
    out = []
    for name in ("kFeatureFloor", "kFeatureBound"):
        m = re.search(r"constexpr\s+float\s+%s\s*=\s*(0x1p[+-]?\d+)f\s*;" % name, text)
        if m is None:
            raise ValueError("no 'constexpr float %s = 0x1p<e>f;' in %s" % (name, HEADER))
        out.append(float.fromhex(m.group(1)))
    return tuple(out)


def leaves_fast_range(frames, text=None):
    """What pad_frames_kernel decides for these frames: True if one of them is NaN, infinite, non-zero below the floor or at /
    beyond the bound."""
    lo, hi = feature_range(text)
    a = np.abs(np.asarray(frames, np.float32))
    return bool(np.any(~(a < np.float32(hi)) | ((a != 0) & (a < np.float32(lo)))))


def mixed_magnitude_corpus(n_seq=20, length=90, dim=13, seed=5):
    """The corpus of tests/test_gpu_sqrt.py::test_strict_distance_bits_with_tiny_zero_and_huge_differences (the defaults give its
    very values): O(1) Gaussian sequences, an identical pair, copies scaled by 1e-30 (squares underflow), that copy shifted by
    1e-38, by 3e-20, 2e-15 and 1e17, and a sequence sharing every third frame with sequence 0.  [n_seq][length][dim] f32."""
    assert n_seq >= 8
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n_seq, length, dim)).astype(np.float32)
    base[1] = base[0]
    base[2] = base[0] * np.float32(1e-30)
    base[3] = base[2] + np.float32(1e-38)
    base[4, ::3] = base[0, ::3]
    base[5] = base[0] * np.float32(3e-20)
    base[6] = base[0] * np.float32(2e-15)
    base[7] = base[0] * np.float32(1e17)
    return base
