"""Open-ended version of tests/test_gpu_feature_sweep.py, and the replay of one of its cases (run on the GPU box).

usage: python tools/debug/fuzz_features.py [n_cases] [seed]
       python tools/debug/fuzz_features.py --replay [stream:]SEED:K[:OP]

The first form draws n_cases (default 100) from tests/_feature_cases.py with the seeds seed * 1000, seed * 1000 + 1, ... (default
seed 1) and four times the suite's budget of checker cells per case: twelve feature cases per seed on one context, then four
stream scenarios on another, as the suite runs them.  One line per failure, then the count.

--replay reruns case K of SEED (a committed seed or one of the above; `stream:` for a stream scenario), as far as operation OP if
given, twice: on a fresh context, and on a context that has run the cases 0 .. K - 1 of the seed before it.  A failure in both runs
is a plain bug; one that needs the preceding cases reads state an earlier call left behind."""
import contextlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
BUDGET_FACTOR = 4


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def run(kind, ctx, case, oracle, stop_after=None):
    """None, or the failure as one line."""
    import test_gpu_feature_sweep as sweep
    try:
        with open(os.devnull, "w") as sink, contextlib.redirect_stdout(sink):     # the comparators print what they measured
            if kind == "feature":
                sweep.run_feature_case(ctx, oracle, case, setenv, stop_after)
            else:
                sweep.run_stream_case(ctx, case, stop_after)
    except AssertionError as e:                                     # a library error (a HIP fault among them) ends the run instead
        return "%s: %s" % (type(e).__name__, " ".join(str(e).split())[:600])
    finally:
        for name in ("APD_PATH_WORKSPACE_BYTES", "APD_SPOT_WORKSPACE_BYTES"):
            setenv(name, None)
    return None


def replay(spec):
    import _feature_cases as fc
    from audio_pattern_discovery_amd import _lib
    from oracle import binding as oracle
    parts = spec.split(":")
    kind = "feature"
    if parts[0] == "stream":
        kind, parts = "stream", parts[1:]
    seed, k = int(parts[0]), int(parts[1])
    stop_after = int(parts[2]) if len(parts) > 2 else None
    make = fc.feature_case if kind == "feature" else fc.stream_case
    budget = fc.CASE_BUDGET if seed in fc.FEATURE_SEEDS + fc.STREAM_SEEDS else BUDGET_FACTOR * fc.CASE_BUDGET
    failed = 0
    for label, before in (("fresh context", []), ("after cases 0 .. %d" % (k - 1), list(range(k)))):
        ctx = _lib.Context(0)
        try:
            for j in before:
                run(kind, ctx, make(seed, j, budget), oracle)
            line = run(kind, ctx, make(seed, k, budget), oracle, stop_after)
        finally:
            ctx.close()
        failed += line is not None
        print("%s: %s" % (label, line or "ok"), flush=True)
    return failed


def sweep(n_cases, seed):
    import _feature_cases as fc
    from audio_pattern_discovery_amd import _lib
    from oracle import binding as oracle
    done = fails = 0
    t0 = time.time()
    at = seed * 1000
    while done < n_cases:
        for kind, make, count in (("feature", fc.feature_case, fc.FEATURE_CASES_PER_SEED), ("stream", fc.stream_case, fc.STREAM_CASES_PER_SEED)):
            ctx = _lib.Context(0)
            try:
                for k in range(count):
                    if done >= n_cases:
                        break
                    line = run(kind, ctx, make(at, k, BUDGET_FACTOR * fc.CASE_BUDGET), oracle)
                    done += 1
                    if line:
                        fails += 1
                        print("FAIL %s %d:%d %s" % (kind, at, k, line), flush=True)
            finally:
                ctx.close()
        fc._FEATURE.clear()
        fc._STREAM.clear()
        print("seed", at, "cases", done, "fails", fails, "%.0fs" % (time.time() - t0), flush=True)
        at += 1
    print("done: cases", done, "fails", fails, "seeds", seed * 1000, "..", at - 1)
    return fails


if __name__ == "__main__":
    args = sys.argv[1:]
    if "-h" in args or "--help" in args:
        print(__doc__)
        sys.exit(0)
    try:
        if args and args[0] == "--replay":
            sys.exit(1 if replay(args[1]) else 0)
        sys.exit(1 if sweep(int(args[0]) if args else 100, int(args[1]) if len(args) > 1 else 1) else 0)
    except (IndexError, ValueError, OSError, ImportError, RuntimeError) as e:     # a malformed command line, no GPU or library here,
        print(__doc__)                                                           # or a library error: nothing more is started
        print("stopped: %s: %s" % (type(e).__name__, e))
        sys.exit(2)
