"""Timing of the device LU (np_lu.hip): getrf, inverse and solve (one right-hand side) over n, after a GEMM warm-up
that covers the clock ramp.  getrf is timed together with the copy that restores its input (2 n^2 floats, included).
Prints ms per call, TFLOP/s (2/3 n^3 for getrf, 2 n^3 for the inverse, 2/3 n^3 + 2 n^2 for solve), kernel launches per
call, and numpy's fp32 solve on the host for comparison (the median of a few calls after a warm-up call).  The share of the trailing GEMMs comes from a run under
`rocprofv3 --kernel-trace --stats` (profiles/linalg/).  Usage: python tools/linalg_sweep.py [--sizes 64,256,...] [--reps N]

--cholesky runs the Cholesky leg instead (profiles/linalg/cholesky_sweep.log): np_potrf against np_getrf of the same run at
the same n and on the same matrix (A = X X^T / n + I), both timed with the copy that restores their input; TFLOP/s over
n^3 / 3 and 2/3 n^3; the residual ||A - L L^T||_1 / ||A||_1 of np_cholesky's factor in float64 over eps = 2^-23 next to
that of numpy's fp32 cholesky, and numpy's time on the host (the median of five calls after a warm-up), up to n = 8192.
--no-host leaves the host work out (a run under the profiler).

--svd runs the SVD leg (profiles/linalg/svd_sweep.log): np_svd and np_svdvals on G + 2 sqrt(n) I (and a plain Gaussian
4096 x 512), ms per call, sweeps taken, launches per call, numpy's fp32 svd on the host in the same run (median after a
warm-up); it ends with the gate "the device call at n = 2048 is faster than numpy's".  --svd --accuracy prints instead the four
metrics of tests/svd_family.py for every input of the bound tests next to their limits (profiles/linalg/svd_accuracy.log).
The SVD leg imports tests/svd_family.py: the inputs, the metrics and the CPU emulator have that one definition, which the tests
use too.  Sizes of up to 64 are timed twice, on the one-launch path and with it switched off (np_debug_svd_small_path).

--eigh runs the symmetric eigensolver's leg (profiles/linalg/eigh_sweep.log): np_eigh and np_eigvalsh on the seeded random symmetric
matrix of tests/eig_family.py, ms per call (the median of single calls after two untimed ones), sweeps taken, launches per call, the three metrics of tests/eig_family.py in
n eps, np_svd of the same matrix in the same run (the same machinery plus a Gram step) and numpy's fp32 eigh on the host (median
of five after a warm-up).  Sizes of up to 64 are timed on the blocked path too (np_debug_eigh_small_path).

--qr runs the Householder QR's leg (profiles/linalg/qr_sweep.log): np_geqrf (timed with the copy that restores its input), np_qr and
np_lstsq with one and with 64 right-hand sides on a seeded Gaussian matrix at the squares of --sizes and at 16384 x 128 and 65536 x 64,
ms per call (the median of single calls after two untimed ones), TFLOP/s of np_geqrf over 2 n^2 (m - n / 3), launches per call, res and
orth of np_qr's factors in sqrt(n) eps (tests/qr_family.py), np_getrf (squares) and np_svd (up to 4096 columns) of the same matrix in the same
run, and the host's float32 QR: SciPy's (LAPACK sgeqrf + sorgqr) when it imports, otherwise numpy's, which computes in float64 and
rounds.  --no-host times np_geqrf alone (a run under the profiler).

--digest times nothing: one line per call with its info and a sha256 of everything it wrote, for a fixed list of seeded inputs that
reaches every path of the LU, the Cholesky, the SVD and the eigensolver (np_lu.hip, np_cholesky.hip, np_jacobi.hip).  Two builds
of the library compute the same bits exactly when the two outputs are the same text: run it once as it is and once with
NP_HIP_LIB=<the other libnp_hip.so>, each in a process of its own, and diff (profiles/linalg/split_digest.log)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
from numpower_amd import device as D
from numpower_amd._lib import Timer, check, load

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default=None, help="default 64,256,1024,4096,8192,16384 (with --cholesky also 128)")
ap.add_argument("--cholesky", action="store_true", help="the Cholesky leg: np_potrf against np_getrf")
ap.add_argument("--svd", action="store_true", help="the SVD leg: np_svd / np_svdvals against numpy's svd on the host")
ap.add_argument("--eigh", action="store_true", help="the eigensolver's leg: np_eigh / np_eigvalsh against np_svd and numpy's eigh")
ap.add_argument("--qr", action="store_true", help="the QR leg: np_geqrf / np_qr / np_lstsq against np_getrf, np_svd and the host's float32 QR")
ap.add_argument("--accuracy", action="store_true", help="with --svd: the accuracy table of the bound tests' inputs")
ap.add_argument("--digest", action="store_true", help="no timing: info and a sha256 of the outputs of a fixed list of calls")
ap.add_argument("--reps", type=int, default=0, help="0: as many as fit ~0.5 s per size (at least 3)")
ap.add_argument("--no-host", action="store_true", help="skip numpy's solve on the host")
args = ap.parse_args()
if args.sizes is None and args.eigh:
    args.sizes = "8,32,64,128,256,512,1024,2048,4096"
if args.sizes is None and args.qr:
    args.sizes = "512,1024,2048,4096,8192"
if args.sizes is None and args.svd:
    args.sizes = "8,32,64,256,1024,2048,4096"
if args.sizes is None:
    args.sizes = "64,128,256,1024,4096,8192,16384" if args.cholesky else "64,256,1024,4096,8192,16384"

D.init(0)
lib = load()
t = Timer()


def launches():
    c = C.c_ulonglong()
    check(lib.np_debug_launch_count(C.byref(c)))
    return c.value


def timed(fn, reps):
    fn()
    D.sync()
    l0 = launches()
    fn()
    D.sync()
    per_call = launches() - l0
    t.start()
    for _ in range(reps):
        fn()
    t.stop()
    return t.elapsed_ms() / reps, per_call


if args.digest:
    import hashlib
    from tests import eig_family as E
    from tests import svd_family as F

    def line(name, info, outs):
        h = hashlib.sha256()
        for o in outs:
            h.update(np.ascontiguousarray(o.to_host()).tobytes())
        print("%-44s info %-6d sha256 %s" % (name, info, h.hexdigest()), flush=True)

    def dev_int(d):
        return int(d.to_host().view(np.int32).reshape(-1)[0])

    ih = C.c_int()
    # LU: the LDS path and its edge (5, 128), the first blocked size, a ragged last panel, two rows per thread in the panel
    for n in (5, 128, 129, 200, 1030):
        rng = np.random.default_rng(51000 + n)
        g = rng.standard_normal((n, n)).astype(np.float32)
        b3 = rng.standard_normal((n, 3)).astype(np.float32)
        for tag, a in (("gaussian", g), ("gaussian + n I", g + np.float32(n) * np.eye(n, dtype=np.float32))):
            da = D.DeviceArray.from_host(a)
            o1, o2, o3, det = D.DeviceArray((n, n)), D.DeviceArray((n, n)), D.DeviceArray((n, n)), D.DeviceArray((1,))
            check(lib.np_det(da.ptr, n, det.ptr))
            line("np_det %d %s" % (n, tag), 0, [det])
            check(lib.np_inverse(da.ptr, n, o1.ptr, C.byref(ih)))
            line("np_inverse %d %s" % (n, tag), ih.value, [o1])
            for nrhs in (1, 3):
                db, dx = D.DeviceArray.from_host(np.ascontiguousarray(b3[:, :nrhs])), D.DeviceArray((n, nrhs))
                check(lib.np_solve(da.ptr, db.ptr, n, nrhs, dx.ptr, C.byref(ih)))
                line("np_solve %d nrhs %d %s" % (n, nrhs, tag), ih.value, [dx])
                db.free()
                dx.free()
            check(lib.np_lu(da.ptr, n, o1.ptr, o2.ptr, o3.ptr))
            line("np_lu %d %s" % (n, tag), 0, [o1, o2, o3])
            for d in (da, o1, o2, o3, det):
                d.free()
    # Cholesky: the single-kernel path, the first blocked size, ragged, several strips (a Gaussian's lower triangle fails: info > 0)
    for n in (64, 65, 200, 600):
        g = np.random.default_rng(52000 + n).standard_normal((n, n)).astype(np.float32)
        for tag, a in (("gaussian", g), ("gaussian + n I", g + np.float32(n) * np.eye(n, dtype=np.float32))):
            da, work, out, info = D.DeviceArray.from_host(a), D.DeviceArray((n, n)), D.DeviceArray((n, n)), D.DeviceArray((1,))
            check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * n * n))
            check(lib.np_potrf(work.ptr, n, info.ptr))
            line("np_potrf %d %s" % (n, tag), dev_int(info), [work])
            check(lib.np_memset0(out.ptr, 4 * n * n))   # past a failing column np_cholesky leaves what was there
            check(lib.np_cholesky(da.ptr, n, out.ptr, C.byref(ih)))
            line("np_cholesky %d %s" % (n, tag), ih.value, [out])
            for d in (da, work, out, info):
                d.free()
    # SVD: the one-launch path, then the blocked one (64 x 64 with the one-launch path off first)
    svd_cases = [((1, 1), 1), ((3, 7), 1), ((64, 64), 1), ((64, 64), 0), ((65, 65), 1), ((64, 200), 1), ((200, 64), 1), ((130, 64), 1),
                 ((300, 300), 1), ((129, 257), 1)]
    for (m, n), small in svd_cases:
        a = F.shifted_square(n) if m == n and n != 300 else F.gaussian(m, n)
        k = min(m, n)
        da, du, ds, dv = D.DeviceArray.from_host(a), D.DeviceArray((m, k)), D.DeviceArray((k,)), D.DeviceArray((k, n))
        note = "" if small else " small path off"
        check(lib.np_debug_svd_small_path(small))
        check(lib.np_svd(da.ptr, m, n, du.ptr, ds.ptr, dv.ptr, C.byref(ih)))
        line("np_svd %d x %d%s" % (m, n, note), ih.value, [du, ds, dv])
        check(lib.np_svdvals(da.ptr, m, n, ds.ptr, C.byref(ih)))
        line("np_svdvals %d x %d%s" % (m, n, note), ih.value, [ds])
        check(lib.np_debug_svd_small_path(1))
        for d in (da, du, ds, dv):
            d.free()
    # eigensolver: the one-launch path, then the blocked one
    eigh_cases = [(E.random_symmetric, n, 1) for n in (1, 5, 64)] + [(E.random_symmetric, 64, 0)]
    eigh_cases += [(E.random_symmetric, n, 1) for n in (65, 130, 257)] + [(E.graded, 130, 1)]
    for family, n, small in eigh_cases:
        da, dw, dv = D.DeviceArray.from_host(family(n)), D.DeviceArray((n,)), D.DeviceArray((n, n))
        note = "%s%s" % (family.__name__, "" if small else " small path off")
        check(lib.np_debug_eigh_small_path(small))
        check(lib.np_eigh(da.ptr, n, dw.ptr, dv.ptr, C.byref(ih)))
        line("np_eigh %d %s" % (n, note), ih.value, [dw, dv])
        check(lib.np_eigvalsh(da.ptr, n, dw.ptr, C.byref(ih)))
        line("np_eigvalsh %d %s" % (n, note), ih.value, [dw])
        check(lib.np_debug_eigh_small_path(1))
        for d in (da, dw, dv):
            d.free()
    sym = E.random_symmetric(130)
    for tag, a in (("symmetric", sym), ("not symmetric", np.triu(sym) + 2 * np.tril(sym, -1))):
        da = D.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.float32))
        check(lib.np_symmetry_mismatch(da.ptr, 130, C.byref(ih)))
        print("%-44s any  %d" % ("np_symmetry_mismatch 130 %s" % tag, ih.value), flush=True)
        da.free()
    sys.exit(0)


# clock ramp: ~1 s of 4096^3 GEMMs
ga = D.DeviceArray.from_host(np.random.default_rng(0).standard_normal((4096, 4096)).astype(np.float32))
gc = D.DeviceArray((4096, 4096))
t0 = time.time()
while time.time() - t0 < 1.0:
    for _ in range(10):
        check(lib.np_sgemm(4096, 4096, 4096, ga.ptr, ga.ptr, gc.ptr))
    D.sync()
ga.free()
gc.free()



def timed_median(fn, reps):
    """median ms of `reps` single calls after two untimed ones, and the launches of a call; fn must block until its result is known
    (np_eigh, np_eigvalsh and np_svd do: they hand info to the host), so a host clock around the call measures it"""
    fn()
    l0 = launches()
    fn()
    per_call = launches() - l0
    ts = []
    for _ in range(reps):
        D.sync()
        h0 = time.perf_counter()
        fn()
        D.sync()
        ts.append((time.perf_counter() - h0) * 1e3)
    return float(np.median(ts)), per_call


def reps_for(fn):
    t0 = time.time()
    fn()
    D.sync()
    return args.reps or max(3, min(200, int(0.5 / max(time.time() - t0, 1e-5))))


def residual_over_eps(a64, l):
    l64 = l.astype(np.float64)
    return float(np.abs(a64 - l64 @ l64.T).sum(axis=0).max() / np.abs(a64).sum(axis=0).max()) * 2.0 ** 23


if args.qr:
    from tests import qr_family as Q
    try:
        from scipy.linalg import qr as host_qr
        host_name, host_kw = "scipy float32 qr (sgeqrf + sorgqr)", {"mode": "economic"}
    except ImportError:
        host_qr, host_name, host_kw = np.linalg.qr, "numpy qr (float64 arithmetic, rounded to float32)", {}

    squares = [int(x) for x in args.sizes.split(",")]
    shapes = [(n, n) for n in squares] + ([(16384, 128), (65536, 64)] if len(squares) > 1 else [])
    print("%13s %9s %8s %8s %9s %11s %12s %9s %9s  %-15s %s" % ("m x n", "geqrf ms", "TFLOP/s", "launches", "np_qr ms", "lstsq(1) ms", "lstsq(64) ms",
                                                               "getrf ms", "np_svd ms", "res / orth", "host " + host_name), flush=True)
    for m, n in shapes:
        a = Q.gaussian(m, n)
        b = Q.gaussian(m, 64, 9)
        da, work, dtau = D.DeviceArray.from_host(a), D.DeviceArray((m, n)), D.DeviceArray((n,))
        ih = C.c_int()

        def geqrf():
            check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * m * n))
            check(lib.np_geqrf(work.ptr, m, n, dtau.ptr))

        reps = args.reps or (5 if m * n <= 4096 * 4096 else 2)
        g_ms, g_launches = timed_median(geqrf, reps)
        cells = ["-"] * 6
        host = "-"
        if not args.no_host:
            dq, dr = D.DeviceArray((m, n)), D.DeviceArray((n, n))
            db1, db64 = D.DeviceArray.from_host(np.ascontiguousarray(b[:, :1])), D.DeviceArray.from_host(b)
            dx = D.DeviceArray((n, 64))
            piv, info = D.DeviceArray((n,)), D.DeviceArray((1,))

            def qr():
                check(lib.np_qr(da.ptr, m, n, dq.ptr, dr.ptr))

            def lstsq1():
                check(lib.np_lstsq(da.ptr, db1.ptr, m, n, 1, dx.ptr, C.byref(ih)))

            def lstsq64():
                check(lib.np_lstsq(da.ptr, db64.ptr, m, n, 64, dx.ptr, C.byref(ih)))

            def getrf():
                check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * n * n))
                check(lib.np_getrf(work.ptr, n, piv.ptr, info.ptr))

            cells[0] = "%.3f" % timed_median(qr, reps)[0]
            got = Q.growth(a, dq.to_host(), dr.to_host())
            cells[1] = "%.3f" % timed_median(lstsq1, reps)[0]
            cells[2] = "%.3f" % timed_median(lstsq64, reps)[0]
            assert ih.value == 0
            if m == n:
                cells[3] = "%.3f" % timed_median(getrf, reps)[0]
            if n <= 4096:
                k = min(m, n)
                du, ds, dv = D.DeviceArray((m, k)), D.DeviceArray((k,)), D.DeviceArray((k, n))

                def svd():
                    check(lib.np_svd(da.ptr, m, n, du.ptr, ds.ptr, dv.ptr, C.byref(ih)))

                cells[4] = "%.3f" % timed_median(svd, 1 if n >= 2048 else 3)[0]
                for d in (du, ds, dv):
                    d.free()
            cells[5] = "%.3f / %.3f" % (got["res"], got["orth"])
            host_qr(a, **host_kw)                       # warm-up
            ts = []
            for _ in range(3):
                h0 = time.perf_counter()
                host_qr(a, **host_kw)
                ts.append((time.perf_counter() - h0) * 1e3)
            host = "%.3f ms (median of 3 after a warm-up)" % float(np.median(ts))
            for d in (dq, dr, db1, db64, dx, piv, info):
                d.free()
        print("%6d x %-5d %9.3f %8.2f %8d %9s %11s %12s %9s %9s  %-15s %s" % (
            m, n, g_ms, 2.0 * n * n * (m - n / 3.0) / g_ms / 1e9, g_launches, cells[0], cells[1], cells[2], cells[3], cells[4], cells[5], host), flush=True)
        for d in (da, work, dtau):
            d.free()
    sys.exit(0)

if args.eigh:
    from tests import eig_family as E

    print("%6s %10s %14s %7s %9s %10s %11s   %-22s %s" % ("n", "np_eigh ms", "np_eigvalsh ms", "sweeps", "launches", "np_svd ms", "svd sweeps",
                                                         "res / orth / werr (n eps)", "host numpy fp32 eigh"), flush=True)
    for n in [int(x) for x in args.sizes.split(",")]:
        a = E.random_symmetric(n)
        da, dw, dv, du = D.DeviceArray.from_host(a), D.DeviceArray((n,)), D.DeviceArray((n, n)), D.DeviceArray((n, n))
        ih, sw, ssw = C.c_int(), C.c_int(), C.c_int()

        def eigh():
            check(lib.np_eigh(da.ptr, n, dw.ptr, dv.ptr, C.byref(ih)))

        def eigvalsh():
            check(lib.np_eigvalsh(da.ptr, n, dw.ptr, C.byref(ih)))

        def svd():
            check(lib.np_svd(da.ptr, n, n, du.ptr, dw.ptr, dv.ptr, C.byref(ih)))

        rows = [("", 1)] + ([(" (the one-launch path switched off)", 0)] if n <= 64 else [])
        for note, small in rows:
            check(lib.np_debug_eigh_small_path(small))
            ms, per_call = timed_median(eigh, reps_for(eigh))
            check(lib.np_debug_eigh_last_sweeps(C.byref(sw)))
            assert ih.value == 0
            got = E.metrics(a, dw.to_host().reshape(n), dv.to_host().reshape(n, n))
            msv, _ = timed_median(eigvalsh, reps_for(eigvalsh))
            check(lib.np_debug_eigh_small_path(1))
            mss, _ = timed_median(svd, reps_for(svd))
            check(lib.np_debug_svd_last_sweeps(C.byref(ssw)))
            host = "-"
            if not args.no_host and not note:
                np.linalg.eigh(a)                   # warm-up
                ts = []
                for _ in range(5):
                    h0 = time.perf_counter()
                    np.linalg.eigh(a)
                    ts.append((time.perf_counter() - h0) * 1e3)
                host = "%.3f ms (median of 5 after a warm-up)" % float(np.median(ts))
            print("%6d %10.3f %14.3f %7d %9d %10.3f %11d   %-22s %s%s" % (
                n, ms, msv, sw.value, per_call, mss, ssw.value,
                " / ".join("%.3f" % (got[k] / (n * E.EPS)) for k in E.METRICS), host, note), flush=True)
        for d in (da, dw, dv, du):
            d.free()
    sys.exit(0)

if args.svd:
    from tests import svd_family as F

    def svd_call(a, vals=False):
        m, n = a.shape
        k = min(m, n)
        da, du, ds, dv = D.DeviceArray.from_host(a), D.DeviceArray((m, k)), D.DeviceArray((k,)), D.DeviceArray((k, n))
        ih, sw = C.c_int(), C.c_int()

        def run():
            if vals:
                check(lib.np_svdvals(da.ptr, m, n, ds.ptr, C.byref(ih)))
            else:
                check(lib.np_svd(da.ptr, m, n, du.ptr, ds.ptr, dv.ptr, C.byref(ih)))

        return run, (da, du, ds, dv), ih, sw

    if args.accuracy:
        cases = [("shifted", F.shifted_square(n), None, 0) for n in F.SQUARE_SIZES]
        cases += [("gaussian", F.gaussian(*s), None, 0) for s in F.RECT_SHAPES]
        cases += [("scaled", F.scaled_case(*s), None, 0) for s in F.SCALED_SHAPES]
        cases += [("rank%d" % r, F.rank_case(m, n, r), None, min(m, n) - r) for m, n, r in F.RANK_CASES]
        cases += [("hadamard",) + F.hadamard_case(*s) + (0,) for s in F.HADAMARD_SHAPES]
        print("figures in eps = 2^-23: rec / orthA / orthN / serr of the device, then of the limit (4 x the CPU emulator, floored at 2, up to "
              "max(m, n) = 512; max(m, n) / 2 above)", flush=True)
        for name, a, sigma, excluded in cases:
            m, n = a.shape
            run, bufs, ih, sw = svd_call(a)
            run()
            check(lib.np_debug_svd_last_sweeps(C.byref(sw)))
            got = F.metrics(a, bufs[1].to_host().reshape(m, -1), bufs[2].to_host().reshape(-1), bufs[3].to_host().reshape(-1, n), sigma)
            if max(m, n) <= 512:
                ref = F.metrics(a, *F.jacobi_svd_emulated(a)[:3], sigma)
                lim = {k: max(2.0, 4 * ref[k] / F.EPS) for k in ("rec", "orthA", "orthN", "serr")}
            else:
                lim = {k: max(m, n) / 2 for k in ("rec", "orthA", "orthN", "serr")}
            keys = ("rec", "orthA", "orthN", "serr")
            worst = max(got[k] / F.EPS / lim[k] for k in keys)
            print("%-9s %5d x %-5d info %d sweeps %2d live %4d/%-4d  device %s  limit %s  worst ratio %.2f" %
                  (name, m, n, ih.value, sw.value, got["live"], min(m, n) - excluded, " / ".join("%.1f" % (got[k] / F.EPS) for k in keys),
                   " / ".join("%.1f" % lim[k] for k in keys), worst), flush=True)
            for d in bufs:
                d.free()
        sys.exit(0)

    print("%13s %10s %12s %7s %9s   %s" % ("m x n", "np_svd ms", "np_svdvals ms", "sweeps", "launches", "host numpy fp32 svd"), flush=True)
    shapes = [(int(s), int(s)) for s in args.sizes.split(",")] + ([(500, 64), (4096, 512)] if len(args.sizes.split(",")) > 1 else [])
    gate = None
    for m, n in shapes:
        a = F.shifted_square(n) if m == n else F.gaussian(m, n)
        run, bufs, ih, sw = svd_call(a)
        ms, per_call = timed(run, reps_for(run))
        check(lib.np_debug_svd_last_sweeps(C.byref(sw)))
        assert ih.value == 0
        runv, bufsv, ihv, _ = svd_call(a, vals=True)
        msv, _ = timed(runv, reps_for(runv))
        host, med = "-", None
        if not args.no_host:
            np.linalg.svd(a, full_matrices=False)      # warm-up
            ts = []
            for _ in range(5 if n <= 1024 else 3):
                h0 = time.perf_counter()
                np.linalg.svd(a, full_matrices=False)
                ts.append((time.perf_counter() - h0) * 1e3)
            med = float(np.median(ts))
            host = "%.3f ms (median of %d after a warm-up)" % (med, len(ts))
        if (m, n) == (2048, 2048) and med is not None:
            gate = (ms, med)
        print("%6d x %-5d %10.3f %12.3f %7d %9d   %s" % (m, n, ms, msv, sw.value, per_call, host), flush=True)
        if min(m, n) <= 64:   # the same shape on the blocked path
            check(lib.np_debug_svd_small_path(0))
            msb, per_b = timed(run, reps_for(run))
            check(lib.np_debug_svd_last_sweeps(C.byref(sw)))
            msvb, _ = timed(runv, reps_for(runv))
            check(lib.np_debug_svd_small_path(1))
            print("%6d x %-5d %10.3f %12.3f %7d %9d   (the one-launch path switched off)" % (m, n, msb, msvb, sw.value, per_b), flush=True)
        for d in bufs + bufsv:
            d.free()
    if gate:
        print("gate: np_svd at 2048 takes %.1f ms, numpy's fp32 svd on the host %.1f ms: %s" %
              (gate[0], gate[1], "faster" if gate[0] < gate[1] else "NOT faster"), flush=True)
        sys.exit(0 if gate[0] < gate[1] else 1)
    sys.exit(0)

if args.cholesky:
    print("%6s %10s %9s %9s %10s %9s %9s %7s %8s %8s   %s" % ("n", "potrf ms", "TFLOP/s", "launches", "getrf ms", "TFLOP/s", "launches",
                                                             "ratio", "r/eps", "ref/eps", "host numpy fp32 cholesky"), flush=True)
    for n in [int(s) for s in args.sizes.split(",")]:
        x = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
        a = x @ x.T / np.float32(n) + np.eye(n, dtype=np.float32)
        del x
        a = np.tril(a) + np.tril(a, -1).T
        da, work, piv, info = D.DeviceArray.from_host(a), D.DeviceArray((n, n)), D.DeviceArray((n,)), D.DeviceArray((1,))

        def potrf():
            check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * n * n))
            check(lib.np_potrf(work.ptr, n, info.ptr))

        def getrf():
            check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * n * n))
            check(lib.np_getrf(work.ptr, n, piv.ptr, info.ptr))

        p_ms, p_launches = timed(potrf, reps_for(potrf))
        assert int(info.to_host().view(np.int32)[0]) == 0
        g_ms, g_launches = timed(getrf, reps_for(getrf))
        r = ref = host = "-"
        if not args.no_host and n <= 8192:
            ih = C.c_int()
            check(lib.np_cholesky(da.ptr, n, work.ptr, C.byref(ih)))
            a64 = a.astype(np.float64)
            r = "%.3f" % residual_over_eps(a64, work.to_host())
            ref = "%.3f" % residual_over_eps(a64, np.linalg.cholesky(a))   # also the warm-up call
            ts = []
            for _ in range(5):
                h0 = time.perf_counter()
                np.linalg.cholesky(a)
                ts.append((time.perf_counter() - h0) * 1e3)
            host = "%.3f ms (median of 5 after a warm-up)" % float(np.median(ts))
        print("%6d %10.3f %9.2f %9d %10.3f %9.2f %9d %7.3f %8s %8s   %s"
              % (n, p_ms, n ** 3 / 3 / p_ms / 1e9, p_launches, g_ms, 2 / 3 * n ** 3 / g_ms / 1e9, g_launches, p_ms / g_ms, r, ref, host),
              flush=True)
        for d in (da, work, piv, info):
            d.free()
    sys.exit(0)

print("%6s %-8s %10s %9s %9s   %s" % ("n", "op", "ms", "TFLOP/s", "launches", "host numpy fp32 solve"), flush=True)
for n in [int(s) for s in args.sizes.split(",")]:
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n)).astype(np.float32)
    b = rng.standard_normal((n, 1)).astype(np.float32)
    da, db = D.DeviceArray.from_host(a), D.DeviceArray.from_host(b)
    work, out = D.DeviceArray((n, n)), D.DeviceArray((n, n))
    piv, info = D.DeviceArray((n,)), D.DeviceArray((1,))
    ih = C.c_int()

    def getrf():
        check(lib.np_memcpy_d2d(work.ptr, da.ptr, 4 * n * n))
        check(lib.np_getrf(work.ptr, n, piv.ptr, info.ptr))

    def inverse():
        check(lib.np_inverse(da.ptr, n, out.ptr, C.byref(ih)))

    def solve():
        check(lib.np_solve(da.ptr, db.ptr, n, 1, out.ptr, C.byref(ih)))

    for name, fn, flops in (("getrf", getrf, 2 / 3 * n ** 3), ("inv", inverse, 2 * n ** 3),
                            ("solve", solve, 2 / 3 * n ** 3 + 2 * n * n)):
        t0 = time.time()
        fn()
        D.sync()
        one = max(time.time() - t0, 1e-5)
        reps = args.reps or max(3, min(200, int(0.5 / one)))
        ms, per_call = timed(fn, reps)
        host = ""
        if name == "solve" and not args.no_host and n <= 8192:
            np.linalg.solve(a, b)                  # warm-up: the first call pays for thread start-up
            ts = []
            for _ in range(5 if n <= 4096 else 3):
                h0 = time.perf_counter()
                np.linalg.solve(a, b)
                ts.append((time.perf_counter() - h0) * 1e3)
            host = "%.3f ms (median of %d after a warm-up)" % (float(np.median(ts)), len(ts))
        print("%6d %-8s %10.3f %9.2f %9d   %s" % (n, name, ms, flops / ms / 1e9, per_call, host), flush=True)
    for x in (da, db, work, out, piv, info):
        x.free()
