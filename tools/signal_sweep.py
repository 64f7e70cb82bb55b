"""Timing of the device 2-D correlation (np_signal.hip): np_correlate2d in 'same' mode under 'fill' on n x n images with
k x k windows, after a GEMM warm-up that covers the clock ramp.  Writes profiles/signal/conv2d_sweep.log (and prints it).

Per case: ms per call (device events around `reps` calls; conv and the project's own a + b on the same shape ALTERNATE, round
by round, and the median of the rounds is reported), the bytes the algorithm needs (8 per element: one read, one write) over
8 TB/s, the FMAs (k^2 per element) over the fp32 vector peak of 78.6 TFMA/s (157.3 TFLOP/s), which of the two bounds the
case, the share of that bound reached, and scipy.signal.correlate2d in fp32 on the host up to 4096^2 where SciPy is importable
(one call).

The one comparison that is a target: 3 x 3 on 8192^2 moves 8 B per element where a + b moves 12, so with its halo re-reads
and 9 FMAs per element it should take no longer than a + b on the same shape in the same run.  The last line states the
ratio and whether it holds.

Usage: python tools/signal_sweep.py [--sizes 1024,4096,...] [--windows 3,5,...] [--rounds N] [--no-host] [--out FILE]
--profile runs each case a few times only, without the host work, for a run under the kernel profiler."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
from numpower_amd import device as D
from numpower_amd._lib import BINARY_OPS, NP_FULL, Timer, check, load

HBM_BYTES_PER_S = 8.0e12
FMA_PER_S = 157.3e12 / 2

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,4096,8192,16384")
ap.add_argument("--windows", default="3,5,7,15,31,63")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-host", action="store_true", help="skip scipy.signal on the host")
ap.add_argument("--profile", action="store_true", help="three calls per case and nothing else")
ap.add_argument("--out", default=str(ROOT / "profiles" / "signal" / "conv2d_sweep.log"))
args = ap.parse_args()

D.init(0)
lib = load()
t = Timer()
lines = []


def say(line=""):
    print(line, flush=True)
    lines.append(line)


def window_ms(fn, reps):
    t.start()
    for _ in range(reps):
        fn()
    t.stop()
    return t.elapsed_ms() / reps


def reps_for(fn):
    fn()
    D.sync()
    t0 = time.time()
    fn()
    D.sync()
    return max(3, min(500, int(0.1 / max(time.time() - t0, 1e-5))))


if not args.profile:   # clock ramp: ~1 s of 4096^3 GEMMs
    ga = D.DeviceArray.from_host(np.random.default_rng(0).standard_normal((4096, 4096)).astype(np.float32))
    gc = D.DeviceArray((4096, 4096))
    t0 = time.time()
    while time.time() - t0 < 1.0:
        for _ in range(10):
            check(lib.np_sgemm(4096, 4096, 4096, ga.ptr, ga.ptr, gc.ptr))
        D.sync()
    ga.free()
    gc.free()

try:
    from scipy import signal as host_signal
except ImportError:
    host_signal = None

say("np_correlate2d, 'same' / 'fill', fp32; conv and add alternate, median of %d rounds" % args.rounds)
say("%6s %4s %10s %10s %8s %10s %10s %6s %7s %5s %10s" % ("n", "k", "conv ms", "add ms", "conv/add", "bytes ms", "fma ms", "bound", "share", "path", "scipy ms"))
rng = np.random.default_rng(1)
target = None
for n in (int(s) for s in args.sizes.split(",")):
    a = rng.standard_normal((n, n)).astype(np.float32)
    da, db2, do = D.DeviceArray.from_host(a), D.DeviceArray.from_host(a), D.DeviceArray((n, n))
    for k in (int(s) for s in args.windows.split(",")):
        w = rng.standard_normal((k, k)).astype(np.float32)
        dw = D.DeviceArray.from_host(w)

        def conv():
            check(lib.np_correlate2d(da.ptr, n, n, dw.ptr, k, k, 1, 0, C.c_float(0.0), 0, do.ptr))

        def add():
            check(lib.np_binary(BINARY_OPS["add"], da.ptr, NP_FULL, db2.ptr, NP_FULL, do.ptr, n, n, 0, 0))

        if args.profile:
            for _ in range(3):
                conv()
                add()
            D.sync()
            dw.free()
            continue
        rc, ra = reps_for(conv), reps_for(add)
        conv_ms, add_ms = [], []
        for _ in range(args.rounds):
            conv_ms.append(window_ms(conv, rc))
            add_ms.append(window_ms(add, ra))
        cm, am = statistics.median(conv_ms), statistics.median(add_ms)
        path = C.c_int()
        check(lib.np_debug_conv2d_last_path(C.byref(path)))
        bytes_ms = 8.0 * n * n / HBM_BYTES_PER_S * 1e3
        fma_ms = float(k * k) * n * n / FMA_PER_S * 1e3
        bound = "HBM" if bytes_ms >= fma_ms else "VALU"
        host_ms = ""
        if host_signal is not None and not args.no_host and n <= 4096 and k <= 15:
            t0 = time.time()
            host_signal.correlate2d(a, w, "same", "fill")
            host_ms = "%.0f" % ((time.time() - t0) * 1e3)
        say("%6d %4d %10.4f %10.4f %8.3f %10.4f %10.4f %6s %6.1f%% %5d %10s" % (n, k, cm, am, cm / am, bytes_ms, fma_ms, bound,
                                                                              100.0 * max(bytes_ms, fma_ms) / cm, path.value, host_ms))
        if n == 8192 and k == 3:
            target = (cm, am, min(conv_ms), max(conv_ms), min(add_ms), max(add_ms))
        dw.free()
    for d in (da, db2, do):
        d.free()
if target:
    cm, am = target[0], target[1]
    say()
    say("target: 3 x 3 on 8192^2 takes %.4f ms (rounds %.4f .. %.4f), a + b on the same shape %.4f ms (%.4f .. %.4f): ratio %.3f — %s"
        % (cm, target[2], target[3], am, target[4], target[5], cm / am, "met (no longer than a + b)" if cm <= am else "MISSED"))
if not args.profile:
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
