"""The two K loops of the 256 x 128 LDS-DMA kernels against each other: flat per-lane source pointers (np_sgemm_set_variant(-31))
and buffer-addressed sources with three K-tiles per trip (-32), one process, one device, the two taking turns.
2 s of back-to-back launches first (clock ramp, warm box), then ROUNDS rounds of: 20 steps of 16 products over 4 operand sets
(bench.py's bench_matmul) per loop, in 5 blocks of 4 steps with an event pair each.  Prints every round (median and range of its
blocks per loop, and whether the gain exceeds the flat loop's range in that round), then median / min / max per loop, which loop
the launches ran (np_sgemm_debug_kloop_stats) and whether both loops leave the same bits.
Usage: python tools/gemm_kloop_ab.py [rounds, default 7] [M N K, default 4096 4096 4096] [lane: -28 on (default) | -27 off]"""
import ctypes as C
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
from numpower_amd import device as D, synth
from numpower_amd._lib import Timer, check, load

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
M, N, K = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (4096, 4096, 4096)
LANE = int(sys.argv[5]) if len(sys.argv) > 5 else -28
STEPS, PRODUCTS, SETS = 20, 16, 4
OLD, NEW = -31, -32

D.init(0)
lib = load()
check(lib.np_sgemm_set_variant(LANE))
A = D.DeviceArray.from_host(synth.uniform((M, K), 3, -1.0, 1.0))
B = D.DeviceArray.from_host(synth.uniform((K, N), 4, -1.0, 1.0))
sets = [(A, B, D.DeviceArray((M, N)))]
for i in range(1, SETS):
    scale = D.DeviceArray.from_host(np.float32([2.0 ** -i]))
    Ai = D.binary("multiply", A, "full", scale, "scalar", 1, M * K, out=D.DeviceArray((M, K)))
    Bi = D.DeviceArray((K, N))
    check(lib.np_memcpy_d2d(Bi.ptr, B.ptr, 4 * K * N))
    sets.append((Ai, Bi, D.DeviceArray((M, N))))
D.sync()


def stats():
    out = (C.c_ulonglong * 2)()
    check(lib.np_sgemm_debug_kloop_stats(out))
    return list(out)


def step():
    for j in range(PRODUCTS):
        a, b, c = sets[j % SETS]
        D.sgemm(a, b, out=c)


t0 = time.perf_counter()
while time.perf_counter() - t0 < 2.0:
    step()
    D.sync()
t = Timer()
BLOCKS = 5                      # a loop's turn in a round: 5 blocks of STEPS / 5 steps, each timed by one event pair
ms = {"flat": [], "buffer": []}   # per round: the median of the blocks
rng = {"flat": [], "buffer": []}  # per round: max - min of the blocks
went, bits = {}, {}
for rnd in range(ROUNDS):
    for name, code in (("flat", OLD), ("buffer", NEW)) if rnd % 2 == 0 else (("buffer", NEW), ("flat", OLD)):
        check(lib.np_sgemm_set_variant(code))
        step()
        D.sync()
        before = stats()
        blocks = []
        for _ in range(BLOCKS):
            t.start()
            for _ in range(STEPS // BLOCKS):
                step()
            t.stop()
            blocks.append(t.elapsed_ms() / (STEPS // BLOCKS))
        ms[name].append(float(np.median(blocks)))
        rng[name].append(max(blocks) - min(blocks))
        went[name] = [x - y for x, y in zip(stats(), before)]
        bits[name] = sets[0][2].to_host().view(np.uint32)
    gain = ms["flat"][-1] - ms["buffer"][-1]
    print("round %d: flat %.4f ms/step (range %.4f), buffer %.4f ms/step (range %.4f), buffer / flat %.4f, gain %.4f ms %s the flat loop's range"
          % (rnd, ms["flat"][-1], rng["flat"][-1], ms["buffer"][-1], rng["buffer"][-1], ms["buffer"][-1] / ms["flat"][-1], gain,
             "ABOVE" if gain > rng["flat"][-1] else "inside"), flush=True)
check(lib.np_sgemm_set_variant(-28))
flop = 2.0 * M * N * K * PRODUCTS
for name in ("flat", "buffer"):
    v = sorted(ms[name])
    med = float(np.median(v))
    print("%-6s median %.4f ms/step (%.1f TFLOP/s)  min %.4f  max %.4f   launches per round: buffer loop %d, flat loop %d"
          % (name, med, flop / med / 1e9, v[0], v[-1], *went[name]))
print("%d x %d x %d, lane %d: median buffer / flat = %.4f; rounds where the gain exceeds the flat loop's range in that round: %d of %d"
      % (M, N, K, LANE, float(np.median(ms["buffer"])) / float(np.median(ms["flat"])),
         sum(f - b > r for f, b, r in zip(ms["flat"], ms["buffer"], rng["flat"])), ROUNDS))
print("same bits from both loops:", bool((bits["flat"] == bits["buffer"]).all()))
