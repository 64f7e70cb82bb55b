"""The headline's 16 independent 4096^3 products per step with every launch on the library stream (np_sgemm_set_variant(-27))
against alternating with the runtime's side lane (-28, the default): one process, one device, the two variants taking turns.
2 s of back-to-back launches first (the matrix clock ramps over the first ~50 ms of matrix work and the box should be warm),
then ROUNDS rounds of: 20 steps of 16 products over 4 operand sets (bench.py's bench_matmul) per variant, timed by one event
pair.  Prints every round, then median / min / max per variant and where the launches went.
Usage: python tools/gemm_overlap_ab.py [rounds, default 7]"""
import ctypes as C
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
from numpower_amd import device as D, synth
from numpower_amd._lib import Timer, check, load

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS, PRODUCTS, SETS, N = 20, 16, 4, 4096

D.init(0)
lib = load()
A = D.DeviceArray.from_host(synth.uniform((N, N), 3, -1.0, 1.0))
B = D.DeviceArray.from_host(synth.uniform((N, N), 4, -1.0, 1.0))
sets = [(A, B, D.DeviceArray((N, N)))]
for i in range(1, SETS):
    scale = D.DeviceArray.from_host(np.float32([2.0 ** -i]))
    Ai = D.binary("multiply", A, "full", scale, "scalar", 1, N * N, out=D.DeviceArray((N, N)))
    Bi = D.DeviceArray((N, N))
    check(lib.np_memcpy_d2d(Bi.ptr, B.ptr, 4 * N * N))
    sets.append((Ai, Bi, D.DeviceArray((N, N))))
D.sync()


def stats():
    out = (C.c_ulonglong * 3)()
    check(lib.np_sgemm_overlap_stats(out))
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
ms = {"off": [], "on": []}
went = {}
for rnd in range(ROUNDS):
    for name, code in (("off", -27), ("on", -28)) if rnd % 2 == 0 else (("on", -28), ("off", -27)):
        check(lib.np_sgemm_set_variant(code))
        step()
        D.sync()
        before = stats()
        t.start()
        for _ in range(STEPS):
            step()
        t.stop()
        ms[name].append(t.elapsed_ms() / STEPS)
        went[name] = [x - y for x, y in zip(stats(), before)]
    print("round %d: off %.4f ms/step, on %.4f ms/step, on / off %.4f" % (rnd, ms["off"][-1], ms["on"][-1], ms["on"][-1] / ms["off"][-1]), flush=True)
check(lib.np_sgemm_set_variant(-28))
flop = 2.0 * N ** 3 * PRODUCTS
for name in ("off", "on"):
    v = sorted(ms[name])
    med = float(np.median(v))
    print("%-3s median %.4f ms/step (%.1f TFLOP/s)  min %.4f  max %.4f   launches per round: side %d, next to the lane %d, joined %d"
          % (name, med, flop / med / 1e9, v[0], v[-1], *went[name]))
print("median on / off = %.4f" % (float(np.median(ms["on"])) / float(np.median(ms["off"]))))
# the outputs of the last round (overlap off or on, whichever came last) against linearity: C_i = C_0 * 2^-i bit for bit
C0 = sets[0][2].to_host()
print("linearity bit-exact:", all(bool((sets[i][2].to_host().view(np.uint32) == (C0 * np.float32(2.0 ** -i)).view(np.uint32)).all()) for i in range(1, SETS)))
