"""Timing of the device convolution layer (np_dnn.hip): np_conv2d_forward, np_conv2d_backward_data and np_conv2d_backward_filter
on a short list of layers, after a GEMM warm-up that covers the clock ramp.  Writes profiles/dnn/conv2d_sweep.log (and prints it).

Per layer and operation: ms per call (device events around `reps` calls, the median of the rounds), TFLOP/s (2 M N K of the
implicit GEMM: forward F x N.P x C.kh.kw, dX C x N.H.W x F.kh.kw, dW F x C.kh.kw x N.P), and np_sgemm on DENSE operands of the same
(M, N, K) in the same run with the ratio gemm / conv: the ceiling the project's own GEMM sets for those extents.  The 1 x 1 layer
is a GEMM with no gather: a ratio far below 1 THERE is a tile-loop problem, not a gather problem.

Layers with a stride or a dilation (a fifth entry (sh, sw, dh, dw)) go through the _ex entry points; the others through the
calls they always went through.  Their TFLOP/s count the USEFUL 2 M N K: dX of a strided layer is counted as C x N.P x F.kh.kw,
the multiply-adds that meet a gradient, while the dilated-input kernel computes C x N.H.W x F.kh.kw, about sh.sw times as many,
over stored zeros; the last column is the form of the gather (np_debug_dnn_last_form).

Every layer runs in a child process of its own under its own time limit (--limit seconds); the sweep stops at the first
layer that fails or runs out of time.  --torch adds, as information, torch.nn.functional.conv2d and its autograd on the device
where this installation runs them (one more child); if it does not, the log says so in one line.

--act is the leg of the layer's bias and activation (np_conv2d_forward_act, np_conv2d_backward_act): per layer, in one child,
the plain forward pass, the fused one (a bias and relu) with the ratio fused / plain, and the plain pass plus ONE elementwise
pass over y (np_binary add of two arrays of numel(y): the cheapest unfused alternative if N-D broadcasting existed); then
np_conv2d_backward_act (relu, dz and db) against an elementwise multiply on arrays of the same element count (both move
12 B / element: two reads and a write), with the ratio and the fraction of 8 TB/s; and the same pair at one large case of about
10^8 elements.  Writes profiles/dnn/conv2d_act_sweep.log.
--forward-only times the forward pass alone, one line per layer: for alternating two builds of the library in one session.
--pool is the leg of the pooling layers (np_pool.hip: np_pool2d_forward, np_pool2d_backward), which are streaming kernels: per
layer (POOL_LAYERS) and mode, in one child, the forward pass (y alone), for max the forward pass that also writes idx, the gather
of the backward pass, and for max the backward pass as the glue runs it (the forward pass again into scratch, then the gather).
Each operation alternates, round by round in one session, with the library's float4 device copy (np_memcpy_d2d) moving the SAME
number of bytes, read plus written: 4 (numel(x) + numel(y)), plus 4 numel(y) where an idx is written or read.  Reported: ms, achieved
TB/s and the ratio copy / pool (1.00 = the copy's rate, the platform ceiling for streaming kernels), medians of the rounds.  The
operand sets are rotated (--sets) so that together they pass the 256 MiB Infinity Cache.  Writes profiles/dnn/pool2d_sweep.log.
--softmax is the leg of softmax, log-softmax, their backward passes and the cross-entropy with its gradient (np_softmax.hip), on
shapes that reach every kernel form (SOFTMAX_SHAPES).  Each operation alternates, round by round in one session, with the float4
copy of the SAME bytes (8 per element forward, 12 backward, 8 plus the labels and the losses for the cross-entropy) and, for the row
shapes, with the four-pass composition examples/softmax_regression.py uses (max, two fused chains, the loss chain), which is how the
library computed a softmax loss before.  Reported: ms, TB/s, copy / op (1.00 = the copy's rate, the ceiling of a form that reads a row
once and writes it once) and composition / op.  The log is stamped with the sources it ran on.  Writes profiles/dnn/softmax_sweep.log.
--optim is the leg of the optimizer steps (np_optim.hip), four cases (OPTIM_CASES).  0 and 1: plain SGD, momentum SGD and AdamW (12, 20
and 28 bytes per element) on one tensor of 10^8 elements and on a ResNet-like list of 301 tensors with the same total, each alternating
round by round with np_memcpy_d2d (the float4 copy) of the same bytes and with np_binary add over the same bytes; reported: ms, TB/s,
copy / step, copy / add, and the spread of both over the rounds.  2: the wall time of one step for 300 tensors of 1000 elements,
np_sgd_step and np_adam_step through the C ABI and through NDArray, against the per-tensor `p - g * lr` loop and against the Adam
composition from NDArray calls.  3: np_grad_norm on the two lists against np_reduce_all (sum) over the same bytes.  Writes
profiles/dnn/optim_sweep.log.

--batchnorm is the leg of batch normalization (np_batchnorm.hip): training forward, inference forward and backward on BATCHNORM_SHAPES,
which reach every kernel form.  Each operation alternates, round by round in one session, with the float4 copy of the bytes its form
moves (8 per element for inference and the one-launch training form, 12 for the split and rows training forward, 12 for the
one-launch backward, 20 for the split and rows backward) and, for the (N, C) shapes, the training forward with the composition a user
would write from NDArray calls (two column means, a centred square, three row broadcasts); an NCHW composition needs transposes and
is not expressed.  Reported: ms, TB/s, copy / op and composition / op.  Writes profiles/dnn/batchnorm_sweep.log.
--groupnorm is the leg of layer and group normalization (np_groupnorm.hip): forward, backward with the parameter gradients and
backward without them on GROUPNORM_SHAPES.  Each operation alternates, round by round in one session, with the float4 copy of the
bytes its form moves (forward 8 per element with the row in registers, 12 split; backward 12 or 20, and 8 more for the parameter
reduction) and, for the two 2-D shapes where it can be written, the forward pass with the composition from NDArray calls and with
np_batchnorm_forward's rows form on the same array.  Reported: ms, TB/s, copy / op, composition / op and batch norm / op.  Writes
profiles/dnn/groupnorm_sweep.log.
--attention is the leg of scaled dot-product attention (np_attention.hip): forward, backward and backward with dq alone on
ATTENTION_SHAPES, causal and not.  Reported: ms, the useful TFLOP/s (4.BH.Sq.Sk.D forward, 10.BH.Sq.Sk.D backward, halved under causal)
and its fraction of the 157.3 TFLOP/s fp32 matrix peak; for the forward pass without causal also the ratio to the composition from
NDArray calls (batched_matmul on a transposed k, a multiply, softmax, batched_matmul) and to np_sgemm_strided_batched on the two
products alone, alternating round by round in one session.  Writes profiles/dnn/attention_sweep.log.
--linear is the leg of the dense layer (np_linear.hip) on LINEAR_SHAPES (M, K, N), from below the examples' sizes to 4096^3.  Per shape,
in one child: each of the three products (y = x . w^T, dx = dz . w, dw = dz^T . x) with the tile form forced and with the library form
forced (np_debug_linear_force_form), alternating round by round, and bare np_sgemm on dense, already transposed operands of the same
extents as information, with ms, TFLOP/s, the fraction of the 157.3 TFLOP/s fp32 matrix peak, TM and S, which form is faster and which
form the unforced call takes: the dispatcher's constants (the work M.K.N from which a product takes the library form) are set where
the faster form changes in this table; then the whole layer, unforced, with a bias and tanh, forward and backward
(y, dz, dx, dw, db), against the composition from NDArray calls the examples used (transposes, bare products, a broadcast add, the
activation, its gradient, a column sum) and against the 1 x 1 convolution route (np_conv2d_forward_act, np_conv2d_backward_act,
np_conv2d_backward_filter, np_conv2d_backward_data); then the dz / db kernel alone against the float4 copy of its 12 bytes per element.
A shape where the layer is slower than the composition by more than the composition's own spread is marked FINDING.  Writes
profiles/dnn/linear_sweep.log.

Usage: python tools/dnn_sweep.py [--layers 0,1,...] [--rounds N] [--limit S] [--torch] [--out FILE]
       python tools/dnn_sweep.py --act [--layers ...]         the bias / activation leg
       python tools/dnn_sweep.py --forward-only [--layers ...]
       python tools/dnn_sweep.py --pool [--layers ...]        the pooling leg
       python tools/dnn_sweep.py --softmax [--layers ...]     the softmax / cross-entropy leg
       python tools/dnn_sweep.py --batchnorm [--layers ...]   the batch-normalization leg
       python tools/dnn_sweep.py --groupnorm [--layers ...]   the layer / group normalization leg
       python tools/dnn_sweep.py --attention [--layers ...]   the attention leg
       python tools/dnn_sweep.py --optim [--layers ...]       the optimizer leg
       python tools/dnn_sweep.py --linear [--layers ...]      the dense-layer leg
       python tools/dnn_sweep.py --profile LAYER     three calls of each operation and nothing else, for a run under the kernel profiler"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# name, (N, C, H, W), (F, kh, kw), (ph, pw)
LAYERS = [("3x3 64->64 at 56^2, batch 32", (32, 64, 56, 56), (64, 3, 3), (1, 1)),
          ("3x3 128->128 at 28^2, batch 32", (32, 128, 28, 28), (128, 3, 3), (1, 1)),
          ("1x1 256->64 at 56^2, batch 32", (32, 256, 56, 56), (64, 1, 1), (0, 0)),
          ("7x7 3->64 at 224^2 pad 3, batch 8", (8, 3, 224, 224), (64, 7, 7), (3, 3)),
          ("5x5 1->32 at 28^2, batch 512", (512, 1, 28, 28), (32, 5, 5), (0, 0)),
          # name, (N, C, H, W), (F, kh, kw), (ph, pw), (sh, sw, dh, dw)
          ("3x3/2 64->128 at 56^2 pad 1, batch 32", (32, 64, 56, 56), (128, 3, 3), (1, 1), (2, 2, 1, 1)),
          ("7x7/2 3->64 at 224^2 pad 3, batch 8", (8, 3, 224, 224), (64, 7, 7), (3, 3), (2, 2, 1, 1)),
          ("1x1/2 256->512 at 56^2, batch 32", (32, 256, 56, 56), (512, 1, 1), (0, 0), (2, 2, 1, 1)),
          ("3x3 dil 2 128->128 at 28^2 pad 2, batch 32", (32, 128, 28, 28), (128, 3, 3), (2, 2), (1, 1, 2, 2))]

# name, (N, C, H, W), (kh, kw), (sh, sw), (ph, pw), modes
POOL_LAYERS = [("2x2/2 64 ch at 112^2, batch 32", (32, 64, 112, 112), (2, 2), (2, 2), (0, 0), ("max", "avg")),
               ("3x3/2 pad 1 64 ch at 112^2, batch 32", (32, 64, 112, 112), (3, 3), (2, 2), (1, 1), ("max", "avg")),
               ("2x2/2 256 ch at 56^2, batch 32", (32, 256, 56, 56), (2, 2), (2, 2), (0, 0), ("max", "avg")),
               ("3x3/2 pad 1 256 ch at 56^2, batch 32", (32, 256, 56, 56), (3, 3), (2, 2), (1, 1), ("max", "avg")),
               ("7x7 global average 2048 ch at 7^2, batch 256", (256, 2048, 7, 7), (7, 7), (7, 7), (0, 0), ("avg",)),
               ("3x3/1 pad 1 256 ch at 28^2, batch 32", (32, 256, 28, 28), (3, 3), (1, 1), (1, 1), ("max", "avg"))]
POOL_MODE = {"max": 0, "avg": 1, "avg_valid": 2}

# name, (outer, cols, inner)
SOFTMAX_SHAPES = [("10^7 x 10", (10 ** 7, 10, 1)), ("200000 x 10", (200000, 10, 1)), ("65536 x 1000", (65536, 1000, 1)),
                  ("8192 x 32768", (8192, 32768, 1)), ("64 x 10^6", (64, 10 ** 6, 1)), ("NCHW channels (64, 21, 128, 128)", (64, 21, 128 * 128))]

# name, (N, C, inner)
BATCHNORM_SHAPES = [("(64, 64, 112, 112)", (64, 64, 112 * 112)), ("(64, 3, 224, 224)", (64, 3, 224 * 224)), ("(256, 512, 7, 7)", (256, 512, 49)),
                    ("(65536, 1024)", (65536, 1024, 1)), ("(10^6, 16)", (10 ** 6, 16, 1)), ("(64, 2048, 7, 7)", (64, 2048, 49)),
                    ("(32, 512, 14, 14)", (32, 512, 196))]

# name, (N, G, D, inner), compare with the composition and batch norm's rows form
GROUPNORM_SHAPES = [("layer (65536, 1024)", (65536, 1, 1024, 1), True), ("layer (10^6, 16)", (10 ** 6, 1, 16, 1), True),
                    ("layer (8192, 8192)", (8192, 1, 8192, 1), False), ("layer (64, 10^6)", (64, 1, 10 ** 6, 1), False),
                    ("group 32 (64, 64, 112, 112)", (64, 32, 2, 112 * 112), False), ("group 32 (256, 512, 7, 7)", (256, 32, 16, 49), False),
                    ("group 32 (2, 64, 112, 112)", (2, 32, 2, 112 * 112), False), ("instance (64, 64, 56, 56)", (64, 64, 1, 56 * 56), False)]

# (BH, S, D): Sq = Sk = S
ATTENTION_SHAPES = [(64, 512, 64), (64, 2048, 64), (16, 8192, 64), (64, 2048, 128), (512, 197, 64), (64, 2048, 32)]
MATRIX_PEAK_TFLOPS = 157.3

LINEAR_SHAPES = [(32, 32, 32), (64, 64, 32), (128, 64, 64), (128, 128, 64), (128, 256, 128), (256, 128, 128), (256, 256, 256), (4096, 64, 10), (16, 1024, 1024),
                 (512, 784, 256), (1024, 1024, 1024), (4096, 1024, 1024), (8192, 4096, 1024), (128, 4096, 4096), (4096, 4096, 4096)]      # (M, K, N)
OPTIM_CASES = ["one tensor of 10^8", "ResNet-like list of 301 tensors, 10^8 in all", "300 tensors of 1000: wall time of a step", "np_grad_norm"]
OPTIM_TOTAL = 10 ** 8


def optim_resnet_like():
    """100 3x3 convolutions over 64 .. 512 channels, each with a gamma and a beta, and one dense layer that brings the total to 10^8"""
    counts = []
    for j in range(100):
        c = (64, 128, 256, 512)[j % 4]
        counts += [c * c * 9, c, c]
    return counts + [OPTIM_TOTAL - sum(counts)]


ap = argparse.ArgumentParser()
ap.add_argument("--batchnorm", action="store_true")
ap.add_argument("--optim", action="store_true")
ap.add_argument("--linear", action="store_true")
ap.add_argument("--groupnorm", action="store_true")
ap.add_argument("--attention", action="store_true")
ap.add_argument("--pool", action="store_true")
ap.add_argument("--softmax", action="store_true")
ap.add_argument("--sets", type=int, default=0, help="--pool: operand sets to rotate through (0: enough to pass 256 MiB)")
ap.add_argument("--layers", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=120, help="seconds each child process may take")
ap.add_argument("--torch", action="store_true")
ap.add_argument("--act", action="store_true")
ap.add_argument("--forward-only", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--profile", type=int, default=None)
ap.add_argument("--child", default=None, help="internal: 'layer:<i>' or 'torch'")
args = ap.parse_args()
if args.layers is None:
    args.layers = ",".join(str(i) for i in range(len(LINEAR_SHAPES if args.linear else OPTIM_CASES if args.optim else ATTENTION_SHAPES if args.attention else GROUPNORM_SHAPES if args.groupnorm else BATCHNORM_SHAPES if args.batchnorm else SOFTMAX_SHAPES if args.softmax else POOL_LAYERS if args.pool else LAYERS)))
if args.out is None:
    args.out = str(ROOT / "profiles" / "dnn" / ("linear_sweep.log" if args.linear else "optim_sweep.log" if args.optim else "attention_sweep.log" if args.attention else "groupnorm_sweep.log" if args.groupnorm else "batchnorm_sweep.log" if args.batchnorm else "softmax_sweep.log" if args.softmax else "pool2d_sweep.log" if args.pool else "conv2d_act_sweep.log" if args.act else
                                               "conv2d_forward_only.log" if args.forward_only else "conv2d_sweep.log"))
LARGE = (256, 128, 3136)                        # (N, F, P) of the large case of --act: 1.03e8 elements
HBM_TBS = 8.0


def shapes(i):
    _, (N, C, H, W), (F, kh, kw), (ph, pw) = LAYERS[i][:4]
    sh, sw, dh, dw = geometry(i)
    oh, ow = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    useful_dx = N * H * W if (sh, sw) == (1, 1) else N * oh * ow      # the pixels whose products meet a gradient
    gemms = {"forward": (F, N * oh * ow, C * kh * kw), "dX": (C, useful_dx, F * kh * kw), "dW": (F, C * kh * kw, N * oh * ow)}
    return (N, C, H, W), (F, C, kh, kw), (N, F, oh, ow), (ph, pw), gemms


def geometry(i):
    return LAYERS[i][4] if len(LAYERS[i]) > 4 else (1, 1, 1, 1)


def run_layer(i, rounds, profile=False):
    import ctypes as C_
    import numpy as np
    from numpower_amd import device as D
    from numpower_amd._lib import Timer, check, load
    D.init(0)
    lib = load()
    t = Timer()
    xs, ws, ys, (ph, pw), gemms = shapes(i)
    rng = np.random.default_rng(i)
    dev = lambda s: D.DeviceArray.from_host(rng.standard_normal(s).astype(np.float32))
    x, w, dy = dev(xs), dev(ws), dev(ys)
    y, dx, dw = D.DeviceArray(ys), D.DeviceArray(xs), D.DeviceArray(ws)
    dims = (xs[0], xs[1], xs[2], xs[3], ws[0], ws[2], ws[3], ph, pw)
    ops = {"forward": lambda: check(lib.np_conv2d_forward(x.ptr, w.ptr, *dims, y.ptr)),
           "dX": lambda: check(lib.np_conv2d_backward_data(dy.ptr, w.ptr, *dims, dx.ptr)),
           "dW": lambda: check(lib.np_conv2d_backward_filter(x.ptr, dy.ptr, *dims, dw.ptr))}
    if len(LAYERS[i]) > 4:
        dims += geometry(i)
        ops = {"forward": lambda: check(lib.np_conv2d_forward_ex(x.ptr, w.ptr, *dims, y.ptr)),
               "dX": lambda: check(lib.np_conv2d_backward_data_ex(dy.ptr, w.ptr, *dims, dx.ptr)),
               "dW": lambda: check(lib.np_conv2d_backward_filter_ex(x.ptr, dy.ptr, *dims, dw.ptr))}
    if profile:
        for _ in range(3):
            for fn in ops.values():
                fn()
        D.sync()
        return
    ga = dev((4096, 4096))                      # clock ramp: ~1 s of 4096^3 GEMMs
    gc = D.DeviceArray((4096, 4096))
    t0 = time.time()
    while time.time() - t0 < 1.0:
        for _ in range(10):
            check(lib.np_sgemm(4096, 4096, 4096, ga.ptr, ga.ptr, gc.ptr))
        D.sync()

    def median_ms(fn):
        fn()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(3, min(200, int(0.1 / max(time.time() - t0, 1e-5))))
        ms = []
        for _ in range(rounds):
            t.start()
            for _ in range(reps):
                fn()
            t.stop()
            ms.append(t.elapsed_ms() / reps)
        return statistics.median(ms)

    for name, fn in ops.items():
        M, N, K = gemms[name]
        a, b, c = dev((M, K)), dev((K, N)), D.DeviceArray((M, N))
        conv_ms = median_ms(fn)
        tm, s, form = C_.c_int(), C_.c_int(), C_.c_int()
        check(lib.np_debug_dnn_last_path(C_.byref(tm), C_.byref(s)))
        check(lib.np_debug_dnn_last_form(C_.byref(form)))
        gemm_ms = median_ms(lambda: check(lib.np_sgemm(M, N, K, a.ptr, b.ptr, c.ptr)))
        flop = 2.0 * M * N * K
        print("%-42s %-8s %6d %9d %7d %9.4f %8.2f %9.4f %8.2f %7.3f %4d %4d %4d" % (LAYERS[i][0], name, M, N, K, conv_ms, flop / conv_ms * 1e-9, gemm_ms,
                                                                                flop / gemm_ms * 1e-9, gemm_ms / conv_ms, tm.value, s.value, form.value),
              flush=True)
        for d in (a, b, c):
            d.free()


def _setup():
    from numpower_amd import device as D
    from numpower_amd._lib import Timer, check, load
    D.init(0)
    lib = load()
    t = Timer()

    def ramp():                                 # clock ramp: ~1 s of 4096^3 GEMMs
        import numpy as np
        ga = D.DeviceArray.from_host(np.random.default_rng(0).standard_normal((4096, 4096)).astype(np.float32))
        gc = D.DeviceArray((4096, 4096))
        t0 = time.time()
        while time.time() - t0 < 1.0:
            for _ in range(10):
                check(lib.np_sgemm(4096, 4096, 4096, ga.ptr, ga.ptr, gc.ptr))
            D.sync()
        ga.free()
        gc.free()

    def median_ms(fn, rounds):
        fn()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(3, min(200, int(0.1 / max(time.time() - t0, 1e-5))))
        ms = []
        for _ in range(rounds):
            t.start()
            for _ in range(reps):
                fn()
            t.stop()
            ms.append(t.elapsed_ms() / reps)
        return statistics.median(ms)

    return D, lib, check, ramp, median_ms


def _forward_call(lib, check, i, x, w, y, bias=None, act=0, fused=False):
    xs, ws, ys, (ph, pw), _ = shapes(i)
    dims = (xs[0], xs[1], xs[2], xs[3], ws[0], ws[2], ws[3], ph, pw)
    if fused:
        return lambda: check(lib.np_conv2d_forward_act(x.ptr, w.ptr, bias.ptr if bias is not None else None, *dims, *geometry(i), act, y.ptr))
    if len(LAYERS[i]) > 4:
        return lambda: check(lib.np_conv2d_forward_ex(x.ptr, w.ptr, *dims, *geometry(i), y.ptr))
    return lambda: check(lib.np_conv2d_forward(x.ptr, w.ptr, *dims, y.ptr))


def run_forward_only(i, rounds):
    import numpy as np
    D, lib, check, ramp, median_ms = _setup()
    xs, ws, ys, _, _ = shapes(i)
    rng = np.random.default_rng(i)
    dev = lambda s: D.DeviceArray.from_host(rng.standard_normal(s).astype(np.float32))
    x, w, y = dev(xs), dev(ws), D.DeviceArray(ys)
    ramp()
    print("%-42s forward %9.4f" % (LAYERS[i][0], median_ms(_forward_call(lib, check, i, x, w, y), rounds)), flush=True)


def _backward_pair(D, lib, check, median_ms, rounds, name, N, F, P):
    """np_conv2d_backward_act (relu, dz and db) against np_binary multiply on the same element count"""
    import ctypes as C_
    import numpy as np
    rng = np.random.default_rng(F)
    dev = lambda s: D.DeviceArray.from_host(rng.standard_normal(s).astype(np.float32))
    n = N * F * P
    y, dy, dz, db = dev((n,)), dev((n,)), D.DeviceArray((n,)), D.DeviceArray((F,))
    act_ms = median_ms(lambda: check(lib.np_conv2d_backward_act(y.ptr, dy.ptr, N, F, P, 1, dz.ptr, db.ptr)), rounds)
    s = [C_.c_int() for _ in range(3)]
    check(lib.np_debug_dnn_last_epilogue(*(C_.byref(c) for c in s)))
    mul_ms = median_ms(lambda: check(lib.np_binary(2, y.ptr, 0, dy.ptr, 0, dz.ptr, 1, n, 0, 0)), rounds)
    tbs = lambda ms: 12.0 * n / ms * 1e-9
    print("%-42s backward_act (N %d, F %d, P %d, S %d) %9.4f ms %5.2f TB/s (%4.1f %% of %g)   multiply %9.4f ms %5.2f TB/s   act / multiply %6.3f"
          % (name, N, F, P, s[2].value, act_ms, tbs(act_ms), 100 * tbs(act_ms) / HBM_TBS, HBM_TBS, mul_ms, tbs(mul_ms), act_ms / mul_ms), flush=True)
    for d in (y, dy, dz, db):
        d.free()


def run_act(what, rounds):
    import numpy as np
    D, lib, check, ramp, median_ms = _setup()
    ramp()
    if what == "large":
        _backward_pair(D, lib, check, median_ms, rounds, "large", *LARGE)
        return
    i = int(what)
    xs, ws, ys, _, _ = shapes(i)
    rng = np.random.default_rng(i)
    dev = lambda s: D.DeviceArray.from_host(rng.standard_normal(s).astype(np.float32))
    x, w, bias, y, other, out = dev(xs), dev(ws), dev((ws[0],)), D.DeviceArray(ys), dev(ys), D.DeviceArray(ys)
    n = int(np.prod(ys))
    plain = _forward_call(lib, check, i, x, w, y)
    plain_ms = median_ms(plain, rounds)
    fused_ms = median_ms(_forward_call(lib, check, i, x, w, y, bias, 1, fused=True), rounds)

    def unfused():
        plain()
        check(lib.np_binary(0, y.ptr, 0, other.ptr, 0, out.ptr, 1, n, 0, 0))

    unfused_ms = median_ms(unfused, rounds)
    print("%-42s forward plain %9.4f ms   bias + relu fused %9.4f ms   fused / plain %6.3f   plain + one elementwise pass %9.4f ms   fused / that %6.3f"
          % (LAYERS[i][0], plain_ms, fused_ms, fused_ms / plain_ms, unfused_ms, fused_ms / unfused_ms), flush=True)
    _backward_pair(D, lib, check, median_ms, rounds, LAYERS[i][0], ys[0], ys[1], ys[2] * ys[3])


def run_pool(i, rounds, sets):
    """one pooling layer: every operation alternates with a float4 copy of the same bytes, round by round"""
    import ctypes as C_
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    t = Timer()
    name, (N, Cc, H, W), (kh, kw), (sh, sw), (ph, pw), modes = POOL_LAYERS[i]
    planes, oh, ow = N * Cc, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    nx, ny = planes * H * W, planes * oh * ow
    if sets < 1:
        sets = max(2, -(-(256 << 20) // (4 * nx)) + 1)
    rng = np.random.default_rng(i)
    host_x, host_dy = rng.standard_normal(nx).astype(np.float32), rng.standard_normal(ny).astype(np.float32)
    xs = [D.DeviceArray.from_host(host_x) for _ in range(sets)]
    cs, cd = [D.DeviceArray((nx + 2 * ny,)) for _ in range(sets)], [D.DeviceArray((nx + 2 * ny,)) for _ in range(sets)]      # the copy's own operands
    for c in cs:
        check(lib.np_memset0(c.ptr, 4 * (nx + 2 * ny)))
    dxs = [D.DeviceArray((nx,)) for _ in range(sets)]
    dys = [D.DeviceArray.from_host(host_dy) for _ in range(sets)]
    ys, idxs, scratch = [D.DeviceArray((ny,)) for _ in range(sets)], [D.DeviceArray((ny,)) for _ in range(sets)], D.DeviceArray((2 * ny,))
    dims = (planes, H, W, kh, kw, ph, pw, sh, sw)
    ramp()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def copy_of(total_bytes):
        half = total_bytes // 2 // 16 * 16        # a copy of B / 2 bytes reads B / 2 and writes B / 2
        assert half <= 4 * (nx + 2 * ny)
        return rotating(lambda k: check(lib.np_memcpy_d2d(cd[k].ptr, cs[k].ptr, half)))

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    for mode in modes:
        m = POOL_MODE[mode]
        for k in range(sets):                     # every idx holds its plane's maxima before a gather reads it
            check(lib.np_pool2d_forward(xs[k].ptr, *dims, 0, ys[k].ptr, idxs[k].ptr))
        ops = [("forward", rotating(lambda k: check(lib.np_pool2d_forward(xs[k].ptr, *dims, m, ys[k].ptr, None))), 4 * (nx + ny))]
        if H * W <= 8192:                         # the staged form took it: the direct form on the same layer, through the A-B switch

            def forced_direct(k):
                check(lib.np_debug_pool_forward_form(1))
                try:
                    check(lib.np_pool2d_forward(xs[k].ptr, *dims, m, ys[k].ptr, None))
                finally:
                    check(lib.np_debug_pool_forward_form(0))

            ops.append(("forward, direct form forced", rotating(forced_direct), 4 * (nx + ny)))
        if mode == "max":
            ops.append(("forward + idx", rotating(lambda k: check(lib.np_pool2d_forward(xs[k].ptr, *dims, m, ys[k].ptr, idxs[k].ptr))), 4 * (nx + 2 * ny)))
            ops.append(("gather", rotating(lambda k: check(lib.np_pool2d_backward(dys[k].ptr, idxs[k].ptr, *dims, m, dxs[k].ptr))), 4 * (nx + 2 * ny)))

            def layer_backward(k):                # what NPH_Pool2D_Backward launches: y and idx again into scratch, then the gather
                check(lib.np_pool2d_forward(xs[k].ptr, *dims, m, scratch.ptr, scratch.ptr + 4 * ny))
                check(lib.np_pool2d_backward(dys[k].ptr, scratch.ptr + 4 * ny, *dims, m, dxs[k].ptr))

            ops.append(("backward (recomputed idx)", rotating(layer_backward), 4 * (nx + 2 * ny) + 4 * (nx + 2 * ny)))
        else:
            ops.append(("gather = backward", rotating(lambda k: check(lib.np_pool2d_backward(dys[k].ptr, None, *dims, m, dxs[k].ptr))), 4 * (nx + ny)))
        for label, fn, nbytes in ops:
            copy = copy_of(nbytes)
            for f in (fn, copy):                  # warm
                for _ in range(3):
                    f()
            D.sync()
            t0 = time.time()
            fn()
            D.sync()
            reps = max(5, min(200, int(0.05 / max(time.time() - t0, 1e-5))))
            pool_ms, copy_ms = [], []
            for _ in range(rounds):               # alternating in one session
                pool_ms.append(timed(fn, reps))
                copy_ms.append(timed(copy, reps))
            pm, cm = statistics.median(pool_ms), statistics.median(copy_ms)
            form = [C_.c_int(), C_.c_int()]
            check(lib.np_debug_pool_last_path(C_.byref(form[0]), C_.byref(form[1])))
            print("%-44s %-9s %-28s forms %d %d %7.1f MB %9.4f ms %5.2f TB/s   copy %9.4f ms %5.2f TB/s   copy / pool %5.2f   (min %5.2f max %5.2f)"
                  % (name, mode, label, form[0].value, form[1].value, nbytes * 1e-6, pm, nbytes / pm * 1e-9, cm, nbytes / cm * 1e-9, cm / pm,
                     min(c / p for c, p in zip(copy_ms, pool_ms)), max(c / p for c, p in zip(copy_ms, pool_ms))), flush=True)


def run_batchnorm(i, rounds, sets):
    """one shape: training forward, inference forward and backward, each alternating with a float4 copy of the bytes its form moves"""
    import ctypes as C_
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    t = Timer()
    name, (N, C, inner) = BATCHNORM_SHAPES[i]
    n = N * C * inner
    if sets < 1:
        sets = max(2, -(-(256 << 20) // (4 * n)) + 1)
    rng = np.random.default_rng(i)
    block = rng.standard_normal(1 << 20).astype(np.float32)
    host = np.resize(block, n)
    xs = [D.DeviceArray.from_host(host) for _ in range(sets)]
    ys, dys, dxs = ([D.DeviceArray((n,)) for _ in range(sets)] for _ in range(3))
    for d in dys:
        check(lib.np_memcpy_d2d(d.ptr, xs[0].ptr, 4 * n))
    words = 5 * n // 2 + 16
    cs, cd = [D.DeviceArray((words,)) for _ in range(sets)], [D.DeviceArray((words,)) for _ in range(sets)]      # the copy's own operands
    for c in cs:
        check(lib.np_memset0(c.ptr, 4 * words))
    gamma, beta = D.DeviceArray.from_host(rng.standard_normal(C).astype(np.float32)), D.DeviceArray.from_host(rng.standard_normal(C).astype(np.float32))
    rm, rv = D.DeviceArray.from_host(np.zeros(C, np.float32)), D.DeviceArray.from_host(np.ones(C, np.float32))
    mean, invstd, dgamma, dbeta = (D.DeviceArray((C,)) for _ in range(4))
    dims = (N, C, inner)
    ramp()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def copy_of(total_bytes):
        half = total_bytes // 2 // 16 * 16        # a copy of B / 2 bytes reads B / 2 and writes B / 2
        return rotating(lambda k: check(lib.np_memcpy_d2d(cd[k].ptr, cs[k].ptr, half)))

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    def probe():
        form, launches, slices = C_.c_int(), C_.c_int(), C_.c_size_t()
        check(lib.np_debug_batchnorm_last_path(C_.byref(form), C_.byref(launches), C_.byref(slices)))
        return form.value, launches.value, slices.value

    composition = None
    if inner == 1:                                # what a user writes today for an (N, C) array: single-axis means and row broadcasts
        from numpower_amd.ndarray import NDArray as nd
        gx = nd.array(host.reshape(N, C)).gpu()
        gg, gb = nd.array(np.ones(C, np.float32)).gpu(), nd.array(np.zeros(C, np.float32)).gpu()

        def composition():
            m = nd.mean(gx, 0)
            xc = gx - m
            inv = 1.0 / nd.sqrt(nd.mean(xc * xc, 0) + 1e-5)
            return xc * inv * gg + gb

    training = rotating(lambda k: check(lib.np_batchnorm_forward(xs[k].ptr, gamma.ptr, beta.ptr, *dims, 1, 0.1, 1e-5, rm.ptr, rv.ptr, ys[k].ptr, mean.ptr, invstd.ptr)))
    inference = rotating(lambda k: check(lib.np_batchnorm_forward(xs[k].ptr, gamma.ptr, beta.ptr, *dims, 0, 0.1, 1e-5, rm.ptr, rv.ptr, ys[k].ptr, None, None)))
    backward = rotating(lambda k: check(lib.np_batchnorm_backward(xs[k].ptr, dys[k].ptr, gamma.ptr, mean.ptr, invstd.ptr, *dims, dxs[k].ptr, dgamma.ptr, dbeta.ptr)))
    training()
    one = probe()[0] == 1
    ops = [("training forward", training, (8 if one else 12) * n, True), ("inference forward", inference, 8 * n, False),
           ("backward", backward, (12 if one else 20) * n, False)]
    for label, fn, nbytes, against in ops:
        copy = copy_of(nbytes)
        for f in (fn, copy):                      # warm
            for _ in range(3):
                f()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(5, min(200, int(0.05 / max(time.time() - t0, 1e-5))))
        op_ms, copy_ms, comp_ms = [], [], []
        for _ in range(rounds):                   # alternating in one session
            op_ms.append(timed(fn, reps))
            copy_ms.append(timed(copy, reps))
            if against and composition is not None:
                comp_ms.append(timed(composition, max(2, reps // 8)))
        fn()
        form, launches, slices = probe()
        om, cm = statistics.median(op_ms), statistics.median(copy_ms)
        tail = ""
        if comp_ms:
            pm = statistics.median(comp_ms)
            tail = "   composition %9.4f ms   composition / op %6.2f" % (pm, pm / om)
        print("%-20s %-18s form %d launches %d S %4d %8.1f MB %9.4f ms %5.2f TB/s   copy %9.4f ms %5.2f TB/s   copy / op %5.2f   (min %5.2f max %5.2f)%s"
              % (name, label, form, launches, slices, nbytes * 1e-6, om, nbytes / om * 1e-9, cm, nbytes / cm * 1e-9, cm / om,
                 min(c / p for c, p in zip(copy_ms, op_ms)), max(c / p for c, p in zip(copy_ms, op_ms)), tail), flush=True)


def run_optim(i, rounds):
    """one case of OPTIM_CASES"""
    import ctypes as C_
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import BINARY_OPS, REDUCE_OPS, Timer
    t = Timer()
    rng = np.random.default_rng(i)
    block = rng.standard_normal(1 << 20).astype(np.float32)
    vec = lambda values: (C_.c_void_p * len(values))(*values)

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    def reps_for(fn):
        for _ in range(3):
            fn()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        return max(5, min(200, int(0.05 / max(time.time() - t0, 1e-5))))

    def probe():
        launches, chunks, wide, scalar = C_.c_int(), C_.c_size_t(), C_.c_int(), C_.c_int()
        check(lib.np_debug_optim_last_path(C_.byref(launches), C_.byref(chunks), C_.byref(wide), C_.byref(scalar)))
        return launches.value, chunks.value, wide.value, scalar.value

    def carve(counts, value=None):
        """one allocation cut into the tensors of a list, each on a 16-byte boundary -> (the allocation, the pointers)"""
        starts, at = [], 0
        for n in counts:
            starts.append(at)
            at += -(-n // 4) * 4
        whole = D.DeviceArray.from_host(np.resize(block, at) if value is None else np.full(at, value, np.float32))
        return whole, vec([whole.ptr + 4 * s for s in starts])

    if i in (0, 1, 3):
        counts = [OPTIM_TOTAL] if i == 0 else optim_resnet_like()
        lists = [("one tensor of 10^8", [OPTIM_TOTAL]), ("list of 301, 10^8 in all", optim_resnet_like())] if i == 3 else [(OPTIM_CASES[i], counts)]
    if i in (0, 1):
        T, n = len(counts), sum(counts)
        sizes = (C_.c_size_t * T)(*counts)
        (hp, p), (hg, g), (hm, m), (hv, v) = carve(counts), carve(counts), carve(counts, 0.0), carve(counts, 0.0)
        words = 28 * n // 8 + 16
        cs, cd, third = D.DeviceArray((words,)), D.DeviceArray((words,)), D.DeviceArray((28 * n // 12 + 16,))
        check(lib.np_memset0(cs.ptr, 4 * words))
        check(lib.np_memset0(cd.ptr, 4 * words))
        ramp()
        steps = [("plain SGD", 12, lambda: check(lib.np_sgd_step(p, g, None, sizes, T, 1e-3, 0.0, 0.0, 0.0, 0, 0, None))),
                 ("momentum SGD", 20, lambda: check(lib.np_sgd_step(p, g, m, sizes, T, 1e-3, 0.9, 0.0, 0.0, 0, 0, None))),
                 ("AdamW", 28, lambda: check(lib.np_adam_step(p, g, m, v, sizes, T, 10, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, None)))]
        for label, per, fn in steps:
            nbytes = per * n
            half, n_add = nbytes // 2 // 16 * 16, nbytes // 12
            copy = lambda: check(lib.np_memcpy_d2d(cd.ptr, cs.ptr, half))
            add = lambda: check(lib.np_binary(BINARY_OPS["add"], cs.ptr, 0, cd.ptr, 0, third.ptr, 1, n_add, 0, 0))
            reps = reps_for(fn)
            for f in (copy, add):
                for _ in range(3):
                    f()
            step_ms, copy_ms, add_ms = [], [], []
            for _ in range(rounds):                   # alternating in one session
                step_ms.append(timed(fn, reps))
                copy_ms.append(timed(copy, reps))
                add_ms.append(timed(add, reps))
            fn()
            launches, chunks, wide, scalar = probe()
            sm, cm, am = statistics.median(step_ms), statistics.median(copy_ms), statistics.median(add_ms)
            ratios, add_ratios = [c / x for c, x in zip(copy_ms, step_ms)], [c / a for c, a in zip(copy_ms, add_ms)]
            print("%-44s %-13s launches %d chunks %6d vec %3d scalar %d %7.1f MB %8.4f ms %5.2f TB/s   copy %8.4f ms %5.2f TB/s   copy / step %5.3f (min %5.3f max %5.3f)"
                  "   add %8.4f ms   copy / add %5.3f (min %5.3f max %5.3f)"
                  % (OPTIM_CASES[i], label, launches, chunks, wide, scalar, nbytes * 1e-6, sm, nbytes / sm * 1e-9, cm, nbytes / cm * 1e-9, cm / sm, min(ratios),
                     max(ratios), am, cm / am, min(add_ratios), max(add_ratios)), flush=True)
    elif i == 2:
        from numpower_amd.ndarray import NDArray as nd
        T, each = 300, 1000
        counts = [each] * T
        sizes = (C_.c_size_t * T)(*counts)
        (hp, p), (hg, g), (hm, m), (hv, v) = carve(counts), carve(counts), carve(counts, 0.0), carve(counts, 0.0)
        host = lambda value=None: [nd.array(block[:each] if value is None else np.full(each, value, np.float32)).gpu() for _ in range(T)]
        P, G, M, V = host(), host(), host(0.0), host(0.0)
        state = {"P": P, "M": M, "V": V}
        lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
        bc2s, ss = float(np.sqrt(1.0 - b2 ** 10)), lr / (1.0 - b1 ** 10)

        def sgd_loop():
            state["P"] = [a - b * lr for a, b in zip(state["P"], G)]

        def adam_composition():
            state["M"] = [a * b1 + b * (1.0 - b1) for a, b in zip(state["M"], G)]
            state["V"] = [a * b2 + b * b * (1.0 - b2) for a, b in zip(state["V"], G)]
            state["P"] = [a - (b / (nd.sqrt(c) / bc2s + eps)) * ss for a, b, c in zip(state["P"], state["M"], state["V"])]

        ramp()
        cases = [("np_sgd_step, the C ABI", lambda: check(lib.np_sgd_step(p, g, None, sizes, T, lr, 0.0, 0.0, 0.0, 0, 0, None))),
                 ("NDArray.dnn_sgd_step", lambda: nd.dnn_sgd_step(P, G, lr)),
                 ("the loop p - g * lr", sgd_loop),
                 ("np_adam_step, the C ABI", lambda: check(lib.np_adam_step(p, g, m, v, sizes, T, 10, lr, b1, b2, eps, 0.0, 0, None))),
                 ("NDArray.dnn_adam_step", lambda: nd.dnn_adam_step(P, G, M, V, 10, lr, (b1, b2), eps)),
                 ("Adam from NDArray calls", adam_composition)]
        walls = {label: [] for label, _ in cases}
        for label, fn in cases:
            for _ in range(3):
                fn()
        D.sync()
        for _ in range(rounds):                       # alternating in one session; a host clock around work that ends in a synchronise
            for label, fn in cases:
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                D.sync()
                walls[label].append((time.perf_counter() - t0) / 10 * 1e6)
        base = {"sgd": statistics.median(walls["NDArray.dnn_sgd_step"]), "adam": statistics.median(walls["NDArray.dnn_adam_step"])}
        for label, _ in cases:
            med = statistics.median(walls[label])
            print("%-44s %-26s %9.1f us per step (min %9.1f max %9.1f)   over the NDArray method %6.1fx"
                  % (OPTIM_CASES[i], label, med, min(walls[label]), max(walls[label]), med / base["adam" if "dam" in label else "sgd"]), flush=True)
    else:
        ramp()
        for name, counts in lists:
            T, n = len(counts), sum(counts)
            sizes = (C_.c_size_t * T)(*counts)
            hg, g = carve(counts)
            flat = D.DeviceArray.from_host(np.resize(block, n))
            out = D.DeviceArray((2,))
            value = C_.c_float()
            norm = lambda: check(lib.np_grad_norm(g, sizes, T, 1.0, out.ptr))
            total = lambda: check(lib.np_reduce_all(REDUCE_OPS["sum"], flat.ptr, n, C_.byref(value)))
            reps = reps_for(norm)
            for _ in range(3):
                total()
            norm_ms, sum_ms = [], []
            for _ in range(rounds):
                norm_ms.append(timed(norm, reps))
                sum_ms.append(timed(total, reps))
            launches, chunks, _, _ = probe()
            nm, sm = statistics.median(norm_ms), statistics.median(sum_ms)
            ratios = [a / b for a, b in zip(sum_ms, norm_ms)]
            print("%-44s %-26s launches %d partials %6d %7.1f MB %8.4f ms %5.2f TB/s   np_reduce_all sum %8.4f ms %5.2f TB/s   sum / norm %5.3f (min %5.3f max %5.3f)"
                  % (OPTIM_CASES[i], name, launches, chunks, 4e-6 * n, nm, 4e-9 * n / nm * 1e3 * 1e-3, sm, 4e-9 * n / sm * 1e3 * 1e-3, sm / nm, min(ratios), max(ratios)), flush=True)
            hg.free()
            flat.free()


def run_linear(i, rounds):
    """one shape: the three products against bare np_sgemm, the whole layer against the NDArray composition and the 1 x 1 convolution
    route, the dz / db kernel against the float4 copy, alternating round by round in one session"""
    import ctypes as C
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    from numpower_amd.ndarray import NDArray as nd
    t = Timer()
    M, K, N = LINEAR_SHAPES[i]
    rng = np.random.default_rng(i)
    draw = lambda *shape: np.resize(rng.standard_normal(1 << 20).astype(np.float32), int(np.prod(shape))).reshape(shape)
    hx, hw, hb, hdy = draw(M, K), draw(N, K) * np.float32(1.0 / np.sqrt(K)), draw(N), draw(M, N)
    x, w, b, dy = (D.DeviceArray.from_host(h) for h in (hx, hw, hb, hdy))
    y, dz, dx, dw, db = D.DeviceArray((M, N)), D.DeviceArray((M, N)), D.DeviceArray((M, K)), D.DeviceArray((N, K)), D.DeviceArray((N,))
    wt = D.DeviceArray.from_host(np.ascontiguousarray(hw.T))       # dense operands of the bare products, made outside the timing
    dyt = D.DeviceArray.from_host(np.ascontiguousarray(hdy.T))
    c1, c2 = D.DeviceArray((3 * M * N // 2 + 4,)), D.DeviceArray((3 * M * N // 2 + 4,))
    gx, gw, gb, gdy = (nd.array(h).gpu() for h in (hx, hw, hb, hdy))
    TANH = 2
    chosen = C.c_int(0)

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    def probe(product):
        v = [C.c_int(0) for _ in range(4)]
        check(lib.np_debug_linear_last_path(product, *(C.byref(c) for c in v)))
        return v[1].value, v[2].value

    def against(fn, others, divide=4):
        """-> the rounds of fn and of every other, alternating"""
        for f in [fn] + others:
            for _ in range(2):
                f()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(3, min(100, int(0.05 / max(time.time() - t0, 1e-5))))
        op_ms, other_ms = [], [[] for _ in others]
        for _ in range(rounds):
            op_ms.append(timed(fn, reps))
            for f, ms in zip(others, other_ms):
                ms.append(timed(f, max(2, reps // divide)))
        return op_ms, other_ms

    fwd_plain = lambda: check(lib.np_linear_forward(x.ptr, w.ptr, None, M, K, N, 0, y.ptr))
    only_dx = lambda: check(lib.np_linear_backward(None, w.ptr, None, dy.ptr, M, K, N, 0, None, dx.ptr, None, None))
    only_dw = lambda: check(lib.np_linear_backward(x.ptr, None, None, dy.ptr, M, K, N, 0, None, None, dw.ptr, None))
    gemm_y = lambda: check(lib.np_sgemm(M, N, K, x.ptr, wt.ptr, y.ptr))
    gemm_dx = lambda: check(lib.np_sgemm(M, K, N, dy.ptr, w.ptr, dx.ptr))
    gemm_dw = lambda: check(lib.np_sgemm(N, K, M, dyt.ptr, x.ptr, dw.ptr))
    ramp()
    flop = 2.0 * M * N * K
    def forced(form, fn):
        def run():
            check(lib.np_debug_linear_force_form(form))
            fn()
            check(lib.np_debug_linear_force_form(0))
        return run

    for label, fn, gemm, product in (("y  = x . w^T", fwd_plain, gemm_y, 0), ("dx = dz . w", only_dx, gemm_dx, 1), ("dw = dz^T . x", only_dw, gemm_dw, 2)):
        t_ms, (l_ms, g_ms) = against(forced(1, fn), [forced(2, fn), gemm], 1)
        forced(1, fn)()
        tm, S = probe(product)
        fn()
        check(lib.np_debug_linear_last_path(product, *(C.byref(c) for c in (chosen, C.c_int(), C.c_int(), C.c_int()))))
        tm_, lm, gm = statistics.median(t_ms), statistics.median(l_ms), statistics.median(g_ms)
        print("(%d, %d, %d) work %.3g %-14s tile form TM %3d S %3d %9.4f ms %7.2f TFLOP/s %5.3f of the matrix peak (min %.4f max %.4f)   library form %9.4f ms %7.2f TFLOP/s "
              "%5.3f of the peak (min %.4f max %.4f)   tile / library %5.2f: the %s form is faster; unforced takes form %d   np_sgemm alone %9.4f ms (min %.4f max %.4f)"
              % (M, K, N, float(M) * K * N, label, tm, S, tm_, flop / tm_ * 1e-9, flop / tm_ * 1e-9 / MATRIX_PEAK_TFLOPS, min(t_ms), max(t_ms), lm, flop / lm * 1e-9,
                 flop / lm * 1e-9 / MATRIX_PEAK_TFLOPS, min(l_ms), max(l_ms), tm_ / lm, "library" if lm < tm_ else "tile", chosen.value, gm, min(g_ms), max(g_ms)), flush=True)

    def layer():
        check(lib.np_linear_forward(x.ptr, w.ptr, b.ptr, M, K, N, TANH, y.ptr))
        check(lib.np_linear_backward(x.ptr, w.ptr, y.ptr, dy.ptr, M, K, N, TANH, dz.ptr, dx.ptr, dw.ptr, db.ptr))

    def composition():
        gy = nd.tanh(nd.matmul(gx, nd.transpose(gw)) + gb)
        gz = gdy * (1.0 - gy * gy)
        return nd.sum(gz, 0), nd.matmul(nd.transpose(gz), gx), nd.matmul(gz, gw)

    dims = (M, K, 1, 1, N, 1, 1, 0, 0)

    def conv_route():
        check(lib.np_conv2d_forward_act(x.ptr, w.ptr, b.ptr, *dims, 1, 1, 1, 1, TANH, y.ptr))
        check(lib.np_conv2d_backward_act(y.ptr, dy.ptr, M, N, 1, TANH, dz.ptr, db.ptr))
        check(lib.np_conv2d_backward_filter(x.ptr, dz.ptr, *dims, dw.ptr))
        check(lib.np_conv2d_backward_data(dz.ptr, w.ptr, *dims, dx.ptr))

    others, names = [conv_route], ["1 x 1 convolution route"]
    try:
        composition()
        others, names = [composition] + others, ["NDArray composition"] + names
    except Exception as e:      # a composition this build cannot express is named, not hidden
        print("(%d, %d, %d) the NDArray composition is not expressed: %s" % (M, K, N, str(e)[:100]), flush=True)
    op_ms, other_ms = against(layer, others)
    om = statistics.median(op_ms)
    tail = ""
    for name, ms in zip(names, other_ms):
        med = statistics.median(ms)
        tail += "   %s %9.4f ms (min %.4f max %.4f) / layer %6.2f" % (name, med, min(ms), max(ms), med / om)
        if name == "NDArray composition" and om > med + (max(ms) - min(ms)):
            tail += "  FINDING: the layer is slower than the composition by more than its spread"
    print("(%d, %d, %d) layer, bias and tanh, forward + backward (y, dz, dx, dw, db) %9.4f ms %7.2f TFLOP/s (min %.4f max %.4f)%s"
          % (M, K, N, om, 3 * flop / om * 1e-9, min(op_ms), max(op_ms), tail), flush=True)

    act_only = lambda: check(lib.np_linear_backward(None, None, y.ptr, dy.ptr, M, K, N, TANH, dz.ptr, None, None, db.ptr))
    nbytes = 12 * M * N
    copy = lambda: check(lib.np_memcpy_d2d(c1.ptr, c2.ptr, nbytes // 2))
    op_ms, (c_ms,) = against(act_only, [copy], 1)
    act_only()
    om, cm = statistics.median(op_ms), statistics.median(c_ms)
    print("(%d, %d, %d) dz and db (tanh), S %3d %9.4f ms %5.2f TB/s (min %.4f max %.4f)   float4 copy of the same bytes %9.4f ms %5.2f TB/s (min %.4f max %.4f)   "
          "copy / kernel %5.2f" % (M, K, N, probe(3)[1], om, nbytes / om * 1e-9, min(op_ms), max(op_ms), cm, nbytes / cm * 1e-9, min(c_ms), max(c_ms), cm / om), flush=True)


def run_groupnorm(i, rounds, sets):
    """one shape: forward, backward with the parameter gradients, backward without them, each alternating with a float4 copy of the
    bytes its forms move; for the 2-D shapes the forward pass also with the NDArray composition and batch norm's rows form"""
    import ctypes as C_
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    t = Timer()
    name, (N, G, Dg, inner), compare = GROUPNORM_SHAPES[i]
    M, L, P = N * G, Dg * inner, G * Dg
    n = M * L
    if sets < 1:
        sets = max(2, -(-(256 << 20) // (4 * n)) + 1)
    rng = np.random.default_rng(i)
    block = rng.standard_normal(1 << 20).astype(np.float32)
    host = np.resize(block, n)
    xs = [D.DeviceArray.from_host(host) for _ in range(sets)]
    ys, dys, dxs = ([D.DeviceArray((n,)) for _ in range(sets)] for _ in range(3))
    for d in dys:
        check(lib.np_memcpy_d2d(d.ptr, xs[0].ptr, 4 * n))
    words = 7 * n // 2 + 16
    cs, cd = [D.DeviceArray((words,)) for _ in range(sets)], [D.DeviceArray((words,)) for _ in range(sets)]      # the copy's own operands
    for c in cs:
        check(lib.np_memset0(c.ptr, 4 * words))
    gamma, beta = D.DeviceArray.from_host(rng.standard_normal(P).astype(np.float32)), D.DeviceArray.from_host(rng.standard_normal(P).astype(np.float32))
    stat = max(M, P)
    mean, invstd = D.DeviceArray((stat,)), D.DeviceArray((stat,))
    dgamma, dbeta = D.DeviceArray((P,)), D.DeviceArray((P,))
    dims = (N, G, Dg, inner)
    ramp()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def copy_of(total_bytes):
        half = total_bytes // 2 // 16 * 16        # a copy of B / 2 bytes reads B / 2 and writes B / 2
        return rotating(lambda k: check(lib.np_memcpy_d2d(cd[k].ptr, cs[k].ptr, half)))

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    def probe():
        v = [C_.c_int(), C_.c_int(), C_.c_int(), C_.c_size_t(), C_.c_size_t()]
        check(lib.np_debug_groupnorm_last_path(*[C_.byref(a) for a in v]))
        return tuple(a.value for a in v)

    composition = batchnorm = None
    if compare:                                   # what a user writes today for an (M, L) array: single-axis means and column broadcasts
        from numpower_amd.ndarray import NDArray as nd
        gx = nd.array(host.reshape(M, L)).gpu()
        gg, gb = nd.array(np.ones(L, np.float32)).gpu(), nd.array(np.zeros(L, np.float32)).gpu()

        def composition():
            m = nd.reshape(nd.mean(gx, 1), [M, 1])
            xc = gx - m
            inv = 1.0 / nd.sqrt(nd.reshape(nd.mean(xc * xc, 1), [M, 1]) + 1e-5)
            return xc * inv * gg + gb

        try:
            composition()
        except Exception as e:                    # the composition is a comparison, not the subject
            print("%-28s the NDArray composition is not expressed: %s" % (name, e), flush=True)
            composition = None
        # the nearest call the library had: batch normalization's rows form on the same (M, L) array, statistics per column
        batchnorm = rotating(lambda k: check(lib.np_batchnorm_forward(xs[k].ptr, gamma.ptr, beta.ptr, M, L, 1, 1, 0.1, 1e-5, None, None, ys[k].ptr, mean.ptr, invstd.ptr)))

    forward = rotating(lambda k: check(lib.np_groupnorm_forward(xs[k].ptr, gamma.ptr, beta.ptr, *dims, 1e-5, ys[k].ptr, mean.ptr, invstd.ptr)))
    backward = rotating(lambda k: check(lib.np_groupnorm_backward(xs[k].ptr, dys[k].ptr, gamma.ptr, mean.ptr, invstd.ptr, *dims, dxs[k].ptr, dgamma.ptr, dbeta.ptr)))
    backward_dx = rotating(lambda k: check(lib.np_groupnorm_backward(xs[k].ptr, dys[k].ptr, gamma.ptr, mean.ptr, invstd.ptr, *dims, dxs[k].ptr, None, None)))
    forward()
    split = probe()[0] == 4
    ops = [("forward", forward, (12 if split else 8) * n, True), ("backward", backward, (28 if split else 20) * n, False),
           ("backward, dx alone", backward_dx, (20 if split else 12) * n, False)]
    for label, fn, nbytes, against in ops:
        copy = copy_of(nbytes)
        for f in (fn, copy):                      # warm
            for _ in range(3):
                f()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(5, min(200, int(0.05 / max(time.time() - t0, 1e-5))))
        op_ms, copy_ms, comp_ms, bn_ms = [], [], [], []
        for _ in range(rounds):                   # alternating in one session
            op_ms.append(timed(fn, reps))
            copy_ms.append(timed(copy, reps))
            if against and composition is not None:
                comp_ms.append(timed(composition, max(2, reps // 8)))
            if against and batchnorm is not None:
                bn_ms.append(timed(batchnorm, reps))
        fn()
        row, param, launches, rs, ps = probe()
        om, cm = statistics.median(op_ms), statistics.median(copy_ms)
        tail = ""
        if comp_ms:
            pm = statistics.median(comp_ms)
            tail += "   composition %9.4f ms   composition / op %6.2f" % (pm, pm / om)
        if bn_ms:
            bm = statistics.median(bn_ms)
            tail += "   batch norm rows form %9.4f ms   batch norm / op %6.2f" % (bm, bm / om)
        print("%-28s %-18s forms %d %d launches %d S %4d %4d %8.1f MB %9.4f ms %5.2f TB/s   copy %9.4f ms %5.2f TB/s   copy / op %5.2f   (min %5.2f max %5.2f)%s"
              % (name, label, row, param, launches, rs, ps, nbytes * 1e-6, om, nbytes / om * 1e-9, cm, nbytes / cm * 1e-9, cm / om,
                 min(c / p for c, p in zip(copy_ms, op_ms)), max(c / p for c, p in zip(copy_ms, op_ms)), tail), flush=True)


def run_attention(i, rounds):
    """one shape, causal and not: forward, backward, backward with dq alone; the forward pass without causal also against the NDArray
    composition and against np_sgemm_strided_batched on the two products alone, alternating round by round"""
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    from numpower_amd.ndarray import NDArray as nd
    t = Timer()
    BH, S, Dh = ATTENTION_SHAPES[i]
    n, scale = BH * S * Dh, float(np.float32(1.0) / np.sqrt(np.float32(Dh)))
    rng = np.random.default_rng(i)
    host = [np.resize(rng.standard_normal(1 << 20).astype(np.float32), n) for _ in range(4)]
    q, k, v, dout = (D.DeviceArray.from_host(h) for h in host)
    o, dq, dk, dv = (D.DeviceArray((n,)) for _ in range(4))
    smax, ssum = D.DeviceArray((BH * S,)), D.DeviceArray((BH * S,))
    kt = D.DeviceArray.from_host(np.ascontiguousarray(host[1].reshape(BH, S, Dh).transpose(0, 2, 1)).reshape(-1))      # k^T, made outside the timing
    scores = D.DeviceArray((BH * S * S,))
    gq, gk, gv = (nd.array(h.reshape(BH, S, Dh)).gpu() for h in host[:3])

    def composition():
        return nd.batched_matmul(nd.softmax(nd.batched_matmul(gq, nd.transpose(gk, (0, 2, 1))) * scale, -1), gv)

    def products():
        check(lib.np_sgemm_strided_batched(BH, S, S, Dh, q.ptr, S * Dh, kt.ptr, Dh * S, scores.ptr, S * S))
        check(lib.np_sgemm_strided_batched(BH, S, Dh, S, scores.ptr, S * S, v.ptr, S * Dh, o.ptr, S * Dh))

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    ramp()
    for causal in (0, 1):
        forward = lambda: check(lib.np_attention_forward(q.ptr, k.ptr, v.ptr, BH, S, S, Dh, causal, scale, o.ptr, smax.ptr, ssum.ptr))
        backward = lambda: check(lib.np_attention_backward(q.ptr, k.ptr, v.ptr, o.ptr, dout.ptr, smax.ptr, ssum.ptr, BH, S, S, Dh, causal, scale, dq.ptr, dk.ptr, dv.ptr))
        backward_dq = lambda: check(lib.np_attention_backward(q.ptr, k.ptr, v.ptr, o.ptr, dout.ptr, smax.ptr, ssum.ptr, BH, S, S, Dh, causal, scale, dq.ptr, None, None))
        forward()
        for label, fn, flop, against in (("forward", forward, 4.0 * BH * S * S * Dh, not causal), ("backward", backward, 10.0 * BH * S * S * Dh, False),
                                         ("backward, dq alone", backward_dq, 6.0 * BH * S * S * Dh, False)):
            flop = flop / 2 if causal else flop
            others = [composition, products] if against else []
            for f in [fn] + others:                  # warm
                for _ in range(2):
                    f()
            D.sync()
            t0 = time.time()
            fn()
            D.sync()
            reps = max(3, min(100, int(0.05 / max(time.time() - t0, 1e-5))))
            op_ms, other_ms = [], [[] for _ in others]
            for _ in range(rounds):                   # alternating in one session
                op_ms.append(timed(fn, reps))
                for f, ms in zip(others, other_ms):
                    ms.append(timed(f, max(2, reps // 4)))
            om = statistics.median(op_ms)
            tail = ""
            if against:
                cm, pm = (statistics.median(ms) for ms in other_ms)
                tail = "   composition %9.4f ms   composition / fused %6.2f   two products alone %9.4f ms   products / fused %6.2f" % (cm, cm / om, pm, pm / om)
            print("(%d, %d, %d) %-10s %-19s %9.4f ms %7.2f TFLOP/s %6.3f of the matrix peak (min %.4f max %.4f ms)%s"
                  % (BH, S, Dh, "causal" if causal else "full", label, om, flop / om * 1e-9, flop / om * 1e-9 / MATRIX_PEAK_TFLOPS, min(op_ms), max(op_ms), tail), flush=True)


def run_softmax(i, rounds, sets):
    """one shape: every operation alternates with a float4 copy of the same bytes and (row shapes) with the four-pass composition"""
    import ctypes as C_
    import numpy as np
    D, lib, check, ramp, _ = _setup()
    from numpower_amd._lib import Timer
    t = Timer()
    name, (outer, cols, inner) = SOFTMAX_SHAPES[i]
    n = outer * cols * inner
    if sets < 1:
        sets = max(2, -(-(256 << 20) // (4 * n)) + 1)
    rng = np.random.default_rng(i)
    block = rng.standard_normal(1 << 20).astype(np.float32)
    host = np.resize(block, n)
    labels = rng.integers(0, cols, outer).astype(np.float32)
    xs = [D.DeviceArray.from_host(host) for _ in range(sets)]
    ys, dys, dxs = ([D.DeviceArray((n,)) for _ in range(sets)] for _ in range(3))
    for d in dys:
        check(lib.np_memcpy_d2d(d.ptr, xs[0].ptr, 4 * n))
    cs, cd = [D.DeviceArray((3 * n // 2 + 16,)) for _ in range(sets)], [D.DeviceArray((3 * n // 2 + 16,)) for _ in range(sets)]      # the copy's own operands
    for c in cs:
        check(lib.np_memset0(c.ptr, 4 * (3 * n // 2 + 16)))
    tg, losses = D.DeviceArray.from_host(labels), D.DeviceArray((outer,))
    dims = (outer, cols, inner)
    ramp()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def copy_of(total_bytes):
        half = total_bytes // 2 // 16 * 16        # a copy of B / 2 bytes reads B / 2 and writes B / 2
        return rotating(lambda k: check(lib.np_memcpy_d2d(cd[k].ptr, cs[k].ptr, half)))

    def timed(fn, reps):
        t.start()
        for _ in range(reps):
            fn()
        t.stop()
        return t.elapsed_ms() / reps

    composition = None
    if inner == 1:                                # what examples/softmax_regression.py does per step for its loss: four passes over (rows, cols)
        from numpower_amd.lazy import Lazy  # noqa: F401  (installs NDArray.lazy)
        from numpower_amd.ndarray import NDArray as nd
        logits = nd.array(host.reshape(outer, cols)).gpu()
        onehot = np.zeros((outer, cols), np.float32)
        onehot[np.arange(outer), labels.astype(np.int64)] = 1.0
        gY = nd.array(onehot).gpu()
        del onehot

        def composition():
            row_max = nd.reshape(nd.max(logits, 1), [outer, 1])
            row_sum = nd.reshape((logits.lazy() - row_max).exp().sum(axis=1), [outer, 1])
            P = ((logits.lazy() - row_max).exp() / row_sum).eval()
            return -(P.lazy().log() * gY).sum() / outer

    for k in range(sets):                         # the backward passes read an output of the forward pass
        check(lib.np_softmax_forward(xs[k].ptr, *dims, 0, ys[k].ptr))
    ops = [("softmax", rotating(lambda k: check(lib.np_softmax_forward(xs[k].ptr, *dims, 0, ys[k].ptr))), 8 * n, False),
           ("log-softmax", rotating(lambda k: check(lib.np_softmax_forward(xs[k].ptr, *dims, 1, dxs[k].ptr))), 8 * n, False),
           ("softmax backward", rotating(lambda k: check(lib.np_softmax_backward(ys[k].ptr, dys[k].ptr, *dims, 0, dxs[k].ptr))), 12 * n, False),
           ("log-softmax backward", rotating(lambda k: check(lib.np_softmax_backward(ys[k].ptr, dys[k].ptr, *dims, 1, dxs[k].ptr))), 12 * n, False)]
    if inner == 1:
        ops.append(("cross-entropy + gradient", rotating(lambda k: check(lib.np_cross_entropy(xs[k].ptr, tg.ptr, outer, cols, 0, 1.0 / outer, losses.ptr, dxs[k].ptr))),
                    8 * n + 8 * outer, True))
        ops.append(("cross-entropy, loss alone", rotating(lambda k: check(lib.np_cross_entropy(xs[k].ptr, tg.ptr, outer, cols, 0, 1.0, losses.ptr, None))),
                    4 * n + 8 * outer, True))
    for label, fn, nbytes, against in ops:
        copy = copy_of(nbytes)
        for f in (fn, copy):                      # warm
            for _ in range(3):
                f()
        D.sync()
        t0 = time.time()
        fn()
        D.sync()
        reps = max(5, min(200, int(0.05 / max(time.time() - t0, 1e-5))))
        op_ms, copy_ms, comp_ms = [], [], []
        for _ in range(rounds):                   # alternating in one session
            op_ms.append(timed(fn, reps))
            copy_ms.append(timed(copy, reps))
            if against and composition is not None:
                comp_ms.append(timed(composition, max(2, reps // 8)))
        om, cm = statistics.median(op_ms), statistics.median(copy_ms)
        form = C_.c_int()
        check(lib.np_debug_softmax_last_path(C_.byref(form)))
        tail = ""
        if comp_ms:
            pm = statistics.median(comp_ms)
            tail = "   composition %9.4f ms   composition / op %6.2f" % (pm, pm / om)
        print("%-34s %-26s form %d %8.1f MB %9.4f ms %5.2f TB/s   copy %9.4f ms %5.2f TB/s   copy / op %5.2f   (min %5.2f max %5.2f)%s"
              % (name, label, form.value, nbytes * 1e-6, om, nbytes / om * 1e-9, cm, nbytes / cm * 1e-9, cm / om,
                 min(c / p for c, p in zip(copy_ms, op_ms)), max(c / p for c, p in zip(copy_ms, op_ms)), tail), flush=True)


def run_torch(layers, rounds):
    import torch
    if not torch.cuda.is_available():
        print("torch.nn.functional.conv2d: this torch sees no device", flush=True)
        return
    for i in layers:
        xs, ws, ys, pad, gemms = shapes(i)
        x = torch.randn(xs, device="cuda", requires_grad=True)
        w = torch.randn(ws, device="cuda", requires_grad=True)
        dy = torch.randn(ys, device="cuda")

        def ms(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            out = []
            for _ in range(rounds):
                t0 = time.time()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                out.append((time.time() - t0) / 5 * 1e3)
            return statistics.median(out)

        sh, sw, dh, dw = geometry(i)
        fwd = ms(lambda: torch.nn.functional.conv2d(x.detach(), w.detach(), padding=pad, stride=(sh, sw), dilation=(dh, dw)))

        def both():
            x.grad = w.grad = None
            torch.nn.functional.conv2d(x, w, padding=pad, stride=(sh, sw), dilation=(dh, dw)).backward(dy)

        print("%-42s torch (information): forward %.4f ms, forward + both gradients %.4f ms" % (LAYERS[i][0], fwd, ms(both)), flush=True)


if args.profile is not None:
    run_layer(args.profile, 1, profile=True)
    sys.exit(0)
if args.child:
    if args.child == "torch":
        run_torch([int(s) for s in args.layers.split(",")], args.rounds)
    elif args.child.startswith("act:"):
        run_act(args.child.split(":")[1], args.rounds)
    elif args.child.startswith("pool:"):
        run_pool(int(args.child.split(":")[1]), args.rounds, args.sets)
    elif args.child.startswith("batchnorm:"):
        run_batchnorm(int(args.child.split(":")[1]), args.rounds, args.sets)
    elif args.child.startswith("linear:"):
        run_linear(int(args.child.split(":")[1]), args.rounds)
    elif args.child.startswith("optim:"):
        run_optim(int(args.child.split(":")[1]), args.rounds)
    elif args.child.startswith("attention:"):
        run_attention(int(args.child.split(":")[1]), args.rounds)
    elif args.child.startswith("groupnorm:"):
        run_groupnorm(int(args.child.split(":")[1]), args.rounds, args.sets)
    elif args.child.startswith("softmax:"):
        run_softmax(int(args.child.split(":")[1]), args.rounds, args.sets)
    elif args.child.startswith("fwd:"):
        run_forward_only(int(args.child.split(":")[1]), args.rounds)
    else:
        run_layer(int(args.child.split(":")[1]), args.rounds)
    sys.exit(0)

lines = []


def say(line=""):
    print(line, flush=True)
    lines.append(line)


def child(what):
    """-> True when the child ended well; its output joins the log either way"""
    try:
        proc = subprocess.run([sys.executable, __file__, "--child", what, "--layers", args.layers, "--rounds", str(args.rounds), "--sets", str(args.sets)],
                              capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        say("%s: no result inside %d s" % (what, args.limit))
        return False
    for line in proc.stdout.splitlines():
        say(line)
    if proc.returncode != 0:
        say("%s: ended with status %d: %s" % (what, proc.returncode, proc.stderr.strip().splitlines()[-1] if proc.stderr.strip() else ""))
    return proc.returncode == 0


kind = "linear" if args.linear else "optim" if args.optim else "attention" if args.attention else "groupnorm" if args.groupnorm else "batchnorm" if args.batchnorm else "softmax" if args.softmax else "pool" if args.pool else "act" if args.act else "fwd" if args.forward_only else "layer"
if args.linear:
    import hashlib
    say("np_linear_forward / np_linear_backward, (M, K, N): each product against bare np_sgemm on dense operands of the same extents; the whole layer (a bias, "
        "tanh; y, dz, dx, dw, db) against the composition from NDArray calls and against the 1 x 1 convolution route; the dz / db kernel against np_memcpy_d2d "
        "(the float4 copy) of the same bytes; alternating round by round in one process; TFLOP/s from 2 M N K per product against the %.1f TFLOP/s fp32 matrix "
        "peak; fp32, ms per call, medians of %d rounds.  Every product is timed with the tile form forced and with the library form forced; work = M.K.N is what "
        "the dispatcher compares with its constant per product; the layer and the dz / db kernel run unforced." % (MATRIX_PEAK_TFLOPS, args.rounds))
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_linear.hip", "np_dnn_tile.h", "np_internal.h")))
elif args.optim:
    import hashlib
    say("np_sgd_step / np_adam_step / np_grad_norm: the step against np_memcpy_d2d (the float4 copy) of the same bytes and against np_binary add over the same "
        "bytes, alternating round by round in one process; the wall time of a step over 300 small tensors against the NDArray compositions; the norm against "
        "np_reduce_all; fp32, medians of %d rounds" % args.rounds)
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_optim.hip", "np_internal.h")))
elif args.attention:
    import hashlib
    say("np_attention_forward / np_attention_backward with all three gradients and with dq alone, Sq = Sk = S, causal and not; useful TFLOP/s from 4.BH.S.S.D "
        "forward and 10.BH.S.S.D backward (6 for dq alone: its three products), halved under causal, against the %.1f TFLOP/s fp32 matrix peak; the forward pass without causal "
        "against the composition from NDArray calls and np_sgemm_strided_batched on the two products alone, alternating round by round; fp32, ms per call, "
        "medians of %d rounds" % (MATRIX_PEAK_TFLOPS, args.rounds))
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_attention.hip", "np_elementwise_ops.h", "np_internal.h")))
elif args.groupnorm:
    import hashlib
    say("np_groupnorm_forward / np_groupnorm_backward with and without dgamma and dbeta (row form: 1 short rows, 2 a wave per row, 3 a workgroup per row, "
        "4 split; parameter form: 0 none, 1 columns, 2 planes) against np_memcpy_d2d (the float4 copy) of the bytes the forms move and, for two 2-D shapes, "
        "the forward pass against the composition from NDArray calls and against np_batchnorm_forward's rows form on the same array, alternating round by "
        "round; fp32, ms per call, medians of %d rounds" % args.rounds)
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_groupnorm.hip", "np_batchnorm.hip", "np_internal.h")))
elif args.batchnorm:
    import hashlib
    say("np_batchnorm_forward (training, inference) / np_batchnorm_backward (form of the launch: 1 one launch, 2 split, 3 rows, 4 inference's apply kernel) "
        "against np_memcpy_d2d (the float4 copy) of the bytes the form moves and, for (N, C) shapes, the training forward against the composition from "
        "NDArray calls, alternating round by round; fp32, ms per call, medians of %d rounds" % args.rounds)
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_batchnorm.hip", "np_internal.h")))
elif args.softmax:
    import hashlib
    say("np_softmax_forward / np_softmax_backward / np_cross_entropy (form of the launch: 1 short rows, 2 a wave per row, 3 a workgroup per row, 4 streaming, 5 strided) "
        "against np_memcpy_d2d (the float4 copy) of the same bytes read + written and against the four-pass composition of examples/softmax_regression.py, "
        "alternating round by round; fp32, ms per call, medians of %d rounds" % args.rounds)
    say("sources: " + ", ".join("%s sha256 %s" % (f, hashlib.sha256((ROOT / "numpower_amd" / "csrc" / f).read_bytes()).hexdigest()[:16])
                                for f in ("np_softmax.hip", "np_elementwise_ops.h", "np_internal.h")))
elif args.pool:
    say("np_pool2d_forward / np_pool2d_backward (forms of the last forward and backward launch: forward 1 direct, 2 staged; backward 1 gather) against np_memcpy_d2d (the float4 copy) of the same "
        "bytes read + written, alternating round by round; fp32, ms per call, medians of %d rounds" % args.rounds)
elif args.act:
    say("np_conv2d_forward_act (a bias and relu) against np_conv2d_forward(_ex), np_conv2d_backward_act (relu, dz and db) against np_binary "
        "multiply on the same element count; fp32, ms per call, median of %d rounds" % args.rounds)
elif args.forward_only:
    say("the forward pass alone, fp32, ms per call, median of %d rounds" % args.rounds)
else:
    say("np_conv2d_forward / _backward_data / _backward_filter, fp32, median of %d rounds; gemm = np_sgemm on dense operands of the same M, N, K" % args.rounds)
    say("%-42s %-8s %6s %9s %7s %9s %8s %9s %8s %7s %4s %4s %4s" % ("layer", "op", "M", "N", "K", "conv ms", "TFLOP/s", "gemm ms", "TFLOP/s", "gemm/conv", "TM",
                                                                      "S", "form"))
ok = True
for i in (int(s) for s in args.layers.split(",")):
    ok = child("%s:%d" % (kind, i))
    if not ok:
        break                                   # nothing more is started on a device after a failure
if ok and args.act:
    ok = child("act:large")
if ok and args.torch:
    if not child("torch"):
        say("torch.nn.functional.conv2d did not run on the device in this installation")
out = Path(args.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
