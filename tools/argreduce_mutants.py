"""Mutation record of np_argreduce.hip against tests/test_gpu_argreduce_exact.py (profiles/argreduce/exact_tests.log).

    python tools/argreduce_mutants.py build DIR      # DIR/<name>.hip and DIR/libarg_<name>.so, here (hipcc cross-compiles)
    python tools/argreduce_mutants.py run DIR        # on the GPU: DIR/arg_mut_<name>.log, one child process per mutant
    python tools/argreduce_mutants.py walk TAG [LIB] # one walk of the test module (what `run` starts); DIR/arg_<TAG>.log

A mutant is the source with one edit that changes VALUES AND INDICES ONLY: no address, no trip count, no bound — none of them can
read or write outside an array.  Each is built into a small shared library holding np_argreduce and its probe alone; libnp_hip.so
is loaded first (RTLD_GLOBAL), so the mutant's calls into the runtime resolve there, and the walk hands the mutant's two entry
points to the test module in place of the library's.  The walk calls the module's test functions directly with every parameter
set (no pytest: the library is not rebuilt), prints PASS / FAIL per test id and ends at the first error that is no assertion.
NDArray goes through the host library and never sees a mutant: test_ndarray_* and test_probe_* are left out of mutant walks."""
import contextlib
import inspect
import io
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "numpower_amd" / "csrc" / "np_argreduce.hip"

# mutants no test can catch, and why: np_argreduce's OUTPUT is the same with and without the edit
EQUIVALENT = {
    "fixup_scan": "the fix-up only matters when an accumulator's first element EQUALS the identity and wins; element 0 of the axis is always a "
                  "candidate whose key is no worse than the identity (a NaN there is patched), so such an element ties with an earlier index "
                  "and loses: only partials change",
    "fixup_small_inner": "as fixup_scan: row 0 of every column is a candidate of slab 0",
    "fixup_small_inner4": "as fixup_scan: row 0 of every column is a candidate of slab 0",
    "key_later_nan": "a later NaN enters arg_combine only as the second operand, where a NaN key (every compare false) and the key -Inf "
                     "(ties with nothing earlier than itself) both never replace a real candidate; only a lane that met nothing else keeps "
                     "{identity, none} instead of {-Inf, index}, and that lane never holds the answer (position 0 is no later NaN)",
    "guard_fold_kernel": "every chunk and slab meets at least one element per output, so no partial carries kArgNone; and if one did, "
                         "{identity, 0xffffffff} loses every compare and every tie in arg_replace",
    "guard_fold_block": "as guard_fold_kernel; the filler {best.v, kArgNone} of the lanes past the last chunk ties on the value and loses on the index",
}


def nth(s, a, b, k):
    """s with the k-th (0-based) occurrence of a replaced by b."""
    parts = s.split(a)
    assert len(parts) > k + 1, (a, len(parts))
    return a.join(parts[:k + 1]) + b + a.join(parts[k + 1:])


def mutants():
    SRC = SOURCE.read_text()
    M = {}

    def mut(name, desc, edits):
        s = SRC
        for a, b, k, cnt in edits:
            assert s.count(a) == cnt, (name, a, s.count(a), cnt)
            s = nth(s, a, b, k)
        M[name] = (desc, s)
    mut('take_max_nonstrict','arg_take: x > bv made x >= bv',[('if constexpr (IS_MAX) r = x > bv;','if constexpr (IS_MAX) r = x >= bv;',0,1)])
    mut('take_min_nonstrict','arg_take: !(bv <= x) made !(bv < x)',[('else r = !(bv <= x) && (bv == bv);','else r = !(bv < x) && (bv == bv);',0,1)])
    T='return (vb == va) && (ib < ia);'
    mut('replace_max_tie_reversed','arg_replace<max>: ib < ia reversed',[(T,'return (vb == va) && (ib > ia);',0,2)])
    mut('replace_min_tie_reversed','arg_replace<min>: ib < ia reversed',[(T,'return (vb == va) && (ib > ia);',1,2)])
    mut('replace_nan_tie_reversed','arg_replace<min>, both NaN: ib < ia reversed',[('if (na && nb) return ib < ia;','if (na && nb) return ib > ia;',0,1)])
    mut('acc0_none_scan','arg_scan_contig: start index of accumulator 0 = kArgNone',[('s2 == 0 ? (tid < nvec ? tid : kArgNone)','s2 == 0 ? kArgNone',0,1)])
    A0='s2 == 0 ? (t < nvec ? 0u : kArgNone)'
    mut('acc0_none_small_inner','argreduce_small_inner: start index of accumulator 0 = kArgNone',[(A0,'s2 == 0 ? kArgNone',0,2)])
    mut('acc0_none_small_inner4','argreduce_small_inner4: start index of accumulator 0 = kArgNone',[(A0,'s2 == 0 ? kArgNone',1,2)])
    mut('acc0_none_cols_tile','argreduce_cols_tile: start index ba[k] = kArgNone',[('ba[k] = (first < a1 && (unsigned)k < ncol) ? first : kArgNone;','ba[k] = kArgNone;',0,1)])
    mut('fixup_scan','arg_scan_contig: the !main_runs fix-up removed',[('                if (h1) bt[1][k] = v1;\n                if (h2) bt[2][k] = v2;', '', 0, 1)])
    F = '                    if (h1) bj[1][k] = j + 1;\n                    if (h2) bj[2][k] = j + 2;'
    mut('fixup_small_inner','argreduce_small_inner: the !main_runs fix-up removed',[(F,'',0,2)])
    mut('fixup_small_inner4','argreduce_small_inner4: the !main_runs fix-up removed',[(F,'',1,2)])
    mut('head_dropped','arg_scan_contig: the head lanes\' candidate dropped',[('    if (tid < head) best = arg_combine<IS_MAX>(best, ArgPair{arg_key_later<IS_MAX>(q[tid]), base + tid});\n','',0,1)])
    mut('tail_dropped','arg_scan_contig: the tail lanes\' candidate dropped',[('    if (t < count) best = arg_combine<IS_MAX>(best, ArgPair{arg_key_later<IS_MAX>(q[t]), base + t});\n','',0,1)])
    mut('leftover_dropped_small_inner','argreduce_small_inner: the leftover elements\' candidates dropped',[('if (e % inner == t) r = arg_combine','if (false) r = arg_combine',0,1)])
    mut('nan0_rows_kernel','NaN-in-position-0 patch removed: argreduce_rows_kernel',[('        if (IS_MAX && chunk == 0 && p[0] != p[0]) r = ArgPair{INFINITY, 0u};   // a NaN in position 0 is maximal\n','',0,1)])
    mut('nan0_rows_wave','NaN-in-position-0 patch removed: argreduce_rows_wave',[('        if (IS_MAX && p[0] != p[0]) best = ArgPair{INFINITY, 0u};\n','',0,1)])
    mut('nan0_small_inner','NaN-in-position-0 patch removed: argreduce_small_inner',[('        if (IS_MAX && r0 == 0 && p[t] != p[t]) r = ArgPair{INFINITY, 0u};   // a NaN in position 0 is maximal\n','',0,1)])
    mut('nan0_small_inner4','NaN-in-position-0 patch removed: argreduce_small_inner4',[('        if (IS_MAX && r0 == 0 && p[t] != p[t]) r = ArgPair{INFINITY, 0u};\n','',0,1)])
    mut('nan0_cols_tile','NaN-in-position-0 patch removed: argreduce_cols_tile',[('if (x0 != x0) r = ArgPair{INFINITY, 0u};','if (false) r = ArgPair{INFINITY, 0u};',0,1)])
    mut('key_later_nan','arg_key_later returns x for a NaN',[('if constexpr (IS_MAX) return (x != x) ? -INFINITY : x;\n    return x;\n}\n\ntypedef v4f arg_v4f_u','return x;\n}\n\ntypedef v4f arg_v4f_u',0,1)])
    mut('guard_fold_kernel','argreduce_fold_kernel: the q.i != kArgNone guard removed',[('        if (q.i != 0xffffffffu) r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);\n    }\n    out[idx] = (float)r.i;','        r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);\n    }\n    out[idx] = (float)r.i;',0,1)])
    mut('guard_fold_block','argreduce_fold_block_kernel: the three != kArgNone guards removed',[
        ('            if (q[u].i != 0xffffffffu) best =','            best =',0,1),
        ('        if (q.i != 0xffffffffu) best = (best.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(best, q);\n    }\n    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;','        best = (best.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(best, q);\n    }\n    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;',0,1),
        ('            if (q.i != 0xffffffffu) r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);\n        }\n        out[idx] = (float)r.i;','            r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);\n        }\n        out[idx] = (float)r.i;',0,1)])
    mut('rows_per_trip_small_inner','argreduce_small_inner: rows_per_trip off by one',[('const unsigned rows_per_trip = 4 * T / inner;','const unsigned rows_per_trip = 4 * T / inner + 1;',0,1)])
    mut('rows_per_trip_small_inner4','argreduce_small_inner4: rows_per_trip off by one',[('const unsigned rows_per_trip = T / inner4, row0','const unsigned rows_per_trip = T / inner4 + 1, row0',0,1)])
    mut('xcd_runs_c','argreduce_cols_tile: the xcd_runs renumbering of c left out',[('        c = (unit / T) % chunks;\n','',0,1)])
    return M


def build(outdir):
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    M = mutants()
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"

    def one(name):
        src = outdir / (name + ".hip")
        src.write_text(M[name][1])
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I%s" % (ROOT / "include"),
                            "-I%s" % SOURCE.parent, str(src), "-o", str(outdir / ("libarg_%s.so" % name))], capture_output=True, text=True)
        return name, r.returncode, r.stderr[-500:]
    with ThreadPoolExecutor(8) as ex:
        for name, rc, err in ex.map(one, list(M)):
            print(name, "ok" if rc == 0 else "FAILED\n" + err)
    (outdir / "LIST.txt").write_text("".join("%s\t%s\n" % (k, v[0]) for k, v in M.items()))


def walk(outdir, tag, lib=None):
    sys.path.insert(0, str(ROOT))
    import ctypes as C
    from numpower_amd import _lib, device
    device.init(0)
    from tests import test_gpu_argreduce_exact as t
    dev = t.Dev()
    if lib:
        mlib = C.CDLL(str(lib))
        for fname in ("np_argreduce", "np_debug_argreduce_last_record"):
            f = getattr(mlib, fname)
            f.restype, f.argtypes = _lib.PROTOTYPES[fname]
            setattr(dev.L, fname, f)
    log = open(Path(outdir) / ("arg_%s.log" % tag), "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    say("mutant %s cus %d" % (lib or "none", dev.cus))
    npass = nfail = 0
    t0 = time.time()
    for name, fn in inspect.getmembers(t, inspect.isfunction):
        if not name.startswith("test_") or (lib and name.startswith(("test_ndarray", "test_probe"))):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        combos = [({}, "")]
        if marks:
            names = [a.strip() for a in marks[0].args[0].split(",")]
            ids = marks[0].kwargs.get("ids") or [str(i) for i in range(len(marks[0].args[1]))]
            combos = [(dict(zip(names, v if len(names) > 1 else (v,))), i) for v, i in zip(marks[0].args[1], ids)]
        for kw, cid in combos:
            tid, t1 = "%s[%s]" % (name, cid), time.time()
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    fn(dev=dev, **kw)
                say("PASS %.2fs %s" % (time.time() - t1, tid))
                npass += 1
            except AssertionError as e:      # anything else (a device error) ends the walk
                say("FAIL %.2fs %s :: %s" % (time.time() - t1, tid, str(e).replace("\n", " ")[:400]))
                nfail += 1
    say("DONE pass %d fail %d in %.1fs" % (npass, nfail, time.time() - t0))


def run(outdir):
    outdir = Path(outdir)
    for line in (outdir / "LIST.txt").read_text().splitlines():
        name = line.split("\t")[0]
        r = subprocess.run([sys.executable, __file__, "walk", "mut_" + name, str(outdir / ("libarg_%s.so" % name)), str(outdir)],
                           capture_output=True, text=True, timeout=300)
        print("%s: %s" % (name, (r.stdout.strip().splitlines() or ["no output"])[-1]), flush=True)
        if r.returncode != 0:
            print("STOP: %s ended with status %d\n%s" % (name, r.returncode, r.stderr[-800:]))
            return 1
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build(sys.argv[2])
    elif sys.argv[1] == "run":
        sys.exit(run(sys.argv[2]))
    elif sys.argv[1] == "walk":
        walk(sys.argv[4] if len(sys.argv) > 4 else ".", sys.argv[2], sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] else None)
