"""Which kernel mutation does each exact attention test catch?  

Builds np_attention.hip five more times, each with ONE line of the forward kernel changed by a text substitution, links every copy
with the library's other objects into build/attention_mutations/libnp_hip_<name>.so, and runs the by-bits tests of
tests/test_gpu_attention.py against each through NP_HIP_LIB (the C ABI of the tests goes to the mutated library; the NDArray layer
keeps the shipped one).  Writes profiles/dnn/attention_tests.log: per mutation the tests that fail, and the ones that still pass.
A mutation no test catches is a finding, printed as such.

    no_rescale         the running sum and output are not multiplied when the maximum rises
    reciprocal         o = acc . (1 / l) instead of acc / l
    mask_off_by_one    causal lets row i see key i + 1
    dropped_tail_tile  the last, partial key tile is not visited
    scale_on_q_first   q is multiplied by scale before the chain, the finished dot product is not

Usage: python tools/attention_mutations.py [--limit S]      needs the GPU; each pytest child runs under its own time limit"""
import argparse
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from numpower_amd import build  # noqa: E402

MUTATIONS = {
    "no_rescale": [("        if (__any(up)) {   // a lane whose maximum stayed multiplies by exactly 1", "        if (false) {")],
    "reciprocal": [("if (d < a.D) ob[d] = __fdiv_rn(oacc[nb][r], l);", "if (d < a.D) ob[d] = oacc[nb][r] * __fdiv_rn(1.0f, l);")],
    "mask_off_by_one": [("            if (mask && (j >= a.Sk || (a.causal && j > qi))) x[r] = -INFINITY;", "            if (mask && (j >= a.Sk || (a.causal && j > qi + 1))) x[r] = -INFINITY;")],
    "dropped_tail_tile": [("    const unsigned kt_end = key_tiles_of(q0, a.Sq, a.nkt, a.causal);\n    TileRegs<DP> pk, pv;",
                           "    const unsigned kt_full = key_tiles_of(q0, a.Sq, a.nkt, a.causal);\n"
                           "    const unsigned kt_end = kt_full - ((a.Sk % kTK) && kt_full > 1 ? 1u : 0u);\n    TileRegs<DP> pk, pv;")],
    "scale_on_q_first": [("    attn_v16f oacc[NB];\n#pragma unroll\n    for (int nb = 0; nb < NB; ++nb) oacc[nb] = attn_v16f{};\n    float m = -INFINITY, l = 0.0f;",
                          "    attn_v16f oacc[NB];\n#pragma unroll\n    for (int nb = 0; nb < NB; ++nb) oacc[nb] = attn_v16f{};\n    float m = -INFINITY, l = 0.0f;\n"
                          "#pragma unroll\n    for (int s = 0; s < DP / 2; ++s) qr[s] = qr[s] * a.scale;"),
                         ("            x[r] = s[r] * a.scale;\n            if (mask && (j >= a.Sk || (a.causal && j > qi))) x[r] = -INFINITY;\n            tm = row_max(tm, x[r]);",
                          "            x[r] = s[r];\n            if (mask && (j >= a.Sk || (a.causal && j > qi))) x[r] = -INFINITY;\n            tm = row_max(tm, x[r]);")],
}
TESTS = "exact_family_by_bits or causal_equals or saturated or null_subset or gaussian_inside"


def build_mutant(name, edits):
    src = (build.CSRC / "np_attention.hip").read_text()
    for old, new in edits:
        assert src.count(old) == 1, (name, old)
        src = src.replace(old, new)
    out = ROOT / "build" / "attention_mutations"
    out.mkdir(parents=True, exist_ok=True)
    unit, obj, lib = out / ("np_attention_%s.hip" % name), out / ("np_attention_%s.o" % name), out / ("libnp_hip_%s.so" % name)
    unit.write_text(src)
    hipcc = build._hipcc()
    build._run([hipcc, *build.HIP_FLAGS, "-c", str(unit), "-o", str(obj)])
    others = [build.OBJDIR / (Path(s).stem + ".o") for s in build.HIP_SOURCES if s != "np_attention.hip"]
    build._run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, others), str(obj), "-o", str(lib), "-ldl"])
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=240, help="seconds each pytest child may take")
    args = ap.parse_args()
    build.build_all()
    lines = ["the by-bits and bound tests of tests/test_gpu_attention.py (-k '%s') against np_attention.hip with one line of the forward kernel mutated" % TESTS]
    ok = True
    for name, edits in MUTATIONS.items():
        lib = build_mutant(name, edits)
        env = dict(os.environ, NP_HIP_LIB=str(lib))
        try:
            proc = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_attention.py", "-m", "gpu", "-q", "-k", TESTS, "-p", "no:cacheprovider", "-rf",
                                   "--tb=no"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append("%-18s no result inside %d s" % (name, args.limit))
            ok = False
            break                                  # nothing more is started on a device after that
        failed = sorted(set(re.findall(r"^FAILED tests/test_gpu_attention\.py::(\S+)", proc.stdout, flags=re.M)))
        tally = proc.stdout.strip().splitlines()[-1] if proc.stdout.strip() else "(no output)"
        lines.append("%-18s %s" % (name, tally))
        if proc.returncode not in (0, 1):
            lines.append("%-18s pytest ended with status %d: %s" % (name, proc.returncode, proc.stderr.strip().splitlines()[-1] if proc.stderr.strip() else ""))
            ok = False
            break
        lines.append("    caught by: " + (", ".join(failed) if failed else "NO TEST (a finding)"))
    out = ROOT / "profiles" / "dnn" / "attention_tests.log"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
