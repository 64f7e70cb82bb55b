#!/usr/bin/env python3
"""Record the C interface a --with-hip drop-in has to match as a data fixture.

Reads numpower.c, src/ndarray.h, src/initializers.h, src/ndmath/cuda/cuda_math.h and src/gpu_alloc.h
of a NumPower checkout and writes tests/golden/reference_abi.json:
  * for every function the --with-hip glue replaces (the cuda_* math functions, the
    NDArrayMathGPU_ElementWise* drivers and the device-buffer functions): name, return type, parameter types;
  * the unary methods whose device branch is NDArrayMathGPU_ElementWise(nda, cuda_float_<name>) in numpower.c;
  * the NDArray_* / NDARRAY_* names ndarray.h + initializers.h declare (as a macro or a function), the
    return and parameter types of the three functions ext/hip_fast.c relies on, the types of the two
    struct NDArray fields ext/hip_lazy.c reads, and whether NDArray_ADDREF increments refcount.
Parameter names, declarations and macro bodies themselves are not stored.

Run:  python tests/golden/make_reference_abi.py <NumPower checkout>
"""
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from tests.test_ext_glue_cpu import DRIVERS, GPU_ALLOC, _prototypes, _types   # noqa: E402

OUT = Path(__file__).resolve().parent / "reference_abi.json"


def main(ref: Path):
    math = _prototypes((ref / "src" / "ndmath" / "cuda" / "cuda_math.h").read_text())
    alloc = _prototypes((ref / "src" / "gpu_alloc.h").read_text())
    record = lambda protos, names: {n: dict(zip(("returns", "params"), _types(protos[n]))) for n in sorted(names)}
    nd_h = (ref / "src" / "ndarray.h").read_text()
    headers = nd_h + (ref / "src" / "initializers.h").read_text()
    declared = sorted(n for n in set(re.findall(r"\b(NDArray_\w+|NDARRAY_\w+)\b", headers))
                      if re.search(r"#define\s+%s\b|\b%s\s*\(" % (n, n), headers))
    sites = re.findall(r"NDArrayMathGPU_ElementWise\(\s*nda\s*,\s*cuda_float_(\w+)\s*\)", (ref / "numpower.c").read_text(errors="ignore"))
    fields = {name: re.sub(r"\s*\*", "*", typ) for typ, name in
              re.findall(r"^\s*(struct NDArray\s*\*|int)\s*(base|refcount)\s*;", nd_h, flags=re.M)}
    out = {
        "reference": "NumPower/numpower @ 2024_08_07",
        "generator": "tests/golden/make_reference_abi.py",
        "cuda_math": record(math, [n for n in math if n.startswith("cuda_")]),
        "drivers": record(math, DRIVERS),
        "gpu_alloc": record(alloc, GPU_ALLOC),
        "unary_call_sites": sorted(set(sites)),
        "ndarray_header_names": declared,
        "ndarray_header_functions": record(_prototypes(headers), ["NDArray_EmptyLike", "NDArray_FREE", "NDArray_IsBroadcastable"]),
        "ndarray_fields": fields,
        "addref_increments_refcount": bool(re.search(r"#define NDArray_ADDREF\(a\) \(\(a\)->refcount\+\+\)", headers)),
    }
    OUT.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
