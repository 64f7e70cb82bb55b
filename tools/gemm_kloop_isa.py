"""The K loops of sgemm_dma_kernel / sgemm_streamk_kernel as the compiler emits them: for every instantiation the resource lines
(VGPRs, scratch, LDS, occupancy) and, for its hottest basic block (the one with the most MFMAs: the steady-state iteration of
the flat-addressed loop, the three-tile trip of the buffer-addressed one), the instruction counts by class.
Usage: python tools/gemm_kloop_isa.py [np_sgemm.s]   (without an argument: compiles numpower_amd/csrc/np_sgemm.hip with -S first)
A record for profiles/kloop/kloop_isa.log, not a test."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def assembly():
    if len(sys.argv) > 1:
        return Path(sys.argv[1]).read_text()
    from numpower_amd import build
    out = Path(tempfile.mkdtemp()) / "np_sgemm.s"
    subprocess.run([build._hipcc(), *build.HIP_FLAGS, "--cuda-device-only", "-S", str(build.CSRC / "np_sgemm.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def classify(op):
    if "mfma" in op:
        return "MFMA"
    if op.startswith("ds_"):
        return "DS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


text = assembly()
for m in re.finditer(r"^(_ZN\S*(sgemm_dma_kernel|sgemm_streamk_kernel)\S*):[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel(.*?; Occupancy:\s*\d+)", text, re.S | re.M):
    name, body, info = m.group(1), m.group(3), m.group(4)
    flags = re.search(r"kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
    edge, ktail, prio, buf = (int(x) for x in flags.groups())
    res = {k: re.search(r"\.amdhsa_%s\s+(\S+)" % k, body) for k in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
    occ = re.search(r"; Occupancy:\s*(\d+)", info)
    scratch = re.search(r"; ScratchSize:\s*(\d+)", info)
    vg = re.search(r"; NumVgprs:\s*(\d+)", info)
    print("%s<EDGE=%d, KTAIL=%d, PRIO=%d, BUF=%d>: VGPRs %s, scratch %s B, LDS %s B, occupancy %s waves/SIMD"
          % (m.group(2), edge, ktail, prio, buf, vg.group(1) if vg else "?", scratch.group(1) if scratch else "?",
             res["group_segment_fixed_size"].group(1) if res["group_segment_fixed_size"] else "?", occ.group(1) if occ else "?"))
    code = body.split(".section")[0]
    blocks, cur, label = [], [], "entry"
    for line in code.splitlines():
        line = line.split(";")[0].strip()
        if not line or line.startswith("."):
            if line.startswith(".LBB") and line.endswith(":"):
                blocks.append((label, cur))
                cur, label = [], line[:-1]
            continue
        if line.endswith(":"):
            blocks.append((label, cur))
            cur, label = [], line[:-1]
            continue
        cur.append(line)
    blocks.append((label, cur))
    print("    blocks with MFMAs: " + ", ".join("%s %d" % (l, sum("mfma" in i for i in b)) for l, b in blocks if any("mfma" in i for i in b)))
    label, hot = max(blocks, key=lambda b: sum("mfma" in i for i in b[1]))
    counts = {}
    for ins in hot:
        c = classify(ins.split()[0])
        counts[c] = counts.get(c, 0) + 1
    lds_dma = sum(1 for i in hot if i.split()[0].startswith(("buffer_load", "global_load")) and " lds" in i + " ")
    valu = sorted({i.split()[0] for i in hot if classify(i.split()[0]) == "VALU"})
    print("    hottest block %s: %s; LDS-DMA pieces %d; VALU opcodes: %s"
          % (label, ", ".join("%s %d" % kv for kv in sorted(counts.items())), lds_dma, " ".join(valu) or "none"))
