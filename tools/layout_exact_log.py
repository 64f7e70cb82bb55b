"""profiles/layout/exact_tests.log from one run of the exact layout tests on the GPU:

    python -m pytest tests/test_gpu_layout_exact.py -m gpu -vv -s --junitxml=run.xml > run.txt
    python tools/layout_exact_log.py run.txt run.xml

-s lets the `LAYOUT-RECORD <call> | <record>` line of every launch through, -vv names the test in front of its lines; the
times come from the junit file, which has every test to the millisecond (--durations rounds to 10 ms).  The log holds, per test
id, its wall time (setup + call + teardown) and the distinct records its launches asserted with their counts; the table kernel instantiation -> first test id that asserts it;
the values of out_pitch mod 32 the write-aligned launches covered."""
import collections
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
MODULE = "tests/test_gpu_layout_exact.py::"


def instantiation(record):
    head = record.split(" ")[0]
    order, runs = re.search(r" order=(\d)", record), re.search(r" xcd_runs=(\d)", record)
    return head + (" order=" + order.group(1) if order and head.startswith(("TILE", "WALIGN")) else "") + (" xcd_runs=" + runs.group(1) if runs else "")


def main(source, junit, target):
    import xml.etree.ElementTree as ET
    lines = Path(source).read_text().splitlines()
    tests, current = collections.OrderedDict(), None
    seconds = {MODULE + case.get("name"): float(case.get("time")) for case in ET.parse(junit).getroot().iter("testcase")}
    for line in lines:
        if line.startswith(MODULE):
            cut = line.find(" LAYOUT-RECORD ")
            if cut < 0:
                cut = max(line.rfind(" PASSED"), line.rfind(" FAILED"))
            current = line[:cut] if cut >= 0 else line
            tests.setdefault(current, [])
            line = line[cut + 1:] if cut >= 0 else ""
        if line.startswith("LAYOUT-RECORD ") and current:
            tests[current].append(line[len("LAYOUT-RECORD "):].rstrip())
    summary = [l for l in lines if re.search(r"\d+ (passed|failed)", l)][-1].strip("= ")
    first, counts, shifts, pitched = collections.OrderedDict(), collections.Counter(), {64: set(), 128: set()}, collections.OrderedDict()
    for tid, records in tests.items():
        for entry in records:
            what, record = entry.split(" | ")
            key = instantiation(record)
            first.setdefault(key, tid)
            counts[key] += 1
            walign = re.match(r"WALIGN<(\d+)>.*pitch=\d+/(\d+)", record)
            if walign:
                shifts[int(walign.group(1))].add(int(walign.group(2)) % 32)
            if what.startswith("permute") and record.startswith(("TILE", "WALIGN")):
                pitched.setdefault("%s through np_permute, nbatch=%s" % (key, re.search(r"nbatch=(\d)", record).group(1)), tid)
    out = ["# tests/test_gpu_layout_exact.py on one MI355X (256 CUs): %s; %d launches, each with the whole framed output compared" % (
               summary, sum(len(v) for v in tests.values())),
           "# bit for bit and the whole record of np_debug_layout_last_record asserted against the restated dispatcher.  Made by",
           "# tools/layout_exact_log.py from the run's output.", "",
           "## kernel instantiation -> launches asserted, first test id that asserts it"]
    out += ["%-34s %5d  %s" % (k, counts[k], first[k][len(MODULE):]) for k in sorted(first)]
    out += ["%-62s %s" % (k, v[len(MODULE):]) for k, v in pitched.items()]
    out += ["not reached here: permute_gather_kernel<uint64_t, 1 | 4> (2^31 elements and more; docs/COVERAGE.md row (f3))", "",
            "## out_pitch % 32 of the write-aligned launches"]
    out += ["WALIGN<%d>: %s%s" % (t, " ".join(map(str, sorted(shifts[t]))), "  (all of 1 .. 31)" if shifts[t] >= set(range(1, 32)) else "  INCOMPLETE")
            for t in (64, 128)]
    out += ["", "## per test id: wall time in seconds (setup + call + teardown; the first test's setup loads the library; 0.000 = below half a millisecond), then the distinct",
            "## records its launches asserted (x count)"]
    for tid, records in tests.items():
        out.append("%6.3f  %s" % (seconds[tid], tid[len(MODULE):]))
        distinct = collections.OrderedDict()
        for entry in records:
            distinct[entry.split(" | ")[1]] = distinct.get(entry.split(" | ")[1], 0) + 1
        out += ["        %s%s" % (record, "  x%d" % n if n > 1 else "") for record, n in distinct.items()]
    out.append("slowest test: %.3f s; all tests together %.3f s" % (max(seconds.values()), sum(seconds.values())))
    Path(target).parent.mkdir(parents=True, exist_ok=True)
    Path(target).write_text("\n".join(out) + "\n")
    print("%s: %d tests, %d launches" % (target, len(tests), sum(len(v) for v in tests.values())))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ROOT / "profiles" / "layout" / "exact_tests.log")
