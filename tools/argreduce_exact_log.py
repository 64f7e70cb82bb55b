"""profiles/argreduce/exact_tests.log from one run of the exact argmax / argmin tests on the GPU and one mutation run:

    python -m pytest tests/test_gpu_argreduce_exact.py -m gpu -vv -s --junitxml=run.xml > run.txt
    python tools/argreduce_mutants.py build DIR && python tools/argreduce_mutants.py run DIR
    python tools/argreduce_exact_log.py run.txt run.xml DIR

-s lets the `ARG-RECORD <case> | <record>` line of every (case, offset) and the `ARG-LAUNCHES <kernel> | <count>` line of every case
through, -vv names the test in front of its lines; the times come from the junit file.  The log holds the table kernel instantiation
-> first test id that asserts it, per mutant the tests of the module that fail on it, and per test id its wall time (setup + call +
teardown), its launches and the distinct records it asserted."""
import collections
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
MODULE = "tests/test_gpu_argreduce_exact.py::"
sys.path.insert(0, str(ROOT / "tools"))


def main(source, junit, mutant_dir, target):
    import xml.etree.ElementTree as ET
    from argreduce_mutants import EQUIVALENT
    lines = Path(source).read_text().splitlines()
    tests, launches, current = collections.OrderedDict(), collections.Counter(), None
    seconds = {MODULE + case.get("name"): float(case.get("time")) for case in ET.parse(junit).getroot().iter("testcase")}
    for line in lines:
        if line.startswith(MODULE):
            cut = min([c for c in (line.find(" ARG-RECORD "), line.find(" ARG-LAUNCHES ")) if c >= 0] or [-1])
            if cut < 0:
                cut = max(line.rfind(" PASSED"), line.rfind(" FAILED"))
            current = line[:cut] if cut >= 0 else line
            tests.setdefault(current, [])
            line = line[cut + 1:] if cut >= 0 else ""
        if line.startswith("ARG-RECORD ") and current:
            tests[current].append(line[len("ARG-RECORD "):].rstrip())
        if line.startswith("ARG-LAUNCHES ") and current:
            launches[current] += int(line.rsplit("| ", 1)[1])
    summary = [l for l in lines if re.search(r"\d+ (passed|failed)", l)][-1].strip("= ")
    first, counts = collections.OrderedDict(), collections.Counter()
    for tid, records in tests.items():
        for entry in records:
            key = entry.split(" | ")[1].split(" grid=")[0] + (" xcd_runs=1" if " xcd_runs=1" in entry else "")
            first.setdefault(key, tid)
            counts[key] += 1
    listing = (Path(mutant_dir) / "LIST.txt").read_text().splitlines()
    # the device's own CU count as the walks of tools/argreduce_mutants.py printed it (`mutant <lib> cus <n>`)
    cus = {int(re.search(r" cus (\d+)$", (Path(mutant_dir) / ("arg_mut_%s.log" % e.split("\t")[0])).read_text().splitlines()[0]).group(1)) for e in listing}
    assert len(cus) == 1, cus
    out = ["# tests/test_gpu_argreduce_exact.py on one device of %d CUs: %s; %d np_argreduce calls, each with the whole framed output" % (
               cus.pop(), summary, sum(launches.values())),
           "# compared and the whole record of np_debug_argreduce_last_record asserted against the restated planner.  Made by",
           "# tools/argreduce_exact_log.py from the run's output and the logs of tools/argreduce_mutants.py.", "",
           "## kernel instantiation -> (case, offset) pairs that assert it, first test id that does"]
    out += ["%-48s %4d  %s" % (k, counts[k], first[k][len(MODULE):]) for k in sorted(first)]
    out += ["", "## mutants of np_argreduce.hip (values and indices only) -> tests of the module that fail on them"]
    uncaught = []
    for entry in listing:
        name, desc = entry.split("\t")
        log = (Path(mutant_dir) / ("arg_mut_%s.log" % name)).read_text().splitlines()
        assert log[-1].startswith("DONE"), name
        failed = [l.split(" ", 3)[2] for l in log if l.startswith("FAIL ")]
        per = collections.Counter(f.split("[")[0] for f in failed)
        out.append("%-30s %s" % (name, desc))
        if failed:
            out.append("        caught by %d of %d: %s" % (len(failed), len([l for l in log if l.startswith(("PASS ", "FAIL "))]),
                                                            ", ".join("%s x%d" % kv for kv in sorted(per.items()))))
            out.append("        first: %s" % failed[0])
        elif name in EQUIVALENT:
            out.append("        caught by none — EQUIVALENT, np_argreduce returns the same indices: %s" % EQUIVALENT[name])
        else:
            out.append("        UNCAUGHT")
            uncaught.append(name)
    out.append("%d mutants, %d caught, %d equivalent, %d uncaught%s" % (len(listing), len(listing) - len(uncaught) - len([e for e in listing if e.split("\t")[0] in EQUIVALENT]),
                                                                      len([e for e in listing if e.split("\t")[0] in EQUIVALENT]), len(uncaught),
                                                                      ": " + ", ".join(uncaught) if uncaught else ""))
    out += ["", "## per test id: wall time in seconds (setup + call + teardown; the first test's setup loads the library), np_argreduce calls, then the",
            "## distinct records its cases asserted (x count)"]
    for tid, records in tests.items():
        out.append("%6.3f  %5d  %s" % (seconds[tid], launches[tid], tid[len(MODULE):]))
        distinct = collections.OrderedDict()
        for entry in records:
            distinct[entry.split(" | ")[1]] = distinct.get(entry.split(" | ")[1], 0) + 1
        out += ["               %s%s" % (record, "  x%d" % n if n > 1 else "") for record, n in distinct.items()]
    first_id = next(iter(tests))
    out.append("first test (its setup builds what is stale, loads the library and opens the device): %.3f s; slowest of the others: %.3f s; all tests together %.3f s" % (
        seconds[first_id], max(v for k, v in seconds.items() if k != first_id), sum(seconds.values())))
    Path(target).parent.mkdir(parents=True, exist_ok=True)
    Path(target).write_text("\n".join(out) + "\n")
    print("%s: %d tests, %d calls, uncaught mutants: %s" % (target, len(tests), sum(launches.values()), uncaught or "none"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else ROOT / "profiles" / "argreduce" / "exact_tests.log")
