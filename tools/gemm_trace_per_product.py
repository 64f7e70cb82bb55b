"""Time per product of the headline's 256 x 128 LDS-DMA launches from a rocprofv3 --kernel-trace CSV of `python bench.py --steps 20`
(kernel trace alone, no counters): the last 320 launches of sgemm_dma_kernel (the timed region: 20 steps of 16), their durations
and — the figure that compares, since overlapped launches' own durations cover their predecessor too (profiles/overlap/) — the
distance from end stamp to end stamp.
Usage: python tools/gemm_trace_per_product.py <label> <kernel_trace.csv> [last N launches, default 320]"""
import csv
import statistics
import sys

label, path = sys.argv[1], sys.argv[2]
last = int(sys.argv[3]) if len(sys.argv) > 3 else 320
key = lambda r, *names: next((r[n] for n in names if n in r and r[n] != ""), "?")   # noqa: E731
ev = []
for r in csv.DictReader(open(path)):
    name = key(r, "Kernel_Name", "kernel_name")
    if "sgemm_dma_kernel" in name:
        ev.append((int(key(r, "Start_Timestamp", "start_timestamp")), int(key(r, "End_Timestamp", "end_timestamp")), name,
                   key(r, "Queue_Id", "queue_id")))
ev.sort(key=lambda e: e[1])
print("%s: %d launches of sgemm_dma_kernel in the trace; instantiations: %s" % (label, len(ev), sorted({e[2] for e in ev})))
ev = ev[-last:]
dur = [(e[1] - e[0]) / 1e3 for e in ev]
gap = [(b[1] - a[1]) / 1e3 for a, b in zip(ev, ev[1:])]
print("%s kernel duration (end - start stamp): median %.1f us  min %.1f  max %.1f" % (label, statistics.median(dur), min(dur), max(dur)))
print("%s end stamp to end stamp of consecutive launches (= time per product): median %.1f us  min %.1f  max %.1f; first start to last end / %d = %.1f us"
      % (label, statistics.median(gap), min(gap), max(gap), len(ev), (ev[-1][1] - min(e[0] for e in ev)) / 1e3 / len(ev)))
print("%s queues used by these launches: %s" % (label, sorted({e[3] for e in ev})))
