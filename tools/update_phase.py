"""Medians over every step of a rocprofv3 --kernel-trace csv of the FFM headline run: the update
phase's span (the row kernel's end to the next refresh's start) and the durations of the launches
that run inside it.
usage: python tools/update_phase.py <trace dir>"""
import csv
import glob
import statistics
import sys


def main():
    fn = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    ev = []
    for r in csv.DictReader(open(fn)):
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    ev.sort()
    rows = [i for i, e in enumerate(ev) if e[2].startswith("ffm_row_kernel<true")]
    spans, steps, dur = [], [], {}
    for a, b in zip(rows, rows[1:]):
        nxt = [e for e in ev[a + 1:b] if e[2].startswith("ffm_refresh")]
        if not nxt:
            continue
        spans.append((nxt[-1][0] - ev[a][1]) / 1000.0)
        steps.append((ev[b][0] - ev[a][0]) / 1000.0)
        for s, e, n in ev[a + 1:b]:
            if n.startswith("ffm_update"):
                dur.setdefault(n[:40], []).append((e - s) / 1000.0)
    skip = len(spans) // 10  # (warm-up)
    print("steps %d  step us median %.1f  update phase span us median %.1f  (min %.1f max %.1f)" % (
        len(spans) - skip, statistics.median(steps[skip:]), statistics.median(spans[skip:]),
        min(spans[skip:]), max(spans[skip:])))
    for n in sorted(dur):
        print("  %-42s median %.1f us over %d launches" % (n, statistics.median(dur[n][skip:]), len(dur[n]) - skip))


if __name__ == "__main__":
    main()
