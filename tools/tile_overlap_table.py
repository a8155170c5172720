"""rocprofv3 --kernel-trace CSV of a bench.py run -> durations of the step kernels (kick+drift, gradient op), split by which
side-stream kernel (generator, momentum refresh) they overlap; the gaps between step kernels: tile_overlap_table.py TRACE.csv"""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
cols = rows[0].keys()
name_c = next(c for c in cols if c.lower() in ("kernel_name", "name"))
s_c = next(c for c in cols if c.lower().startswith("start"))
e_c = next(c for c in cols if c.lower().startswith("end"))
ks = [(r[name_c], int(r[s_c]), int(r[e_c])) for r in rows]
ks.sort(key=lambda k: k[1])
side = [k for k in ks if "k_zig_parallel" in k[0] or "k_refresh_apply" in k[0] or "k_log_uniform" in k[0]]


def is_step(n):
    """The in-place pair of a resident tile: the per-access-policy kernels, or the plain ones of older builds."""
    return any(k in n for k in ("k_kick_drift_tile", "k_gauss_grad_tile", "k_kick_drift_v2", "k_gauss_grad_v2"))


def short(n):
    n = n.replace("void ", "").replace("(anonymous namespace)::", "")
    return n.split("(")[0]


# only the steady state: the last 60 % of the trace
t0 = ks[0][1] + 0.4 * (ks[-1][2] - ks[0][1])
groups = {}
for n, s, e in ks:
    if s < t0 or not is_step(n):
        continue
    ov = "alone"
    for sn, ss, se in side:
        if ss < e and se > s:
            ov = "beside " + short(sn)
            break
    groups.setdefault((short(n), ov), []).append((e - s) / 1e3)
for (n, ov), d in sorted(groups.items()):
    d.sort()
    print(f"OVERLAP {n:40s} {ov:40s} n={len(d):6d} median {statistics.median(d):8.2f} us  mean {statistics.fmean(d):8.2f}  "
          f"p10 {d[len(d) // 10]:8.2f}  p90 {d[9 * len(d) // 10]:8.2f}")
for sn in sorted({short(k[0]) for k in side}):
    d = [(e - s) / 1e3 for n, s, e in side if short(n) == sn and s >= t0]
    if d:
        print(f"SIDE {sn:40s} n={len(d):5d} median {statistics.median(d):9.2f} us")
# gaps: idle time between consecutive main-stream step kernels
main = [k for k in ks if k[1] >= t0 and k not in side]
busy = sum(e - s for _, s, e in main)
span = main[-1][2] - main[0][1]
print(f"MAIN kernels {len(main)}, busy {busy / 1e6:.2f} ms of span {span / 1e6:.2f} ms")
# gaps between consecutive step kernels (both tile-sized), in launch order
steps = [k for k in main if is_step(k[0])]
gaps = sorted((steps[i + 1][1] - steps[i][2]) / 1e3 for i in range(len(steps) - 1) if steps[i + 1][1] - steps[i][2] < 200e3)
n = len(gaps)
print(f"GAPS between step kernels n={n}: median {gaps[n // 2]:.2f} us  mean {sum(gaps) / n:.2f}  p10 {gaps[n // 10]:.2f}  p90 {gaps[9 * n // 10]:.2f}  "
      f"p99 {gaps[99 * n // 100]:.2f}  sum {sum(gaps) / 1e3:.2f} ms")
