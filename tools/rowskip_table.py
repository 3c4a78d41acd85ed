"""The 3x3 conv_igemm_p8 launches of one scoring chunk, CBW_P8_ROWSKIP off against on (and optionally a third pass, e.g.
CBW_P8_ROWGROUP at flat), from rocprofv3 --pmc FETCH_SIZE passes of bench.py (counter passes serialise the kernels):
per layer the isolated duration, the saving beside the layer's share of all-padding K-tiles, and the fetched bytes
(fabric side: FETCH_SIZE x 2 KB on gfx950).  Medians over the whole chunks of one queue.
usage: python tools/rowskip_table.py PAIRS OFF_DIR ON_DIR [THIRD_DIR]   (PAIRS = bench.py --chunk of the passes)"""
import collections
import csv
import glob
import gzip
import re
import sys

NAMES = ["s2b0 3x3s2", "s2b1 3x3", "s2b2 3x3", "s2b3 3x3", "s3b0 3x3s2", "s3b1 3x3", "s3b2 3x3", "s3b3 3x3", "s3b4 3x3",
         "s3b5 3x3", "s4b0 3x3s2", "s4b1 3x3", "s4b2 3x3"]
# K-tiles that read only padding rows: 2 of 3 Ho (kernel row, output row) pairs; s3b0 (in 10 -> out 5): the top row only
SHARE = {"s2": 2 / 30, "s3b0": 1 / 15, "s3": 2 / 15, "s4": 2 / 9}


def chunks(d):
    f = (glob.glob(f"{d}/**/*counter_collection.csv*", recursive=True) or [d])[0]
    disp = {}
    for r in csv.DictReader(gzip.open(f, "rt") if f.endswith(".gz") else open(f)):
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void ", "")
        disp[int(r["Dispatch_Id"])] = (r["Queue_Id"], name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3,
                                       float(r["Counter_Value"]) * 2048 / 1e6)
    byq = collections.defaultdict(list)
    for k in sorted(disp):
        byq[disp[k][0]].append(disp[k])
    for launches in byq.values():
        st = [i for i, x in enumerate(launches) if x[1].startswith("stem_pool")]
        if len(st) < 4:
            continue
        ch = [launches[st[i]:st[i + 1]] for i in range(1, len(st) - 1)]   # the first chunk warms up, the last is open
        n = collections.Counter(len(c) for c in ch).most_common(1)[0][0]
        return [c for c in ch if len(c) == n]
    raise SystemExit(f"{d}: no queue with whole chunks")


def med(v):
    return sorted(v)[len(v) // 2]


def table(d):
    ch = chunks(d)
    idx = [i for i, x in enumerate(ch[0]) if x[1].startswith("conv_igemm_p8<3, 3")]
    rows = [(name, ch[0][i][1], med([c[i][2] for c in ch]), med([c[i][3] for c in ch])) for name, i in zip(NAMES, idx)]
    return rows, med([sum(x[2] for x in c) for c in ch]), len(ch), len(ch[0])


pairs, dirs = sys.argv[1], sys.argv[2:]
T = [table(d) for d in dirs]
third = len(T) > 2
print(f"one {pairs}-pair chunk, isolated launches: median over {T[0][2]} whole chunks of one queue, {T[0][3]} launches each")
print(f"{'layer':11s} {'kernel':26s} {'off us':>8s} {'on us':>8s} {'saved':>7s} {'K share':>8s} {'off MB':>8s} {'on MB':>8s}"
      + (f" {'3rd us':>8s} {'3rd MB':>8s}" if third else ""))
tot = [0.0] * len(T)
for i, (name, k, d0, f0) in enumerate(T[0][0]):
    share = SHARE["s3b0"] if name.startswith("s3b0") else SHARE[name[:2]]
    d1, f1 = T[1][0][i][2:]
    line = f"{name:11s} {k:26s} {d0:8.1f} {d1:8.1f} {100 * (d0 - d1) / d0:6.1f}% {100 * share:7.1f}% {f0:8.1f} {f1:8.1f}"
    if third:
        line += f" {T[2][0][i][2]:8.1f} {T[2][0][i][3]:8.1f}"
    for j in range(len(T)):
        tot[j] += T[j][0][i][2]
    print(line)
for label, v in (("3x3 total", tot), ("chunk total", [t[1] for t in T])):
    print(f"{label:38s} {v[0]:8.1f} {v[1]:8.1f} {100 * (v[0] - v[1]) / v[0]:6.1f}%" + (f"{'':27s}{v[2]:8.1f}" if third else ""))
