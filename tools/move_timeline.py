#!/usr/bin/env python3
"""Diagnostic: where a self-play move's wall time goes, from a rocprofv3 kernel trace of the resnet headline.
    python3 tools/move_timeline.py <kernel_trace.csv> [moves in the window]
Window: from the first network kernel (k_tower* / k_heads*) to the last one of the trace (warm-up and timed moves of
the headline; the settle run before it plays on k_play and is left out).  Over that window the wall time is split into
  net      at least one network kernel on the device (the matrix pipe has tower or heads work),
  search   no network kernel, but a tree kernel (k_mcts / k_choose / k_advance) or a fill,
  gap      nothing on the device at all.
Also printed: per-kernel launch counts and mean durations, and how much of the summed network device time ran while
another network launch was on the device too (summed launch time over the union: 1.0 on one stream, up to 2 with two
half-pools on two streams).  For the pipelined loop two more blocks: the wall time with 0, 1 and 2
k_tower_f16x3_s16 launches in flight, and per phase how long after half A's tower half B's starts, as a fraction of A's
phase period (near 0 or 1: the halves' towers start and end together; around 0.5: one half's tail, heads and tree launch
fall into the middle of the other half's tower), over the window and move by move (a move ends with half A's k_advance)."""
import bisect
import collections
import csv
import sys


def kind(name):
    if "k_tower" in name or "k_heads" in name or "k_stem" in name or "k_conv" in name:
        return "net"
    if any(k in name for k in ("k_mcts", "k_choose", "k_advance", "k_play", "k_reset", "k_gather")):
        return "tree"
    return "other"


def union(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def length(iv):
    return sum(b - a for a, b in iv)


def intersect(x, y):
    i = j = 0
    out = []
    while i < len(x) and j < len(y):
        a, b = max(x[i][0], y[j][0]), min(x[i][1], y[j][1])
        if a < b:
            out.append([a, b])
        if x[i][1] < y[j][1]:
            i += 1
        else:
            j += 1
    return out


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows]
    net = [(a, b) for a, b, n in ev if kind(n) == "net"]
    if not net:
        raise SystemExit("no network kernels in the trace")
    t0, t1 = min(a for a, _ in net), max(b for _, b in net)
    ev = [(max(a, t0), min(b, t1), n) for a, b, n in ev if b > t0 and a < t1]
    wall = t1 - t0
    net_u = union([(a, b) for a, b, n in ev if kind(n) == "net"])
    any_u = union([(a, b) for a, b, n in ev])
    busy_net, busy_any = length(net_u), length(any_u)
    ms = lambda ns: ns / 1e6
    if len(sys.argv) > 2:
        moves = int(sys.argv[2])
        print("window %.3f ms, %d moves: %.3f ms per move" % (ms(wall), moves, ms(wall) / max(1, moves)))
    else:   # k_choose runs once per move on one stream, once per half-pool per move when pipelined
        print("window %.3f ms, %d k_choose launches" % (ms(wall), sum(1 for _, _, n in ev if "k_choose" in n)))
    print("  net     %8.3f ms  %6.2f %%" % (ms(busy_net), 100.0 * busy_net / wall))
    print("  search  %8.3f ms  %6.2f %%" % (ms(busy_any - busy_net), 100.0 * (busy_any - busy_net) / wall))
    print("  gap     %8.3f ms  %6.2f %%" % (ms(wall - busy_any), 100.0 * (wall - busy_any) / wall))
    # network launches overlapping each other (two halves on two streams)
    by_start = sorted((a, b) for a, b, n in ev if kind(n) == "net")
    summed = sum(b - a for a, b in by_start)
    print("  net device time summed over launches %.3f ms (%.3f x the union)" % (ms(summed), summed / max(1, busy_net)))
    tree_u = union([(a, b) for a, b, n in ev if kind(n) == "tree"])
    print("  tree kernels %.3f ms of union, %.3f ms of it under a network kernel" %
          (ms(length(tree_u)), ms(length(intersect(tree_u, net_u)))))
    per = collections.defaultdict(list)
    for a, b, n in ev:
        per[n.split("(")[0][:60]].append(b - a)
    for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s %6d launches  mean %8.4f ms  sum %9.3f ms" % (n, len(v), ms(sum(v)) / len(v), ms(sum(v))))
    towers_in_flight(rows, t0, t1)


TOWER = "k_tower_f16x3_s16"


def towers_in_flight(rows, t0, t1):
    """How many TOWER launches are on the device at once, and how far apart the two half-pools' towers start."""
    ms = lambda ns: ns / 1e6
    tw = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id") or r.get("Stream_Id") or "0",
           int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)) for r in rows if TOWER in r["Kernel_Name"]]
    tw = [(max(a, t0), min(b, t1), q, g) for a, b, q, g in tw if b > t0 and a < t1]
    if not tw:
        return
    wall = t1 - t0
    # sweep: wall time by the number of tower launches in flight
    edges = sorted([(a, 1) for a, _, _, _ in tw] + [(b, -1) for _, b, _, _ in tw])
    by_n = collections.defaultdict(int)
    depth, last = 0, t0
    for t, step in edges:
        by_n[depth] += t - last
        depth, last = depth + step, t
    by_n[0] += t1 - last
    print("  %s launches in flight (wall time of the window):" % TOWER)
    for n in sorted(by_n):
        print("    %d in flight %9.3f ms  %6.2f %%" % (n, ms(by_n[n]), 100.0 * by_n[n] / wall))
    # phases: a half-pool's full tower launches.  Left out: a call's first evaluation cut in two (smaller grids) and
    # the launches behind a BEGIN phase, which find (almost) no rows and return at once.
    queues = collections.defaultdict(list)
    for a, b, q, g in tw:
        queues[q].append((a, b, g))
    if len(queues) < 2:
        print("  one queue runs every tower launch: no half-pool offset")
        return
    qa, qb = sorted(sorted(queues, key=lambda q: -len(queues[q]))[:2], key=lambda q: min(queues[q])[0])

    def phases(q):
        v = sorted(queues[q])
        grid = collections.Counter(g for _, _, g in v).most_common(1)[0][0]
        dur = sorted(b - a for a, b, _ in v)[len(v) // 2]
        return [a for a, b, g in v if g == grid and b - a >= 0.1 * dur]

    pa, pb = phases(qa), phases(qb)
    fr = []
    j = 0
    for i in range(len(pa) - 1):
        while j < len(pb) and pb[j] < pa[i]:
            j += 1
        if j < len(pb) and pb[j] < pa[i + 1]:
            fr.append((pa[i], (pb[j] - pa[i]) / float(pa[i + 1] - pa[i])))
    if not fr:
        print("  no phase holds a tower start of each half-pool")
        return
    med = lambda v: sorted(v)[len(v) // 2]
    at, fr = [t for t, _ in fr], [f for _, f in fr]
    print("  half B's tower start after half A's, as a fraction of A's phase period (%d phases, median period %.3f ms):"
          % (len(fr), ms(med([pa[i + 1] - pa[i] for i in range(len(pa) - 1)]))))
    print("    min %.3f  median %.3f  max %.3f" % (min(fr), med(fr), max(fr)))
    print("    phases with the offset inside 0.25-0.75: %d of %d" % (sum(1 for f in fr if 0.25 <= f <= 0.75), len(fr)))
    # drift: the same figures move by move; half A's k_advance launches are the move boundaries
    ends = sorted(int(r["Start_Timestamp"]) for r in rows if "k_advance" in r["Kernel_Name"] and
                  (r.get("Queue_Id") or r.get("Stream_Id") or "0") == qa and t0 < int(r["Start_Timestamp"]) < t1)
    by_move = collections.defaultdict(list)
    for t, f in zip(at, fr):
        by_move[bisect.bisect_left(ends, t)].append(f)
    for m in sorted(by_move):
        c = by_move[m]
        print("    move %2d (%2d phases): first %.3f  min %.3f  median %.3f  max %.3f" % (m, len(c), c[0], min(c), med(c), max(c)))


if __name__ == "__main__":
    main()
