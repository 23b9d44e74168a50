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
half-pools on two streams)."""
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


if __name__ == "__main__":
    main()
