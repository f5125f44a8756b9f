#!/usr/bin/env python3
"""Two arms of one replayed training step side by side, kernel by kernel: durations from tools/rocpd_sequence.py's output of each arm,
bytes from tools/pmc_step_traffic.py's table of each arm (the layout of profiles/store_policy_step_sequence.txt).

usage: tools/step_sequence_ab.py <seq_parent.txt> <seq_branch.txt> <pmc_parent.json> <pmc_branch.json>"""
import json
import sys


def sequence(path):
    rows, notes = [], []
    for line in open(path):
        if line.startswith("#"):
            notes.append(line.strip()[2:])
        elif line.strip() and line.strip()[0].isdigit():
            w = line.split()                          # "<i> <kernel> blocks <n> dur <us> us  gap <us> us"
            rows.append((w[1], int(w[3]), float(w[5])))
    return rows, notes


def main():
    (sa, na), (sb, nb) = sequence(sys.argv[1]), sequence(sys.argv[2])
    pa, pb = (json.load(open(p))["sequence"] for p in sys.argv[3:5])
    assert [r[:2] for r in sa] == [r[:2] for r in sb], "the two arms ran different kernel sequences"
    for p in (pa, pb):
        assert [(e["kernel"], e["workgroups"]) for e in p] == [r[:2] for r in sa], "counter passes and trace saw different kernel sequences"
    print("#  i kernel                      blocks | dur us parent  branch   diff | written MB parent branch   diff | fetched MB parent branch   diff")
    tot = [0.0] * 6
    for i, ((k, g, da), (_, _, db), ea, eb) in enumerate(zip(sa, sb, pa, pb)):
        wa, wb, fa, fb = ea["write_MB"], eb["write_MB"], ea["fetch_MB_x2"], eb["fetch_MB_x2"]
        for j, v in enumerate((da, db, wa, wb, fa, fb)):
            tot[j] += v
        print(f"{i:4d} {k:27s} {g:6d} | {da:8.2f} {db:8.2f} {db - da:+7.2f} | {wa:10.2f} {wb:8.2f} {wb - wa:+7.2f} | {fa:10.2f} {fb:8.2f} {fb - fa:+7.2f}")
    print(f"# sums: durations {tot[0]:.1f} -> {tot[1]:.1f} us, written {tot[2]:.1f} -> {tot[3]:.1f} MB, fetched {tot[4]:.1f} -> {tot[5]:.1f} MB")
    for arm, notes in (("parent", na), ("branch", nb)):
        for n in notes:
            print(f"# {arm}: {n}")


if __name__ == "__main__":
    main()
