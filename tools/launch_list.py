"""The ordered launches of a run, from a `rocprofv3 --kernel-trace --output-format csv` kernel trace: one line per dispatch, in dispatch order,
`kernel name | grid x,y,z | workgroup x,y,z`.  Two runs of one program that enqueue the same work give the same list whatever the clock did.

  python tools/launch_list.py list  <kernel_trace.csv> [out.txt]
  python tools/launch_list.py diff  <a_kernel_trace.csv> <b_kernel_trace.csv>      exit status 1 and the first differing lines when the lists differ"""
import csv
import sys


def launches(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        return []
    col = {k.lower(): k for k in rows[0]}
    order = col.get("dispatch_id") or col["start_timestamp"]
    rows.sort(key=lambda r: int(r[order]))
    dims = lambda r, what: ",".join(r[col[f"{what}_size_{a}"]] for a in "xyz")
    return [f"{r[col['kernel_name']]} | {dims(r, 'grid')} | {dims(r, 'workgroup')}" for r in rows]


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "list":
        out = "\n".join(launches(sys.argv[2])) + "\n"
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(out)
        else:
            sys.stdout.write(out)
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "diff":
        a, b = launches(sys.argv[2]), launches(sys.argv[3])
        if a == b:
            print(f"equal: {len(a)} launches")
            return 0
        print(f"DIFFERENT: {len(a)} vs {len(b)} launches")
        shown = 0
        for i in range(max(len(a), len(b))):
            x, y = a[i] if i < len(a) else "-", b[i] if i < len(b) else "-"
            if x != y:
                print(f"  #{i}\n    a: {x}\n    b: {y}")
                shown += 1
                if shown == 5:
                    break
        return 1
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
