"""Per-kernel resource usage from a compile log with -Rpass-analysis=kernel-resource-usage, as a markdown table or as a
comparison of two logs.  Kernels are keyed by their demangled name -- template arguments spelled out, defaulted trailing
`false` / `0` arguments dropped -- so that a template parameter added with a default does not turn every row into a new one.

    hipcc ... -Rpass-analysis=kernel-resource-usage --cuda-device-only -c -o /dev/null unit.hip 2> log.txt
    python tools/resource_table.py log.txt [--only decode_frames_kernel]
    python tools/resource_table.py --compare before.txt after.txt
"""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
SHORT = ["SGPRs", "VGPRs", "AGPRs", "scratch", "occupancy", "SGPR spill", "VGPR spill", "LDS"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def key_of(demangled):
    """`void fa::k<8, -1, false, 1, false, true>(args)` -> `k<8, -1, false, 1, false, true>`, trailing `, false` and `, 0` dropped."""
    m = re.match(r"(?:void )?(?:fa::)?([\w:]+)(<.*>)?\(", demangled)
    if not m:
        return demangled
    name, targs = m.group(1), m.group(2) or ""
    if targs:
        parts = [p.strip() for p in targs[1:-1].split(",")]
        while len(parts) > 1 and parts[-1] in ("false", "0"):  # (defaults of added parameters: `bool X = false`, `int X = 0`)
            parts.pop()
        targs = "<" + ", ".join(parts) + ">"
    return name + targs


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = m.group(2)
    names = demangle(list(rows))
    return {key_of(names[k]): v for k, v in rows.items()}


def table(rows, only=None):
    out = ["| kernel | " + " | ".join(SHORT) + " |", "|---|" + "---:|" * len(SHORT)]
    for k in sorted(rows):
        if only and only not in k:
            continue
        out.append("| `%s` | " % k + " | ".join(rows[k].get(f, "?") for f in FIELDS) + " |")
    return "\n".join(out)


def compare(a, b):
    changed = [k for k in sorted(a) if k in b and a[k] != b[k]]
    gone = [k for k in sorted(a) if k not in b]
    new = [k for k in sorted(b) if k not in a]
    print("kernels before: %d, after: %d, unchanged: %d" % (len(a), len(b), len([k for k in a if k in b and a[k] == b[k]])))
    for k in changed:
        print("CHANGED %s\n  before %s\n  after  %s" % (k, a[k], b[k]))
    for k in gone:
        print("GONE    %s" % k)
    for k in new:
        print("NEW     %s" % k)
    return not changed and not gone


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        sys.exit(0 if compare(parse(args[1]), parse(args[2])) else 1)
    only = args[args.index("--only") + 1] if "--only" in args else None
    print(table(parse(args[0]), only))
