#!/usr/bin/env python3
"""Per-function diff of two device listings of the same source (hipcc ... --cuda-device-only -S -o x.s).

  python tools/isa_compare.py <a.s> <b.s> [symbol]

Per function (only `symbol` when given) one verdict:
  identical  the same instruction sequence once comments and directives are dropped and local labels (.LBB12_3 ...) are
             renumbered in order of appearance;
  reordered  the same multiset of instruction lines in another order: the differing positions are listed with both lines;
  different  with both instruction counts.
Per kernel it prints the register / spill / scratch / LDS / occupancy figures of both listings (the "Kernel info" comments and the
.amdgpu_metadata entry) and every .amdhsa_* descriptor value that differs (or how many agree).  It is a plain listing diff and
looks for no particular instruction.  Exit status 1 when any compared function is not identical.
"""
import collections
import re
import sys

INFO = {"NumVgprs": "VGPRs", "NumAgprs": "AGPRs", "TotalNumSgprs": "SGPRs", "ScratchSize": "scratch B/lane", "LDSByteSize": "LDS B",
        "Occupancy": "occupancy"}
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


class Func:
    def __init__(self):
        self.insts, self.desc, self.info, self.labels = [], {}, {}, {}

    def add(self, text):
        self.insts.append(LABEL.sub(lambda m: self.labels.setdefault(m.group(0), f".L{len(self.labels)}"), " ".join(text.split())))


def parse(path):
    funcs, types, cur, last = collections.OrderedDict(), set(), None, None
    meta_name, meta = None, {}
    for raw in open(path):
        s = raw.split(";")[0].strip() if not raw.lstrip().startswith(";") else ""
        m = re.match(r"\.type\s+([^,\s]+),@function", s)
        if m:
            types.add(m.group(1))
        elif cur is None and s.endswith(":") and s[:-1] in types:
            cur = last = funcs[s[:-1]] = Func()
        elif cur is not None and re.match(r"\.Lfunc_end\d+:", s):
            cur = None
        elif cur is not None and s.startswith(".amdhsa_") and " " in s:
            k, v = s.split(None, 1)
            if k != ".amdhsa_kernel":
                cur.desc[k] = v
        elif cur is not None and s and (s.endswith(":") or not s.startswith(".")):
            cur.add(s)
        elif cur is None and last is not None:  # "; NumVgprs: 128" ... behind the function, then the metadata entries at the end
            m = re.match(r";\s*(\w+)\s*:\s*(\d+)", raw.strip())
            if m and m.group(1) in INFO:
                last.info.setdefault(INFO[m.group(1)], m.group(2))
            m = re.match(r"    \.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", raw)
            if raw.startswith("  - ."):
                meta_name, meta = None, {}
            if m:
                meta[m.group(1)] = m.group(2)
                meta_name = meta.get("name")
            if meta_name in funcs and len(meta) == 3:
                funcs[meta_name].info.update({"SGPR spills": meta["sgpr_spill_count"], "VGPR spills": meta["vgpr_spill_count"]})
    return funcs


def verdict(a, b):
    if a.insts == b.insts:
        return "identical", []
    if collections.Counter(a.insts) == collections.Counter(b.insts):
        return "reordered", [f"      position {i}: `{x}` | `{y}`" for i, (x, y) in enumerate(zip(a.insts, b.insts)) if x != y]
    return "different", []


def main():
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    A, B = parse(sys.argv[1]), parse(sys.argv[2])
    only = sys.argv[3] if len(sys.argv) == 4 else None
    names = [n for n in A if only in (None, n)] + [n for n in B if n not in A and only in (None, n)]
    count = collections.Counter()
    for n in names:
        if n not in A or n not in B:
            print(f"{n}\n    only in {sys.argv[1] if n in A else sys.argv[2]}")
            count["different"] += 1
            continue
        a, b = A[n], B[n]
        v, where = verdict(a, b)
        count[v] += 1
        na, nb = (sum(1 for x in f.insts if not x.endswith(":")) for f in (a, b))
        print(f"{n}\n    {v}: instructions {na}" + ("" if v != "different" else f" | {nb}"))
        print("\n".join(where[:200] + ([f"      ... {len(where) - 200} more"] if len(where) > 200 else [])), end="\n" if where else "")
        if a.desc or b.desc:  # a kernel
            for tag, f in (("a", a), ("b", b)):
                print(f"    {tag}: " + "  ".join(f"{k} {val}" for k, val in f.info.items()))
            diff = [k for k in sorted(set(a.desc) | set(b.desc)) if a.desc.get(k) != b.desc.get(k)]
            print(f"    descriptor: {len(a.desc)} .amdhsa_* values, " + ("all equal" if not diff else "DIFFERENT: " +
                  ", ".join(f"{k} {a.desc.get(k)} | {b.desc.get(k)}" for k in diff)) + f"  (group_segment {a.desc.get('.amdhsa_group_segment_fixed_size')}"
                  f" private_segment {a.desc.get('.amdhsa_private_segment_fixed_size')} next_free_vgpr {a.desc.get('.amdhsa_next_free_vgpr')}"
                  f" next_free_sgpr {a.desc.get('.amdhsa_next_free_sgpr')} in a)")
    print(f"summary: {len(names)} functions: " + ", ".join(f"{count[k]} {k}" for k in ("identical", "reordered", "different")))
    sys.exit(0 if count["reordered"] + count["different"] == 0 else 1)


if __name__ == "__main__":
    main()
