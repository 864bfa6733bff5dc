"""Compare two device assemblies of the library kernel by kernel, instruction for instruction (no GPU needed).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --offload-device-only -S direct_lidar_odometry_amd/csrc/ngicp_api.hip -o new.s
  (the same on a checkout of the commit to compare with -> old.s)
  python scripts/kernel_asm_diff.py old.s new.s [--alias 'NEW NAME=OLD NAME' ...]

Per function of old.s: identical, or the lines that differ.  Directives and comments are dropped; block labels (.LBB<n>_) and mangled
names inside operands are normalised, since both change when a function is added elsewhere in the file.  Functions are matched by
demangled name; --alias maps the name a kernel has in new.s to its name in old.s (a template parameter added with a default changes
the mangled name and nothing else).  Functions only in new.s are listed with their instruction counts.
"""
import argparse
import difflib
import re
import subprocess


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_]\w*):\s*(;.*)?$", line)
        if m and name is None and (m.group(1).startswith("_Z") or m.group(1).startswith("k_")):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", t)))
    return out


def demangled(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--alias", action="append", default=[], help="'NEW NAME=OLD NAME' (substrings of demangled names)")
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    dn_old, dn_new = demangled(list(old)), demangled(list(new))
    by_name = {}
    for k, v in new.items():
        n = dn_new[k]
        for al in a.alias:
            src, dst = al.split("=", 1)
            n = n.replace(src, dst)
        by_name[n] = v
    same = 0
    seen = set()
    for k, v in sorted(old.items(), key=lambda kv: dn_old[kv[0]]):
        n = dn_old[k]
        seen.add(n)
        if n not in by_name:
            print(f"MISSING in new: {n}")
        elif by_name[n] == v:
            same += 1
        else:
            d = [x for x in difflib.unified_diff(v, by_name[n], lineterm="", n=0) if not x.startswith(("---", "+++", "@@"))]
            print(f"DIFFERS {n}: {len(v)} -> {len(by_name[n])} instructions, {len(d)} changed lines")
            print("\n".join("    " + x for x in d[:40]))
    print(f"{same} of {len(old)} functions identical")
    for n, v in sorted(by_name.items()):
        if n not in seen:
            print(f"NEW {n}: {len(v)} instructions")


if __name__ == "__main__":
    main()
