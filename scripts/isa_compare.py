"""Are the kernels of two builds of one source byte-identical?  (DESIGN.md sections 33, 34.)

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <the file's flags of peekvit_amd/_build.py> [-DPV_OPERAND_F16] --cuda-device-only -S SRC -o before.s
    ... the same on the changed tree -o after.s
    python scripts/isa_compare.py [--stats] before.s after.s

Compares the instruction text of every function present in `before` with its text in `after`, with what depends on a function's ordinal in the file
taken out: comments (they name basic blocks as BB<ordinal>_<n>) and the ordinal inside local labels.  Prints the functions that changed or vanished
and the functions that are new; exit status 1 if any function changed or vanished.

--stats: for every changed function that exists on both sides, one table row with the instruction count, the MFMA count and the kernel descriptor's
next_free_vgpr, next_free_sgpr, group_segment_fixed_size (LDS bytes) and private_segment_fixed_size (scratch bytes), before -> after."""
import hashlib
import re
import subprocess
import sys

DESC = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path, stats=None):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        body = re.sub(r"\s*;.*", "", m.group(2))
        body = re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+", r".L\1N", body)
        out[m.group(1)] = hashlib.sha256(body.encode()).hexdigest()
        if stats is not None:
            # an instruction: an indented line that is neither a label nor a directive
            insts = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and ln.strip() and not ln.strip().startswith(".")]
            stats[m.group(1)] = {"instructions": len(insts), "mfma": sum(1 for i in insts if i.startswith("v_mfma"))}
    if stats is not None:
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M):
            if m.group(1) in stats:
                for key in DESC:
                    stats[m.group(1)][key] = int(re.search(rf"\.amdhsa_{key} (\d+)", m.group(2)).group(1))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (s.split("(")[0].replace("void ", "") for s in r.stdout.split("\n"))))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    args = [a for a in sys.argv[1:] if a != "--stats"]
    want_stats = "--stats" in sys.argv[1:]
    sb, sa = ({}, {}) if want_stats else (None, None)
    before, after = kernels(args[0], sb), kernels(args[1], sa)
    changed = [k for k in before if before[k] != after.get(k)]
    new = [k for k in after if k not in before]
    print(f"{len(before)} functions before, {len(after)} after; changed or missing: {len(changed)}; new: {len(new)}")
    for k in changed:
        print("  changed", k)
    for k in new:
        print("  new    ", k)
    both = [k for k in changed if k in after]
    if want_stats and both:
        names = demangle(both)
        print("\n| function | instructions | MFMA | next_free_vgpr | next_free_sgpr | LDS bytes | scratch bytes |")
        print("|---|---|---|---|---|---|---|")
        for k in both:
            b, a = sb[k], sa[k]
            cell = lambda key: f"{b.get(key, '-')} -> {a.get(key, '-')}" if b.get(key) != a.get(key) else f"{b.get(key, '-')}"
            print(f"| `{names[k]}` | {b['instructions']} -> {a['instructions']} ({(a['instructions'] / b['instructions'] - 1) * 100:+.2f} %) | {cell('mfma')} | "
                  + " | ".join(cell(key) for key in DESC) + " |")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
