"""Are the kernels of two builds of one source byte-identical?  

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <the file's flags of peekvit_amd/_build.py> [-DPV_OPERAND_F16] --cuda-device-only -S SRC -o before.s
    ... the same on the changed tree -o after.s
    python scripts/isa_compare.py before.s after.s

Compares the instruction text of every function present in `before` with its text in `after`, with what depends on a function's ordinal in the file
taken out: comments (they name basic blocks as BB<ordinal>_<n>) and the ordinal inside local labels.  Prints the functions that changed or vanished
and the functions that are new; exit status 1 if any function changed or vanished."""
import hashlib
import re
import sys


def kernels(path):
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", open(path).read(), flags=re.S | re.M):
        body = re.sub(r"\s*;.*", "", m.group(2))
        body = re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+", r".L\1N", body)
        out[m.group(1)] = hashlib.sha256(body.encode()).hexdigest()
    return out


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    changed = [k for k in before if before[k] != after.get(k)]
    new = [k for k in after if k not in before]
    print(f"{len(before)} functions before, {len(after)} after; changed or missing: {len(changed)}; new: {len(new)}")
    for k in changed:
        print("  changed", k)
    for k in new:
        print("  new    ", k)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
