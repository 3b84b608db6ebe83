"""Compare the code generated for every kernel of two trees: `codegen_table.py OLD_DIR NEW_DIR [old=new ...]`.
Each directory holds the device assembly of the kernel sources (hipcc -S --cuda-device-only with the flags of
`make -C csrc print-hip-flags`, as tests/test_build.py builds it).  Per kernel: VGPRs, SGPRs, scratch bytes, static
LDS bytes, instructions.  `old=new` pairs are regular-expression renames applied to the OLD tree's demangled names
(a template parameter that went away).  Prints one line per kernel -- same, DIFFERS, or on one side only -- and the
count of identical ones; exit status 1 if a kernel present in both differs."""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("lds", ".group_segment_fixed_size"))


def kernels(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = open(path).read()
        meta = text[text.index("amdhsa.kernels:"):]
        for entry in re.split(r"\n  - (?=\.agpr_count)", meta)[1:]:
            sym = re.search(r"\.symbol:\s+'?([^\s']+?)\.kd'?\s", entry).group(1)
            row = {k: int(re.search(re.escape(f) + r":\s+(\d+)", entry).group(1)) for k, f in FIELDS}
            body = text[text.index("\n%s:" % sym):]
            body = body[:body.index(".Lfunc_end")]
            row["insts"] = len(re.findall(r"^\s+(?:[sv]_|ds_|global_|buffer_|flat_|scratch_)", body, flags=re.M))
            out[sym] = row
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    return {re.sub(r"^void |\(.*$", "", n.replace("(anonymous namespace)::", "")): row for n, row in zip(names, out.values())}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for pair in sys.argv[3:]:
        a, b = pair.split("=", 1)
        old = {re.sub(a, b, n): row for n, row in old.items()}
    same = differ = 0
    cols = [k for k, _ in FIELDS] + ["insts"]
    print("%-70s %s" % ("kernel", "  ".join("%14s" % c for c in cols)))
    for n in sorted(set(old) | set(new)):
        cell = lambda r, c: "-" if r is None else str(r[c])
        if n in old and n in new and old[n] == new[n]:
            same += 1
            print("%-70s %s  same" % (n[:70], "  ".join("%14s" % cell(new[n], c) for c in cols)))
            continue
        differ += n in old and n in new
        print("%-70s %s  %s" % (n[:70], "  ".join("%14s" % ("%s -> %s" % (cell(old.get(n), c), cell(new.get(n), c))) for c in cols),
                                "DIFFERS" if n in old and n in new else ("only in old" if n in old else "only in new")))
    print("%d kernels in both trees with identical %s; %d differ" % (same, ", ".join(cols), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
