"""K5 of a registered AIR program (csrc/air_program.hip, quotient_program_kernel) next to the compiled kernel of the
built-in AIR it transcribes (quotient_air_kernel<4> at 2^16 rows, <7> at 2^14), on the same random LDE matrices,
launches alternating.
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/air_program_k5_probe.py
  python tools/air_program_k5_probe.py --summary OUT      medians per kernel from the trace, the two ratios
  rocprofv3 --pmc <counters> --output-format csv -d OUT2 -- python tools/air_program_k5_probe.py --counters
  python tools/air_program_k5_probe.py --counter-summary OUT2 [OUT3 ...]   per kernel and launch, the counters' values
(profiles/air_program_k5.txt is that summary).  The transcriptions are the tests' (tests/air_program_cases.py)."""
import glob, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CASES = [("arithmetic", 4, 16), ("arithmetic_mul", 7, 14)]
LAUNCHES = 20


def summary(out_dir):
    import csv
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    times = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if "quotient_air_kernel" in k or "quotient_program_kernel" in k or "quotient_sum_kernel" in k:
                key = (k.replace("(anonymous namespace)::", "").split("(")[0], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0),
                       int(r.get("Grid_Size_Y") or 1), int(r.get("LDS_Block_Size") or 0))
                times.setdefault(key, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    print("# per-launch kernel time in microseconds; grid in work-items (256 per workgroup); the first launch of each (warm-up) dropped")
    med = {}
    for key in sorted(times, key=lambda k: (k[1], k[0])):
        t = times[key][1:] if len(times[key]) > 2 else times[key]
        med[key] = statistics.median(t)
        print("%-34s grid=(%d,%d) lds=%-6d launches %2d  median %9.1f  min %9.1f  max %9.1f" %
              (key[0], key[1], key[2], key[3], len(t), med[key], min(t), max(t)))
    for rows in sorted({k[1] for k in med}):
        prog = [v for k, v in med.items() if k[1] == rows and "program" in k[0]]
        built = [v for k, v in med.items() if k[1] == rows and "quotient_air_kernel" in k[0]]
        if prog and built:
            print("ratio interpreted / compiled at %d points: %.2f" % (rows, prog[0] / built[0]))


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, air, log_n in CASES:
        b = getattr(cases, name + "_program")()
        words = b.assemble()
        reg = bpg.ops.air_register(words)
        d = bpg.ops.air_describe(air)
        rows = (1 << log_n) << 1
        tr = torch.randint(0, 2**62, (d.n_cols, rows), dtype=torch.int64, device="cuda", generator=g)
        aux = torch.randint(0, 2**62, (1, rows), dtype=torch.int64, device="cuda", generator=g)
        cfg = bpg.ops.stark_cfg(log_n, d.n_cols)
        ops = {}
        for w in words[10 + 4 * int(words[6]) + int(words[8]) + 1:]:
            ops[int(w) & 0xFF] = ops.get(int(w) & 0xFF, 0) + 1      # (an imm's constant word is counted by its low byte: few)
        print("%s: air %d / program 0x%08x, 2^%d rows, %d points, %d code words, n_regs %d, op counts %s" %
              (name, air, reg, log_n, rows, int(words[9]), int(words[7]), dict(sorted(ops.items()))), flush=True)
        outs = {}
        for _ in range(2 if "--counters" in sys.argv else LAUNCHES + 1):
            for a in (air, reg):
                outs[a] = bpg.ops.quotient_eval(cfg, tr, aux, None, (3, 5, 7, 11), (13, 17), air_id=a)
            torch.cuda.synchronize()
        assert bool((outs[air] == outs[reg]).all())
        del tr, aux


def counter_summary(dirs):
    import csv
    acc = {}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                k = r["Kernel_Name"]
                if "quotient_air_kernel" in k or "quotient_program_kernel" in k:
                    key = (k.replace("(anonymous namespace)::", "").split("(")[0], int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0))
                    a = acc.setdefault(key, {})
                    a.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    print("# per launch (mean over the launches of the pass), summed over the chip's SQs")
    for key in sorted(acc, key=lambda k: (k[1], k[0])):
        print("%-30s grid_x=%-7d %s" % (key[0], key[1], "  ".join("%s=%.4g" % (c, sum(v) / len(v)) for c, v in sorted(acc[key].items()))))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--counter-summary":
        counter_summary(sys.argv[2:])
    else:
        main()
