"""An interpreted lookup port next to the compiled one: the memory table (AIR 3) at 2^17 rows proven under its built-in id
and under the registered transcription whose lookup is a port (tests/air_program_port_cases.py, memory_port_program),
from the same trace, proofs alternating.  Per proof the auxiliary witness is aux_suffix_product_kernel<3> for the
built-in and program_port_terms_kernel + aux_suffix_product_kernel<9> (the term read from the column) for the program;
K5 is quotient_air_kernel<3> against quotient_program_kernel<true>.
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/air_program_ports_probe.py
  python tools/air_program_ports_probe.py --summary OUT      medians per kernel from the trace, the two ratios
(profiles/air_program_ports.txt is that summary)."""
import glob, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LOG_N = 17
PROOFS = 20
KERNELS = ("aux_suffix_product_kernel", "program_port_terms_kernel", "quotient_air_kernel", "quotient_program_kernel", "quotient_sum_kernel")


def summary(out_dir):
    import csv
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    times = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if any(name in k for name in KERNELS):
                key = (k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0),
                       int(r.get("Grid_Size_Y") or 1))
                times.setdefault(key, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    print("# per-launch kernel time in microseconds; grid in work-items; the first launch of each (warm-up) dropped")
    med = {}
    for key in sorted(times):
        t = times[key][1:] if len(times[key]) > 2 else times[key]
        med[key[0]] = statistics.median(t)
        print("%-44s grid=(%d,%d)  launches %2d  median %9.1f  min %9.1f  max %9.1f" % (key[0], key[1], key[2], len(t), med[key[0]], min(t), max(t)))
    pick = lambda part: next(v for k, v in med.items() if part in k)
    port = pick("program_port_terms_kernel") + pick("aux_suffix_product_kernel<9")
    print("auxiliary witness, interpreted port (terms + scan) / compiled (aux_suffix_product_kernel<3>): %.1f / %.1f us = %.2f"
          % (port, pick("aux_suffix_product_kernel<3"), port / pick("aux_suffix_product_kernel<3")))
    print("K5, quotient_program_kernel<true> / quotient_air_kernel<3>: %.1f / %.1f us = %.2f"
          % (pick("quotient_program_kernel"), pick("quotient_air_kernel<3"), pick("quotient_program_kernel") / pick("quotient_air_kernel<3")))


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    import air_program_port_cases as pc
    words = pc.memory_port_program().assemble()
    reg = bpg.ops.air_register(words)
    trace = bpg.ops.memory_trace(LOG_N, seed=0x17)
    g = torch.Generator(device="cuda").manual_seed(1)
    trace[pc.MEM_G] = (torch.randint(0, 3, (1 << LOG_N,), device="cuda", generator=g) == 0).to(torch.int64)
    cfg = cases.cfg_for(3, LOG_N)
    print("memory: air 3 / program 0x%08x, 2^%d rows, %d code words (port unit: %d), n_regs %d" %
          (reg, LOG_N, int(words[9]), int(words[9]) - int(words[11 + 4 * int(words[6]) + 1 + 1]), int(words[7])), flush=True)
    proofs = {}
    for _ in range(PROOFS + 1):
        for a in (3, reg):
            proofs[a] = bpg.ops.stark_prove_trace(a, cfg, trace)
    diff = (proofs[3] != proofs[reg]).nonzero()[0].tolist()
    assert diff == [14], diff[:8]


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
