"""What the run-time stack costs on a wide table: the division table (proof_protocol_decoder_amd/arithmetic_div.py, a
registered program: 1650 columns, 1686 constraints and a 50-element product port, K5 interpreted) next to AIR 7 (the
multiplication table: 1217 columns, 1218 constraints, K5 compiled) at 2^14 rows on one MI355X, calls alternating.
  python tools/arithmetic_div_probe.py                       wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the division table, bp_stark_prove_air(7)
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_div_probe.py
  python tools/arithmetic_div_probe.py --summary OUT         medians per kernel from that trace: the two K5s, the two
                                                             witness kernels, the port's witness pair
(profiles/arithmetic_div.txt is the first output followed by the summary.)  The engine clock is not sampled."""
import glob, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LOG_N = 14
PROOFS = 20
MUL_COLS = 1217
KERNELS = ("arithmetic_div_trace_kernel", "arithmetic_mul_trace_kernel", "quotient_program_kernel", "quotient_air_kernel",
           "program_port_terms_kernel", "aux_suffix_product_kernel")


def summary(out_dir):
    import csv
    from proof_protocol_decoder_amd.arithmetic_div import N_COLS
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
    cells = N_COLS / MUL_COLS
    k5, k5_mul = pick("quotient_program_kernel"), pick("quotient_air_kernel<7")
    print("K5, quotient_program_kernel<true> / quotient_air_kernel<7>: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
          % (k5, k5_mul, k5 / k5_mul, k5 / k5_mul / cells))
    w, w_mul = pick("arithmetic_div_trace_kernel"), pick("arithmetic_mul_trace_kernel")
    print("witness, arithmetic_div_trace_kernel / arithmetic_mul_trace_kernel: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
          % (w, w_mul, w / w_mul, w / w_mul / cells))
    print("the port's witness pair, program_port_terms_kernel + aux_suffix_product_kernel<9>: %.1f + %.1f us"
          % (pick("program_port_terms_kernel"), pick("aux_suffix_product_kernel<9")))


def main():
    import numpy as np
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    from proof_protocol_decoder_amd import arithmetic_div as ad
    reg = ad.register()
    words = ad.program().assemble()
    n = 1 << LOG_N
    rng = np.random.default_rng(0xD1)
    inputs = rng.integers(-(1 << 63), (1 << 63) - 1, size=(n, 9), dtype=np.int64, endpoint=True)
    # operands of every length: the words above a random limb count are cleared
    for side in (1, 5):
        keep = rng.integers(0, 5, size=n)
        for w in range(4):
            inputs[:, side + w] *= (w < keep)
    inputs[:, 0] = rng.integers(1, 3, size=n) | (rng.integers(0, 2, size=n) << 8)
    d_inputs = torch.from_numpy(inputs).cuda()
    trace = bpg.ops.arithmetic_div_trace(LOG_N, d_inputs)
    assert bpg.ops.check_air_trace(reg, trace).ok
    cfg, cfg_mul = cases.cfg_for(reg, LOG_N), cases.cfg_for(7, LOG_N)
    print("division: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; AIR 7: %d columns; 2^%d rows, %d proofs each"
          % (reg, ad.N_COLS, int(words[9]), int(words[7]), int(words[8]), MUL_COLS, LOG_N, PROOFS), flush=True)
    wall, proofs = {reg: [], 7: []}, {}
    for k in range(PROOFS + 1):
        for a in (reg, 7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            proofs[a] = bpg.ops.stark_prove_trace(reg, cfg, trace) if a == reg else bpg.ops.stark_prove_air(7, cfg_mul, 0x77 + k)
            wall[a].append((time.perf_counter() - t0) * 1e3)
        bpg.ops.arithmetic_div_trace(LOG_N, d_inputs)           # the two witness kernels, for the kernel trace
        bpg.ops.arithmetic_mul_trace(LOG_N, seed=0x77 + k)
    torch.cuda.synchronize()
    bpg.ops.stark_verify_air(reg, cfg, proofs[reg])
    bpg.ops.stark_verify_air(7, cfg_mul, proofs[7])
    m = {a: statistics.median(t[1:]) for a, t in wall.items()}
    cells = ad.N_COLS / MUL_COLS
    print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(division) %.2f ms (min %.2f, max %.2f), "
          "bp_stark_prove_air(7) %.2f ms (min %.2f, max %.2f)" % (PROOFS, m[reg], min(wall[reg][1:]), max(wall[reg][1:]), m[7],
                                                                  min(wall[7][1:]), max(wall[7][1:])))
    print("division / AIR 7: %.2f per table, %.2f per trace cell (%.3f times the cells)" % (m[reg] / m[7], m[reg] / m[7] / cells, cells))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
