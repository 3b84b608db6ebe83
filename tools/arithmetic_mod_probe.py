"""What the modular table costs next to the division table: two registered programs on the run-time stack
(proof_protocol_decoder_amd/arithmetic_mod.py: 2560 columns, 2612 constraints, a 66-element product port;
arithmetic_div.py: 1650 columns, 1686 constraints, a 50-element port), K5 interpreted for both, at 2^14 rows on one
MI355X, calls alternating.
  python tools/arithmetic_mod_probe.py                       wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the modular table and on the division table
  python tools/arithmetic_mod_probe.py --units               the modular table's proof with 1, 2 and 4 product columns a unit
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_mod_probe.py
  python tools/arithmetic_mod_probe.py --summary OUT         medians per kernel from that trace: K5 at both widths, the two
                                                             witness kernels
(profiles/arithmetic_mod.txt is the first two outputs followed by the summary.)  The engine clock is not sampled."""
import glob, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LOG_N = 14
PROOFS = 20
KERNELS = ("arithmetic_mod_trace_kernel", "arithmetic_div_trace_kernel", "quotient_program_kernel")


def wg_rows(n_units):
    """the workgroup rows (grid.y) the prover gives K5 on an idle device at 2^LOG_N rows, rate_bits 1 (csrc/prover.cpp)"""
    wg_x = (2 << LOG_N) // 256
    want = min(n_units, max(1, -(-2048 // wg_x)))
    per_row = -(-n_units // want)
    return -(-n_units // per_row)


def kernel_medians(out_dir, kernels):
    """prints one line per (kernel, grid) of the trace under out_dir whose name holds one of `kernels`; {(name, grid x,
    grid y): median us}.  tools/arithmetic_div_probe.py reads its trace with it too."""
    import csv
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    times = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if any(name in k for name in kernels):
                key = (k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0),
                       int(r.get("Grid_Size_Y") or 1))
                times.setdefault(key, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    print("# per-launch kernel time in microseconds; grid in work-items; the first launch of each (warm-up) dropped")
    med = {}
    for key in sorted(times):
        t = times[key][1:] if len(times[key]) > 2 else times[key]
        med[key] = statistics.median(t)
        print("%-44s grid=(%d,%d)  launches %2d  median %9.1f  min %9.1f  max %9.1f" % (key[0], key[1], key[2], len(t), med[key], min(t), max(t)))
    return med


def summary(out_dir):
    from proof_protocol_decoder_amd import arithmetic_div as ad, arithmetic_mod as am
    med = kernel_medians(out_dir, KERNELS)
    cells = am.N_COLS / ad.N_COLS
    # K5 packs a program's units (and the library's one for the port) into workgroup rows, grid.y: at most 16 at this height
    k5 = {key[2]: v for key, v in med.items() if "quotient_program_kernel" in key[0]}
    rows_mod, rows_div = wg_rows(len(am.program().units) + 1), wg_rows(len(ad.program().units) + 1)
    if rows_mod != rows_div and rows_mod in k5 and rows_div in k5:
        print("K5, quotient_program_kernel, modular (grid.y %d) / division (grid.y %d): %.1f / %.1f us = %.2f per table, %.2f per trace cell"
              % (rows_mod, rows_div, k5[rows_mod], k5[rows_div], k5[rows_mod] / k5[rows_div], k5[rows_mod] / k5[rows_div] / cells))
    pick = lambda part: next(v for key, v in med.items() if part in key[0])
    w, w_div = pick("arithmetic_mod_trace_kernel"), pick("arithmetic_div_trace_kernel")
    print("witness, arithmetic_mod_trace_kernel / arithmetic_div_trace_kernel: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
          % (w, w_div, w / w_div, w / w_div / cells))


def inputs_for(n, words, seed):
    """[n, words] int64: word 0 a flag (1 or 2) and an exposed bit, then operands of every length -- the 64-bit words
    above a random count are cleared"""
    import numpy as np
    rng = np.random.default_rng(seed)
    inputs = rng.integers(-(1 << 63), (1 << 63) - 1, size=(n, words), dtype=np.int64, endpoint=True)
    for side in range(1, words, 4):
        keep = rng.integers(0, 5, size=n)
        for w in range(4):
            inputs[:, side + w] *= (w < keep)
    inputs[:, 0] = rng.integers(1, 3, size=n) | (rng.integers(0, 2, size=n) << 8)
    return inputs


def median_proofs(torch, provers, after_round=lambda k: None):
    """provers: [(name, prove(k))]; PROOFS + 1 alternating rounds, round k ending with after_round(k), the first dropped;
    {name: [ms]}.  tools/arithmetic_div_probe.py times its pair with it too."""
    wall = {name: [] for name, _ in provers}
    for k in range(PROOFS + 1):
        for name, prove in provers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prove(k)
            wall[name].append((time.perf_counter() - t0) * 1e3)
        after_round(k)
    return {name: t[1:] for name, t in wall.items()}


def main(units):
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    from proof_protocol_decoder_amd import arithmetic_div as ad, arithmetic_mod as am
    n = 1 << LOG_N
    reg, reg_div = am.register(), ad.register()
    d_mod, d_div = torch.from_numpy(inputs_for(n, 13, 0xA0D)).cuda(), torch.from_numpy(inputs_for(n, 9, 0xD1)).cuda()
    trace, trace_div = bpg.ops.arithmetic_mod_trace(LOG_N, d_mod), bpg.ops.arithmetic_div_trace(LOG_N, d_div)
    assert bpg.ops.check_air_trace(reg, trace).ok and bpg.ops.check_air_trace(reg_div, trace_div).ok
    if units:
        tables = []
        for c in (1, 2, 4):
            words = am.program(c).assemble()
            air_id = bpg.ops.air_register(words)
            tables.append(("%d columns a unit (%d units, n_regs %d)" % (c, int(words[8]), int(words[7])),
                           lambda k, a=air_id, cfg=cases.cfg_for(air_id, LOG_N): bpg.ops.stark_prove_trace(a, cfg, trace)))
        for name, t in median_proofs(torch, tables).items():
            print("modular table, %s: median of %d proofs %.2f ms (min %.2f, max %.2f)" % (name, PROOFS, statistics.median(t), min(t), max(t)))
        return
    words = am.program().assemble()
    print("modular: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; division: %d columns; 2^%d rows, %d proofs each"
          % (reg, am.N_COLS, int(words[9]), int(words[7]), int(words[8]), ad.N_COLS, LOG_N, PROOFS), flush=True)
    cfg, cfg_div = cases.cfg_for(reg, LOG_N), cases.cfg_for(reg_div, LOG_N)
    wall = median_proofs(torch, [("mod", lambda k: bpg.ops.stark_prove_trace(reg, cfg, trace)),
                                 ("div", lambda k: bpg.ops.stark_prove_trace(reg_div, cfg_div, trace_div))])
    for _ in range(PROOFS):                                      # the two witness kernels, for the kernel trace
        bpg.ops.arithmetic_mod_trace(LOG_N, d_mod)
        bpg.ops.arithmetic_div_trace(LOG_N, d_div)
    torch.cuda.synchronize()
    bpg.ops.stark_verify_air(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, trace))
    m = {k: statistics.median(t) for k, t in wall.items()}
    cells = am.N_COLS / ad.N_COLS
    print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(modular) %.2f ms (min %.2f, max %.2f), "
          "bp_stark_prove_trace(division) %.2f ms (min %.2f, max %.2f)" % (PROOFS, m["mod"], min(wall["mod"]), max(wall["mod"]), m["div"],
                                                                            min(wall["div"]), max(wall["div"])))
    print("modular / division: %.2f per table, %.2f per trace cell (%.3f times the cells)" % (m["mod"] / m["div"], m["mod"] / m["div"] / cells, cells))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main(units="--units" in sys.argv[1:])
