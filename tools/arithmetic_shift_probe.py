"""What the shift table costs next to the division table: two registered programs on the run-time stack
(proof_protocol_decoder_amd/arithmetic_shift.py: 1143 columns, 1165 constraints, a 51-element product port;
arithmetic_div.py: 1650 columns, 1686 constraints, a 50-element port), K5 interpreted for both, at 2^14 rows on one
MI355X, calls alternating.
  python tools/arithmetic_shift_probe.py                     wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the shift table and on the division table
  python tools/arithmetic_shift_probe.py --units             the shift table's proof with 1, 2 and 4 limbs a unit
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_shift_probe.py --table shift
  (and again with --table division into OUT2: one table a run, because K5 is one kernel name and the two programs may
  get the same grid)
  (and the --units run into OUT3: the three cuts get grids of 9, 10 and 6 workgroup rows, which tells their K5s apart)
  python tools/arithmetic_shift_probe.py --summary OUT OUT2 [OUT3]
                                                             medians per kernel from those traces: K5 and the witness
                                                             kernel of either table, K5 of every cut
(profiles/arithmetic_shift.txt is the first two outputs followed by the summary.)  The input draw, the alternating rounds
and the reading of a kernel trace are tools/arithmetic_mod_probe.py's."""
import os, statistics, sys
from arithmetic_mod_probe import LOG_N, PROOFS, inputs_for, kernel_medians, median_proofs, wg_rows
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KERNELS = ("arithmetic_shift_trace_kernel", "arithmetic_div_trace_kernel", "quotient_program_kernel")


def shift_inputs(n, seed):
    """inputs_for's draw with the three op bytes, and every second row's shift count cut to its low byte"""
    import numpy as np
    rng = np.random.default_rng(seed ^ 0x5F)
    inputs = inputs_for(n, 9, seed)
    inputs[:, 0] = rng.integers(1, 4, size=n) | (rng.integers(0, 2, size=n) << 8)
    inputs[::2, 1] &= 0xFF
    inputs[::2, 2:5] = 0
    return inputs


def summary(out_shift, out_div, out_units=None):
    from proof_protocol_decoder_amd import arithmetic_div as ad, arithmetic_shift as sh
    med, med_div = kernel_medians(out_shift, KERNELS), kernel_medians(out_div, KERNELS)
    cells = sh.N_COLS / ad.N_COLS
    pick = lambda m, part: next(v for key, v in m.items() if part in key[0])
    k5, k5_div = pick(med, "quotient_program_kernel"), pick(med_div, "quotient_program_kernel")
    print("K5, quotient_program_kernel<true>, shift (grid.y %d) / division (grid.y %d): %.1f / %.1f us = %.2f per table, %.2f per trace cell"
          % (wg_rows(len(sh.program().units) + 1), wg_rows(len(ad.program().units) + 1), k5, k5_div, k5 / k5_div, k5 / k5_div / cells))
    w, w_div = pick(med, "arithmetic_shift_trace_kernel"), pick(med_div, "arithmetic_div_trace_kernel")
    print("witness, arithmetic_shift_trace_kernel / arithmetic_div_trace_kernel: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
          % (w, w_div, w / w_div, w / w_div / cells))
    if out_units:
        k5 = {key[2]: v for key, v in kernel_medians(out_units, ("quotient_program_kernel",)).items()}
        for c in sh.CUTS:
            rows = wg_rows(16 // c + 2)
            print("K5, shift table, %d limbs a unit (grid.y %d): %.1f us" % (c, rows, k5[rows]))


def main(units, only):
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    from proof_protocol_decoder_amd import arithmetic_div as ad, arithmetic_shift as sh
    n = 1 << LOG_N
    reg, reg_div = sh.register(), ad.register()
    d_shift, d_div = torch.from_numpy(shift_inputs(n, 0x5F7)).cuda(), torch.from_numpy(inputs_for(n, 9, 0xD1)).cuda()
    trace, trace_div = bpg.ops.arithmetic_shift_trace(LOG_N, d_shift), bpg.ops.arithmetic_div_trace(LOG_N, d_div)
    assert bpg.ops.check_air_trace(reg, trace).ok and bpg.ops.check_air_trace(reg_div, trace_div).ok
    if units:
        tables = []
        for c in sh.CUTS:
            words = sh.program(c).assemble()
            air_id = bpg.ops.air_register(words)
            tables.append(("%d limbs a unit (%d units, n_regs %d, grid.y %d)" % (c, int(words[8]), int(words[7]), wg_rows(int(words[8]) + 1)),
                           lambda k, a=air_id, cfg=cases.cfg_for(air_id, LOG_N): bpg.ops.stark_prove_trace(a, cfg, trace)))
        for name, t in median_proofs(torch, tables).items():
            print("shift table, %s: median of %d proofs %.2f ms (min %.2f, max %.2f)" % (name, PROOFS, statistics.median(t), min(t), max(t)))
        return
    words = sh.program().assemble()
    print("shift: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; division: %d columns; 2^%d rows, %d proofs each"
          % (reg, sh.N_COLS, int(words[9]), int(words[7]), int(words[8]), ad.N_COLS, LOG_N, PROOFS), flush=True)
    cfg, cfg_div = cases.cfg_for(reg, LOG_N), cases.cfg_for(reg_div, LOG_N)
    provers = [("shift", lambda k: bpg.ops.stark_prove_trace(reg, cfg, trace)),
               ("division", lambda k: bpg.ops.stark_prove_trace(reg_div, cfg_div, trace_div))]
    provers = [p for p in provers if only in (None, p[0])]
    wall = median_proofs(torch, provers)
    for _ in range(PROOFS):                                      # the witness kernels, for the kernel trace
        if only in (None, "shift"):
            bpg.ops.arithmetic_shift_trace(LOG_N, d_shift)
        if only in (None, "division"):
            bpg.ops.arithmetic_div_trace(LOG_N, d_div)
    torch.cuda.synchronize()
    if only != "division":                                       # a run for the division table's K5 launches no other program's
        bpg.ops.stark_verify_air(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, trace))
    m = {k: statistics.median(t) for k, t in wall.items()}
    for name, t in wall.items():
        print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(%s) %.2f ms (min %.2f, max %.2f)"
              % (PROOFS, name, m[name], min(t), max(t)))
    if only is None:
        cells = sh.N_COLS / ad.N_COLS
        print("shift / division: %.2f per table, %.2f per trace cell (%.3f times the cells)"
              % (m["shift"] / m["division"], m["shift"] / m["division"] / cells, cells))


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 2 and args[0] == "--summary":
        summary(*args[1:4])
    else:
        main(units="--units" in args, only=args[args.index("--table") + 1] if "--table" in args else None)
