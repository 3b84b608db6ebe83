"""What the signed table costs next to the division table (the same loop, the same core) and the modular table (the
nearest in columns): three registered programs on the run-time stack (proof_protocol_decoder_amd/arithmetic_sdiv.py: 2499
columns, 2583 constraints, a 50-element product port; arithmetic_div.py: 1650 columns; arithmetic_mod.py: 2560 columns),
K5 interpreted for all, at 2^14 rows on one MI355X, calls alternating.
  python tools/arithmetic_sdiv_probe.py                      wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the signed, the division and the modular table
  python tools/arithmetic_sdiv_probe.py --units              the signed table's proof with 1 and 2 limbs a unit
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_sdiv_probe.py --table signed
  (and again with --table division into OUT2 and --table modular into OUT3: one table a run, because K5 is one kernel
  name and two programs may get the same grid)
  (and the --units run into OUT4: the two cuts get grids of 9 and 10 workgroup rows, which tells their K5s apart)
  python tools/arithmetic_sdiv_probe.py --summary OUT OUT2 OUT3 [OUT4]
                                                             medians per kernel from those traces: K5 and the witness
                                                             kernel of every table, K5 of either cut
(profiles/arithmetic_sdiv.txt is the first two outputs followed by the summary.)  The input draw, the alternating rounds
and the reading of a kernel trace are tools/arithmetic_mod_probe.py's."""
import os, statistics, sys
from arithmetic_mod_probe import LOG_N, PROOFS, inputs_for, kernel_medians, median_proofs, wg_rows
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TABLES = ("signed", "division", "modular")
WITNESS = {"signed": "arithmetic_sdiv_trace_kernel", "division": "arithmetic_div_trace_kernel", "modular": "arithmetic_mod_trace_kernel"}
KERNELS = tuple(WITNESS.values()) + ("quotient_program_kernel",)


def signed_inputs(n, seed):
    """inputs_for's draw of every length, every second x and every third y complemented: negative words whose magnitudes
    have every length too"""
    inputs = inputs_for(n, 9, seed)
    inputs[1::2, 1:5] = ~inputs[1::2, 1:5]
    inputs[2::3, 5:9] = ~inputs[2::3, 5:9]
    return inputs


def modules():
    from proof_protocol_decoder_amd import arithmetic_div, arithmetic_mod, arithmetic_sdiv
    return {"signed": arithmetic_sdiv, "division": arithmetic_div, "modular": arithmetic_mod}


def summary(out_signed, out_div, out_mod, out_units=None):
    mods = modules()
    pick = lambda m, part: next(v for key, v in m.items() if part in key[0])
    med = {name: kernel_medians(out, KERNELS) for name, out in zip(TABLES, (out_signed, out_div, out_mod))}
    k5 = {name: pick(med[name], "quotient_program_kernel") for name in TABLES}
    wit = {name: pick(med[name], WITNESS[name]) for name in TABLES}
    for other in TABLES[1:]:
        cells = mods["signed"].N_COLS / mods[other].N_COLS
        print("K5, quotient_program_kernel<true>, signed (grid.y %d) / %s (grid.y %d): %.1f / %.1f us = %.2f per table, %.2f per trace cell"
              % (wg_rows(len(mods["signed"].program().units) + 1), other, wg_rows(len(mods[other].program().units) + 1), k5["signed"],
                 k5[other], k5["signed"] / k5[other], k5["signed"] / k5[other] / cells))
        print("witness, %s / %s: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
              % (WITNESS["signed"], WITNESS[other], wit["signed"], wit[other], wit["signed"] / wit[other], wit["signed"] / wit[other] / cells))
    if out_units:
        k5 = {key[2]: v for key, v in kernel_medians(out_units, ("quotient_program_kernel",)).items()}
        for c in mods["signed"].CUTS:
            rows = wg_rows(16 // c + 2)
            print("K5, signed table, %d limbs a unit (grid.y %d): %.1f us" % (c, rows, k5[rows]))


def main(units, only):
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    mods = modules()
    n = 1 << LOG_N
    sd = mods["signed"]
    regs = {name: m.register() for name, m in mods.items()}
    d_in = {"signed": torch.from_numpy(signed_inputs(n, 0x5D1)).cuda(), "division": torch.from_numpy(inputs_for(n, 9, 0xD1)).cuda(),
            "modular": torch.from_numpy(inputs_for(n, 13, 0xA0D)).cuda()}
    witness = {"signed": bpg.ops.arithmetic_sdiv_trace, "division": bpg.ops.arithmetic_div_trace, "modular": bpg.ops.arithmetic_mod_trace}
    names = ("signed",) if units else TABLES if only is None else (only,)   # a run for one table's K5 launches no other program's
    traces = {name: witness[name](LOG_N, d_in[name]) for name in names}
    assert all(bpg.ops.check_air_trace(regs[name], traces[name]).ok for name in names)
    if units:
        tables = []
        for c in sd.CUTS:
            words = sd.program(c).assemble()
            air_id = bpg.ops.air_register(words)
            tables.append(("%d limbs a unit (%d units, n_regs %d, grid.y %d)" % (c, int(words[8]), int(words[7]), wg_rows(int(words[8]) + 1)),
                           lambda k, a=air_id, cfg=cases.cfg_for(air_id, LOG_N): bpg.ops.stark_prove_trace(a, cfg, traces["signed"])))
        for name, t in median_proofs(torch, tables).items():
            print("signed table, %s: median of %d proofs %.2f ms (min %.2f, max %.2f)" % (name, PROOFS, statistics.median(t), min(t), max(t)))
        return
    words = sd.program().assemble()
    print("signed: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; division: %d columns; modular: %d columns; 2^%d rows, "
          "%d proofs each" % (regs["signed"], sd.N_COLS, int(words[9]), int(words[7]), int(words[8]), mods["division"].N_COLS,
                              mods["modular"].N_COLS, LOG_N, PROOFS), flush=True)
    cfgs = {name: cases.cfg_for(regs[name], LOG_N) for name in names}
    provers = [(name, lambda k, name=name: bpg.ops.stark_prove_trace(regs[name], cfgs[name], traces[name])) for name in names]
    wall = median_proofs(torch, provers)
    for _ in range(PROOFS):                                      # the witness kernels, for the kernel trace
        for name in names:
            witness[name](LOG_N, d_in[name])
    torch.cuda.synchronize()
    if "signed" in names:
        bpg.ops.stark_verify_air(regs["signed"], cfgs["signed"], bpg.ops.stark_prove_trace(regs["signed"], cfgs["signed"], traces["signed"]))
    m = {k: statistics.median(t) for k, t in wall.items()}
    for name, t in wall.items():
        print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(%s) %.2f ms (min %.2f, max %.2f)"
              % (PROOFS, name, m[name], min(t), max(t)))
    if only is None:
        for other in TABLES[1:]:
            cells = sd.N_COLS / mods[other].N_COLS
            print("signed / %s: %.2f per table, %.2f per trace cell (%.3f times the cells)"
                  % (other, m["signed"] / m[other], m["signed"] / m[other] / cells, cells))


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 3 and args[0] == "--summary":
        summary(*args[1:5])
    else:
        main(units="--units" in args, only=args[args.index("--table") + 1] if "--table" in args else None)
