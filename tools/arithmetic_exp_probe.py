"""What the exponentiation table costs next to the division table and the signed table: three registered programs on the
run-time stack (proof_protocol_decoder_amd/arithmetic_exp.py: 2003 columns, 2357 constraints, a 48-element product port,
the first with transition and last-row families; arithmetic_div.py: 1650 columns; arithmetic_sdiv.py: 2499 columns), K5
interpreted for all, at 2^14 rows on one MI355X, calls alternating.  The exponentiation table is timed on two draws: a
SHORT one, exponents of 1 .. 64 bits (about 500 operations), and the WORST one, 64 operations with exponents of 256 bits,
where a lane replays up to 255 steps and goes on to the last for res.
  python tools/arithmetic_exp_probe.py                       wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the exponentiation table (both draws), the division and the
                                                             signed table
  python tools/arithmetic_exp_probe.py --units               the exponentiation table's proof with 1, 2 and 4 limbs a unit
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_exp_probe.py --table exp-short
  (and again with --table exp-worst into OUT2, --table division into OUT3 and --table signed into OUT4: one table a run,
  because K5 is one kernel name and two programs may get the same grid)
  (and the --units run into OUT5: the three cuts get grids of 9, 10 and 6 workgroup rows, which tells their K5s apart)
  python tools/arithmetic_exp_probe.py --summary OUT OUT2 OUT3 OUT4 [OUT5]
                                                             medians per kernel from those traces: K5 and the witness
                                                             kernel of every table, K5 of every cut
(profiles/arithmetic_exp.txt is the first two outputs followed by the summary.)  The alternating rounds and the reading of
a kernel trace are tools/arithmetic_mod_probe.py's, the signed draw tools/arithmetic_sdiv_probe.py's."""
import os, random, statistics, sys
from arithmetic_mod_probe import LOG_N, PROOFS, inputs_for, kernel_medians, median_proofs, wg_rows
from arithmetic_sdiv_probe import signed_inputs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TABLES = ("exp-short", "exp-worst", "division", "signed")
WITNESS = {"exp-short": "arithmetic_exp_trace_kernel", "exp-worst": "arithmetic_exp_trace_kernel", "division": "arithmetic_div_trace_kernel",
           "signed": "arithmetic_sdiv_trace_kernel"}
KERNELS = tuple(sorted(set(WITNESS.values()))) + ("quotient_program_kernel",)


def exp_ops(n, worst, seed):
    """operations that fill n rows: 256-bit exponents with bit 255 set (worst), else exponents of 1 .. 64 bits; bases of
    256 bits, every second one exposed"""
    rng = random.Random(seed)
    ops, left = [], n
    while left:
        bits = 256 if worst else min(left, rng.randint(1, 64))
        ops.append((1, rng.getrandbits(256), rng.getrandbits(bits) | 1 << (bits - 1), len(ops) & 1))
        left -= bits
    return ops


def modules():
    from proof_protocol_decoder_amd import arithmetic_div, arithmetic_exp, arithmetic_sdiv
    return {"exp-short": arithmetic_exp, "exp-worst": arithmetic_exp, "division": arithmetic_div, "signed": arithmetic_sdiv}


def summary(*outs):
    mods = modules()
    pick = lambda m, part: next(v for key, v in m.items() if part in key[0])
    med = {name: kernel_medians(out, KERNELS) for name, out in zip(TABLES, outs)}
    k5 = {name: pick(med[name], "quotient_program_kernel") for name in TABLES}
    wit = {name: pick(med[name], WITNESS[name]) for name in TABLES}
    for name in TABLES[:2]:
        for other in TABLES[2:]:
            cells = mods[name].N_COLS / mods[other].N_COLS
            print("K5, quotient_program_kernel<true>, %s (grid.y %d) / %s (grid.y %d): %.1f / %.1f us = %.2f per table, %.2f per trace cell"
                  % (name, wg_rows(len(mods[name].program().units) + 1), other, wg_rows(len(mods[other].program().units) + 1), k5[name],
                     k5[other], k5[name] / k5[other], k5[name] / k5[other] / cells))
            print("witness, %s (%s) / %s: %.1f / %.1f us = %.2f per table, %.2f per trace cell"
                  % (WITNESS[name], name, WITNESS[other], wit[name], wit[other], wit[name] / wit[other], wit[name] / wit[other] / cells))
        print("%s: the witness kernel is %.2f of the proof's K5" % (name, wit[name] / k5[name]))
    if len(outs) > 4:
        k5 = {key[2]: v for key, v in kernel_medians(outs[4], ("quotient_program_kernel",)).items()}
        for c in mods["exp-short"].CUTS:
            rows = wg_rows(16 // c + 2)
            print("K5, exponentiation table, %d limbs a unit (grid.y %d): %.1f us" % (c, rows, k5[rows]))


def main(units, only):
    import numpy as np
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    mods = modules()
    n = 1 << LOG_N
    ex = mods["exp-short"]
    regs = {name: m.register() for name, m in mods.items()}
    d_in = {"division": torch.from_numpy(inputs_for(n, 9, 0xD1)).cuda(), "signed": torch.from_numpy(signed_inputs(n, 0x5D1)).cuda()}
    n_ops = {}
    for name, worst in (("exp-short", False), ("exp-worst", True)):
        words, starts = ex.pack_ops(exp_ops(n, worst, 0xE8), LOG_N)
        n_ops[name] = len(words)
        d_in[name] = (torch.from_numpy(words.view(np.int64)).cuda(), torch.from_numpy(starts.view(np.int32)).cuda())
    witness = {"exp-short": lambda: bpg.ops.arithmetic_exp_trace(LOG_N, *d_in["exp-short"]),
               "exp-worst": lambda: bpg.ops.arithmetic_exp_trace(LOG_N, *d_in["exp-worst"]),
               "division": lambda: bpg.ops.arithmetic_div_trace(LOG_N, d_in["division"]),
               "signed": lambda: bpg.ops.arithmetic_sdiv_trace(LOG_N, d_in["signed"])}
    names = ("exp-short",) if units else TABLES if only is None else (only,)   # a run for one table's K5 launches no other program's
    traces = {name: witness[name]() for name in names}
    assert all(bpg.ops.check_air_trace(regs[name], traces[name]).ok for name in names)
    if units:
        tables = []
        for c in ex.CUTS:
            words = ex.program(c).assemble()
            air_id = bpg.ops.air_register(words)
            tables.append(("%d limbs a unit (%d units, n_regs %d, grid.y %d)" % (c, int(words[8]), int(words[7]), wg_rows(int(words[8]) + 1)),
                           lambda k, a=air_id, cfg=cases.cfg_for(air_id, LOG_N): bpg.ops.stark_prove_trace(a, cfg, traces["exp-short"])))
        for name, t in median_proofs(torch, tables).items():
            print("exponentiation table, %s: median of %d proofs %.2f ms (min %.2f, max %.2f)" % (name, PROOFS, statistics.median(t), min(t), max(t)))
        return
    words = ex.program().assemble()
    print("exponentiation: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; %d operations in the short draw, %d in the worst; "
          "division: %d columns; signed: %d columns; 2^%d rows, %d proofs each"
          % (regs["exp-short"], ex.N_COLS, int(words[9]), int(words[7]), int(words[8]), n_ops["exp-short"], n_ops["exp-worst"],
             mods["division"].N_COLS, mods["signed"].N_COLS, LOG_N, PROOFS), flush=True)
    cfgs = {name: cases.cfg_for(regs[name], LOG_N) for name in names}
    provers = [(name, lambda k, name=name: bpg.ops.stark_prove_trace(regs[name], cfgs[name], traces[name])) for name in names]
    wall = median_proofs(torch, provers)
    for _ in range(PROOFS):                                      # the witness kernels, for the kernel trace
        for name in names:
            witness[name]()
    torch.cuda.synchronize()
    for name in names[:2]:
        if name.startswith("exp"):
            bpg.ops.stark_verify_air(regs[name], cfgs[name], bpg.ops.stark_prove_trace(regs[name], cfgs[name], traces[name]))
    m = {k: statistics.median(t) for k, t in wall.items()}
    for name, t in wall.items():
        print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(%s) %.2f ms (min %.2f, max %.2f)"
              % (PROOFS, name, m[name], min(t), max(t)))
    if only is None:
        for name in TABLES[:2]:
            for other in TABLES[2:]:
                cells = ex.N_COLS / mods[other].N_COLS
                print("%s / %s: %.2f per table, %.2f per trace cell (%.3f times the cells)"
                      % (name, other, m[name] / m[other], m[name] / m[other] / cells, cells))
        # the witness kernels' wall time, by device events (the kernel trace has the kernel's own time)
        for name in names:
            times = []
            for _ in range(PROOFS + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                witness[name]()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            print("witness by device events, median of %d (the first dropped): %s (%s) %.1f us" % (PROOFS, WITNESS[name], name, statistics.median(times[1:])))


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) > 4 and args[0] == "--summary":
        summary(*args[1:6])
    else:
        main(units="--units" in args, only=args[args.index("--table") + 1] if "--table" in args else None)
