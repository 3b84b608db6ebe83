"""What the run-time stack costs on a wide table: the division table (proof_protocol_decoder_amd/arithmetic_div.py, a
registered program: 1650 columns, 1686 constraints and a 50-element product port, K5 interpreted) next to AIR 7 (the
multiplication table: 1217 columns, 1218 constraints, K5 compiled) at 2^14 rows on one MI355X, calls alternating.
  python tools/arithmetic_div_probe.py                       wall time per proof, medians of 20: bp_stark_prove_trace on
                                                             the division table, bp_stark_prove_air(7)
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_div_probe.py
  python tools/arithmetic_div_probe.py --summary OUT         medians per kernel from that trace: the two K5s, the two
                                                             witness kernels, the port's witness pair
(profiles/arithmetic_div.txt is the first output followed by the summary.)  The engine clock is not sampled.  The input
draw, the alternating rounds and the reading of a kernel trace are tools/arithmetic_mod_probe.py's."""
import os, statistics, sys
from arithmetic_mod_probe import LOG_N, PROOFS, inputs_for, kernel_medians, median_proofs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MUL_COLS = 1217
KERNELS = ("arithmetic_div_trace_kernel", "arithmetic_mul_trace_kernel", "quotient_program_kernel", "quotient_air_kernel",
           "program_port_terms_kernel", "aux_suffix_product_kernel")


def summary(out_dir):
    from proof_protocol_decoder_amd.arithmetic_div import N_COLS
    med = {key[0]: v for key, v in kernel_medians(out_dir, KERNELS).items()}
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
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    from proof_protocol_decoder_amd import arithmetic_div as ad
    reg = ad.register()
    words = ad.program().assemble()
    n = 1 << LOG_N
    d_inputs = torch.from_numpy(inputs_for(n, 9, 0xD1)).cuda()
    trace = bpg.ops.arithmetic_div_trace(LOG_N, d_inputs)
    assert bpg.ops.check_air_trace(reg, trace).ok
    cfg, cfg_mul = cases.cfg_for(reg, LOG_N), cases.cfg_for(7, LOG_N)
    print("division: program 0x%08x, %d columns, %d code words, n_regs %d, %d units; AIR 7: %d columns; 2^%d rows, %d proofs each"
          % (reg, ad.N_COLS, int(words[9]), int(words[7]), int(words[8]), MUL_COLS, LOG_N, PROOFS), flush=True)
    proofs = {}

    def prove(a):
        def run(k):
            proofs[a] = bpg.ops.stark_prove_trace(reg, cfg, trace) if a == reg else bpg.ops.stark_prove_air(7, cfg_mul, 0x77 + k)
        return a, run

    def witnesses(k):                                            # the two witness kernels, for the kernel trace
        bpg.ops.arithmetic_div_trace(LOG_N, d_inputs)
        bpg.ops.arithmetic_mul_trace(LOG_N, seed=0x77 + k)

    wall = median_proofs(torch, [prove(reg), prove(7)], witnesses)
    torch.cuda.synchronize()
    bpg.ops.stark_verify_air(reg, cfg, proofs[reg])
    bpg.ops.stark_verify_air(7, cfg_mul, proofs[7])
    m = {a: statistics.median(t) for a, t in wall.items()}
    cells = ad.N_COLS / MUL_COLS
    print("wall per proof, median of %d (the first dropped): bp_stark_prove_trace(division) %.2f ms (min %.2f, max %.2f), "
          "bp_stark_prove_air(7) %.2f ms (min %.2f, max %.2f)" % (PROOFS, m[reg], min(wall[reg]), max(wall[reg]), m[7], min(wall[7]), max(wall[7])))
    print("division / AIR 7: %.2f per table, %.2f per trace cell (%.3f times the cells)" % (m[reg] / m[7], m[reg] / m[7] / cells, cells))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
