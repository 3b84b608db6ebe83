"""Where the shift table's K5 time goes: the shipped program next to programs with parts of it left out, one limb a unit,
every one proven from the same 2^14-row trace on one MI355X.  The partial programs are not the table's AIR -- they state
fewer constraints, in one family sized to what they emit -- and exist only to be timed: K5 is interpreted, so its time
is the code's.
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/arithmetic_shift_parts_probe.py
  python tools/arithmetic_shift_parts_probe.py --summary OUT     K5 (quotient_program_kernel<true>) per program, medians
                                                                 of 7 launches, told apart by their order in the trace
(The end of profiles/arithmetic_shift.txt is this output.)  The body of variant() is arithmetic_shift.program()'s limb
loop with switches; its first unit keeps only the flags."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LOG_N, PROOFS = 14, 8


def variant(result=True, cross=True, split=True, bits=True):
    from proof_protocol_decoder_amd import arithmetic_shift as sh
    from proof_protocol_decoder_amd.air_program import ALL_ROWS, Builder
    from proof_protocol_decoder_amd.word_table import BASE, bits_value
    b = Builder(sh.N_COLS)
    b.family(4000, ALL_ROWS, 3)
    used = [0]

    class At(dict):
        def __missing__(self, name):          # a block of indices per family name, handed out on first use
            self[name] = used[0]
            used[0] += dict((n, c) for n, c, _ in sh.FAMILIES)[name]
            return self[name]
    at = At()
    is_shl, is_shr, is_sar = b.loc(sh.COL_IS_SHL), b.loc(sh.COL_IS_SHR), b.loc(sh.COL_IS_SAR)
    g, z, fill, w = b.loc(sh.COL_G), b.loc(sh.COL_Z), b.loc(sh.COL_FILL), b.loc(sh.COL_W)
    right = is_shr + is_sar
    b.unit()
    sh.flags3(b, at, (is_shl, is_shr, is_sar), g, z)
    for k in range(16):
        b.unit()
        if bits:
            sk = bits_value(b, sh.COL_S_BITS + 16 * k, 16, at["operand_bits"] + 16 * k)
            xk = bits_value(b, sh.COL_X_BITS + 16 * k, 16, at["operand_bits"] + 256 + 16 * k)
            b.emit(at["operand_limbs"] + k, b.loc(sh.COL_S + k) - sk)
            b.emit(at["operand_limbs"] + 16 + k, b.loc(sh.COL_X + k) - xk)
        if split:
            lo = bits_value(b, sh.COL_LO_BITS + 16 * k, 16, at["split_bits"] + 16 * k)
            hi = bits_value(b, sh.COL_HI_BITS + 16 * k, 16, at["split_bits"] + 256 + 16 * k)
            b.emit(at["split"] + k, b.loc(sh.COL_X + k) * w - (lo + BASE * hi))
            b.emit(at["y"] + k, b.loc(sh.COL_Y + k) - (is_shl * lo + right * hi))
            if cross and k + 1 < 16:
                b.emit(at["y"] + k + 1, 0 - is_shl * hi)
            if cross and k:
                b.emit(at["y"] + k - 1, 0 - right * lo)
        if result:
            moved = above = 0
            for d in range(-15, k + 1):
                if k - d < 16:
                    moved = moved + b.loc(sh.COL_E + 15 + d) * b.loc(sh.COL_Y + k - d)
                else:
                    above = above + b.loc(sh.COL_E + 15 + d)
            b.emit(at["result"] + k, b.loc(sh.COL_RES + k) - (moved + (BASE - 1) * fill * (above + (1 - z))))
    b.port(g, [b.loc(c) for c in sh.TUPLE_COLS])
    b.families[0] = (0, used[0], ALL_ROWS, 3)
    return b


VARIANTS = [("the limb units (first unit: flags only)", {}), ("... without result", dict(result=False)),
            ("... without the shares of the neighbours' y", dict(cross=False)), ("... without split and y", dict(split=False)),
            ("... without the bits of s and x", dict(bits=False)), ("result alone", dict(split=False, bits=False))]


def programs():
    from proof_protocol_decoder_amd import arithmetic_shift as sh
    return [("shipped", sh.program().assemble())] + [(name, variant(**kw).assemble()) for name, kw in VARIANTS]


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    from arithmetic_shift_probe import shift_inputs
    trace = bpg.ops.arithmetic_shift_trace(LOG_N, torch.from_numpy(shift_inputs(1 << LOG_N, 0x5F7)).cuda())
    for name, words in programs():
        air_id = bpg.ops.air_register(words)
        cfg = cases.cfg_for(air_id, LOG_N)
        for _ in range(PROOFS):                                  # the prover proves what it is given
            bpg.ops.stark_prove_trace(air_id, cfg, trace)
        torch.cuda.synchronize()


def summary(out_dir):
    import csv, glob
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "quotient_program_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    progs = programs()
    assert len(t) == PROOFS * len(progs), "%d K5 launches for %d programs" % (len(t), len(progs))
    print("# K5 per program, microseconds, median of %d launches (the first of each dropped), 2^%d rows" % (PROOFS - 1, LOG_N))
    for i, (name, words) in enumerate(progs):
        print("%-48s %5d code words  %7.1f" % (name, int(words[9]), statistics.median(t[PROOFS * i + 1:PROOFS * (i + 1)])))


if __name__ == "__main__":
    summary(sys.argv[2]) if sys.argv[1:2] == ["--summary"] else main()
