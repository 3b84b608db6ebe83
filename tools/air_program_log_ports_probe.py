"""Range checks two ways: a table of eight 16-bit limbs at 2^16 rows, proven (a) with the bit decomposition in the
program -- 128 bit columns, 128 boolean constraints and 8 recompositions, a "BPGAIRP1" program proven alone -- and (b)
with eight kind-1 log ports (filter 1: every row sends) into a kind-2 port over the constant column 0 .. 2^16 - 1,
whose filter is the column of multiplicities bp_range_multiplicities makes.  A program has at most eight ports, so the
ninth -- the looked one -- is a second table of the set, 2^16 rows of the narrowest width a table has (8 columns, one
of them used): two "BPGAIRP3" programs proven as a two-table set.  Proofs alternate; the wall time of each call is taken
on the host.
  python tools/air_program_log_ports_probe.py                 medians of the alternating proofs
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/air_program_log_ports_probe.py
  python tools/air_program_log_ports_probe.py --summary OUT   medians per witness kernel from the trace
(profiles/air_program_log_ports.txt holds both outputs)."""
import glob, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LOG_N = 16
LIMBS = 8
PROOFS = 10
KERNELS = ("range_multiplicities_kernel", "program_port_terms_kernel", "port_running_columns_kernel", "aux_suffix_product_kernel",
           "quotient_program_kernel")


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
    for key in sorted(times):
        t = times[key][1:] if len(times[key]) > 2 else times[key]
        print("%-44s grid=(%d,%d)  launches %2d  median %9.1f  min %9.1f  max %9.1f" % (key[0], key[1], key[2], len(t), statistics.median(t), min(t), max(t)))


def bit_program():
    """(a) limbs in columns 0 .. 7, limb k's bits in columns 8 + 16 k .. 8 + 16 k + 15"""
    from proof_protocol_decoder_amd.air_program import ALL_ROWS, Builder
    b = Builder(LIMBS + 16 * LIMBS)
    bits = b.family(16 * LIMBS, ALL_ROWS, 2)
    sums = b.family(LIMBS, ALL_ROWS, 1)
    for k in range(LIMBS):
        b.unit()
        acc = 0
        for j in range(16):
            bit = b.loc(LIMBS + 16 * k + j)
            b.emit(bits + 16 * k + j, bit * bit - bit)
            acc = acc + bit * (1 << j)
        b.emit(sums + k, b.loc(k) - acc)
    return b


def lookup_programs():
    """(b) the limb table: limbs in columns 0 .. 7, a port each; the range table: the multiplicities in column 0,
    constant column 0 = 0 .. 2^16 - 1.  (A program states at least one constraint; these tables' are all the library's.)"""
    from proof_protocol_decoder_amd.air_program import ALL_ROWS, Builder
    b = Builder(LIMBS)
    b.unit()
    b.emit(b.family(1, ALL_ROWS, 1), 0)
    for k in range(LIMBS):
        b.log_port(1, [b.loc(k)])
    r = Builder(8, n_const=1)
    r.unit()
    r.emit(r.family(1, ALL_ROWS, 1), 0)
    r.log_port(r.loc(0), [r.cst(0)], multiplicity=True)
    return b, r


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    n = 1 << LOG_N
    g = torch.Generator(device="cuda").manual_seed(16)
    limbs = torch.randint(0, 1 << 16, (LIMBS, n), dtype=torch.int64, device="cuda", generator=g)
    a_prog, (b_prog, r_prog) = bit_program(), lookup_programs()
    a_id, b_id, r_id = (bpg.ops.air_register(p.assemble()) for p in (a_prog, b_prog, r_prog))
    a_trace = torch.cat([limbs] + [(limbs[k:k + 1] >> torch.arange(16, device="cuda").view(16, 1)) & 1 for k in range(LIMBS)]).contiguous()
    consts = torch.arange(n, dtype=torch.int64, device="cuda").view(1, n)
    r_trace = torch.zeros((8, n), dtype=torch.int64, device="cuda")
    a_cfg, b_cfg, r_cfg = (cases.cfg_for(i, LOG_N) for i in (a_id, b_id, r_id))
    tables = [{"air_id": b_id, "cfg": b_cfg}, {"air_id": r_id, "cfg": r_cfg}]
    links = [([(0, k) for k in range(LIMBS)], (1, 0))]
    print("(a) bits: program 0x%08x, %d columns, %d constraints, %d code words; (b) lookup: programs 0x%08x (%d columns, %d ports, %d code "
          "words) and 0x%08x (%d columns + 1 constant, 1 port); 2^%d rows, %d queries"
          % (a_id, a_cfg.n_cols, a_prog.n_constraints, int(a_prog.assemble()[9]), b_id, b_cfg.n_cols, len(b_prog.ports),
             int(b_prog.assemble()[9]), r_id, r_cfg.n_cols, LOG_N, a_cfg.num_queries), flush=True)
    assert bpg.ops.check_air_trace(a_id, a_trace).ok
    wall = {"a": [], "b": [], "b_mult": []}
    for _ in range(PROOFS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a_proof = bpg.ops.stark_prove_trace(a_id, a_cfg, a_trace)
        t1 = time.perf_counter()
        r_trace[0] = bpg.ops.range_multiplicities(limbs, 16)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        container = bpg.ops.stark_prove_table_set([dict(tables[0], trace=limbs), dict(tables[1], trace=r_trace, consts=consts)], links)
        t3 = time.perf_counter()
        wall["a"].append(t1 - t0)
        wall["b_mult"].append(t2 - t1)
        wall["b"].append(t3 - t2)
    assert cases.verify(a_id, a_cfg, a_proof) == 0
    _, lde = bpg.ops.lde_batch(consts, r_cfg.rate_bits)
    cap = bpg.ops.merkle_commit(lde, LOG_N, r_cfg.rate_bits, r_cfg.cap_height).cpu().numpy().view("uint64")[-(1 << r_cfg.cap_height):].reshape(-1)
    bpg.ops.stark_verify_table_set(tables, links, container, const_caps=[None, cap])
    ms = lambda v: 1e3 * statistics.median(v[1:])
    print("# wall time per call in milliseconds, medians of %d alternating proofs (the first of each dropped); engine clock not sampled" % PROOFS)
    print("(a) bit decomposition, bp_stark_prove_trace:                     %8.2f ms, proof %d words" % (ms(wall["a"]), a_proof.size))
    print("(b) log ports, bp_stark_prove_table_set (two tables; commits the constants): %8.2f ms, container %d words" % (ms(wall["b"]), container.size))
    print("(b) bp_range_multiplicities (8 x 2^16 values, log_range 16):     %8.2f ms" % ms(wall["b_mult"]))
    print("(b) / (a): %.2f" % ((ms(wall["b"]) + ms(wall["b_mult"])) / ms(wall["a"])))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
