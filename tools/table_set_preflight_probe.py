"""What the pre-flight of a table set costs next to proving it: bp_check_table_set against bp_stark_prove_table_set on
the same arguments, calls alternating, the wall time of each taken on the host.  Three sets:
  (r)   the two-table range-check set of tools/air_program_log_ports_probe.py (b) at 2^16 rows: eight kind-1 limb ports
        into a kind-2 port over the constant column 0 .. 2^16 - 1;
  (f16) two flag tables (tests/air_program_port_cases.py, flag_program) of 2^16 rows: half the rows of the first send a
        3-element tuple, the second exposes them in a seeded permutation;
  (f20) the same at 2^20 rows.
  python tools/table_set_preflight_probe.py                 medians of the alternating calls
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/table_set_preflight_probe.py
  python tools/table_set_preflight_probe.py --summary OUT   medians per pre-flight kernel from the trace
(profiles/table_set_preflight.txt holds both outputs)."""
import glob, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
CALLS = 10
KERNELS = ("set_keys_program_kernel", "set_keys_builtin_kernel", "set_clear_kernel", "set_scan_kernel", "air_check_program_kernel",
           "air_check_alpha_kernel")


def summary(out_dir):
    import csv
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    times = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if any(name in k for name in KERNELS):
                key = (k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))
                times.setdefault(key, []).append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3)
    print("# per-launch kernel time in microseconds; grid in work-items; the first launch of each (warm-up) dropped")
    for key in sorted(times):
        t = times[key][1:] if len(times[key]) > 2 else times[key]
        print("%-28s grid=%-9d launches %3d  median %9.1f  min %9.1f  max %9.1f" % (key[0], key[1], len(t), statistics.median(t), min(t), max(t)))


def range_set(bpg, cases, torch):
    from air_program_log_ports_probe import LIMBS, LOG_N, lookup_programs
    n = 1 << LOG_N
    g = torch.Generator(device="cuda").manual_seed(16)
    limbs = torch.randint(0, 1 << 16, (LIMBS, n), dtype=torch.int64, device="cuda", generator=g)
    b_id, r_id = (bpg.ops.air_register(p.assemble()) for p in lookup_programs())
    r_trace = torch.zeros((8, n), dtype=torch.int64, device="cuda")
    r_trace[0] = bpg.ops.range_multiplicities(limbs, 16)
    consts = torch.arange(n, dtype=torch.int64, device="cuda").view(1, n)
    tables = [{"air_id": b_id, "cfg": cases.cfg_for(b_id, LOG_N), "trace": limbs},
              {"air_id": r_id, "cfg": cases.cfg_for(r_id, LOG_N), "trace": r_trace, "consts": consts}]
    return tables, [([(0, k) for k in range(LIMBS)], (1, 0))]


def flag_set(bpg, cases, torch, log_n):
    import air_program_port_cases as pc
    n = 1 << log_n
    g = torch.Generator(device="cuda").manual_seed(log_n)
    a = torch.zeros((8, n), dtype=torch.int64, device="cuda")
    a[0] = torch.randint(0, 2, (n,), dtype=torch.int64, device="cuda", generator=g)
    a[1:4] = torch.randint(0, 1 << 62, (3, n), dtype=torch.int64, device="cuda", generator=g)
    a[4] = torch.arange(5, 5 + n, dtype=torch.int64, device="cuda")
    b = a.clone()
    b[:4] = a[:4][:, torch.randperm(n, device="cuda", generator=g)]
    reg = bpg.ops.air_register(pc.flag_program().assemble())
    cfg = cases.cfg_for(reg, log_n)
    return [{"air_id": reg, "cfg": cfg, "trace": a}, {"air_id": reg, "cfg": cfg, "trace": b}], [([(0, 0)], (1, 0))]


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    print("# wall time per call in milliseconds, medians of %d alternating calls (the first of each dropped); %d queries; engine clock "
          "not sampled" % (CALLS, cases.cfg_for(3, 16).num_queries))
    for name, (tables, links) in (("(r)   range set, 2 x 2^16 rows, 9 ports", range_set(bpg, cases, torch)),
                                  ("(f16) flag set,  2 x 2^16 rows, 2 ports", flag_set(bpg, cases, torch, 16)),
                                  ("(f20) flag set,  2 x 2^20 rows, 2 ports", flag_set(bpg, cases, torch, 20))):
        wall = {"check": [], "prove": []}
        for _ in range(CALLS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = bpg.ops.check_table_set(tables, links)
            t1 = time.perf_counter()
            container = bpg.ops.stark_prove_table_set(tables, links)
            t2 = time.perf_counter()
            wall["check"].append(t1 - t0)
            wall["prove"].append(t2 - t1)
        assert report.ok and report.links[0].n_looking > 0, report
        ms = lambda v: 1e3 * statistics.median(v[1:])
        print("%s: bp_check_table_set %8.2f ms   bp_stark_prove_table_set %8.2f ms (container %d words)   check / prove %.3f   "
              "(%d looking, %d looked rows)" % (name, ms(wall["check"]), ms(wall["prove"]), container.size, ms(wall["check"]) / ms(wall["prove"]),
                                                report.links[0].n_looking, report.links[0].n_looked), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
