"""Wall time on the host of the lone table proofs: bp_stark_prove_air on the memory table (2^16 rows) and on AIR 8 (2^12),
bp_stark_prove_trace on the same memory trace, contiguous and as a column slice (stride 2^16 + 3: the pack).  Medians of
10 calls after one warm-up.  BPG_LIBBPG names another build of the library, for an A/B in one session
(profiles/caller_table_refactor_ab.txt).
  python tools/lone_table_probe.py"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CALLS = 10


def median_ms(torch, f):
    f()
    ts = []
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    import torch
    import proof_protocol_decoder_amd as bpg
    import air_program_cases as cases
    log_n = 16
    cfg, cfg8 = cases.cfg_for(3, log_n), cases.cfg_for(8, 12)
    trace = bpg.ops.memory_trace(log_n, seed=7)
    wide = torch.zeros((45, (1 << log_n) + 3), dtype=torch.int64, device="cuda")
    wide[:, :1 << log_n] = trace
    print("# wall time per call in milliseconds, median (min, max) of %d calls; %d queries; engine clock not sampled" % (CALLS, cfg.num_queries))
    for name, f in (("bp_stark_prove_air(3, 2^16)", lambda: bpg.ops.stark_prove_air(3, cfg, 7)),
                    ("bp_stark_prove_trace(3, 2^16)", lambda: bpg.ops.stark_prove_trace(3, cfg, trace)),
                    ("bp_stark_prove_trace(3, 2^16), strided", lambda: bpg.ops.stark_prove_trace(3, cfg, wide[:, :1 << log_n])),
                    ("bp_stark_prove_air(8, 2^12)", lambda: bpg.ops.stark_prove_air(8, cfg8, 7, 9))):
        print("%-40s %7.2f ms (%.2f, %.2f)" % ((name,) + median_ms(torch, f)), flush=True)


if __name__ == "__main__":
    main()
