"""Wall time on the host of bp_check_txn_witness: on the decoded entry of tests/test_gpu_witness_preflight.py with its own
witness (four tables proven by their AIRs, two lookups), on the seeded case with all six AIRs (three lookups, the one
with five looking ends among them) at the tests' heights, and on that case at taller tables (sponge 2^12, logic 2^15,
Keccak-f 2^14, memory 2^13 rows; a state of its own).  Median (min, max) of 10 calls after one warm-up; the arguments are built once, outside
the timed region.  BPG_LIBBPG names another build of the library, for an A/B in one session (profiles/link_check_ab.txt).
  python tools/witness_preflight_probe.py"""
import ctypes as C, os, statistics, struct, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CALLS = 10


def main():
    import txn_table_cases as tc
    from proof_protocol_decoder_amd import proof_gen as pg
    L = pg._bind()
    print("# wall time per call in milliseconds, median (min, max) of %d calls; engine clock not sampled" % CALLS)
    six = next(c for c in tc.ACCEPTED if c.name == "six_together")
    tall = six._replace(name="six_tall", log_n=(6, 9, 7, 14, 12, 15, 13))
    for cfg, arena, cases in ((tc.CFG, 256 << 20, (tc.decoded_case(), (six, None))),
                              (dict(tc.CFG, table_log_hi=[8, 10, 8, 15, 13, 16, 14]), 2 << 30, ((tall, None),))):
        b = pg.ProverStateBuilder()
        for t, name in enumerate(pg.TABLES):
            getattr(b, "set_%s_circuit_size" % name)(range(cfg["table_log_lo"][t], cfg["table_log_hi"][t]))
        b.set(**{k: v for k, v in cfg.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=arena)
        st = b.build()
        try:
            for case, words in cases:
                ir = struct.pack("<25Q", *(words or tc.ir_words(case)))
                w, keep = tc.witness_struct(pg, case)
                rep = pg.WitnessReport()
                ts = []
                for _ in range(CALLS + 1):
                    t0 = time.perf_counter()
                    rc = L.bp_check_txn_witness(st._h, ir, len(ir), C.byref(w) if w is not None else None, C.byref(rep))
                    ts.append(1e3 * (time.perf_counter() - t0))
                    assert rc == 0, L.bp_last_error().decode()
                ts = ts[1:]
                print("bp_check_txn_witness(%-14s heights 2^%s) %7.2f ms (%.2f, %.2f)   lookup rows %s" % (
                    case.name + ",", list(case.log_n), statistics.median(ts), min(ts), max(ts),
                    [(l.n_looking, l.n_looked) for l in rep.lookup]), flush=True)
        finally:
            st.close()

if __name__ == "__main__":
    main()
