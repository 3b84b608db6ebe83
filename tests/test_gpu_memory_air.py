"""AIR 3 (memory log, csrc/air.hpp) on the GPU against the oracle's independent statement of it (oracle/memory_air.c):
the witness generator, K5 alone through bp_quotient_eval, and whole table proofs byte for byte.  The tests are
builtin_airs.gpu_tests, the same for all seven AIRs, over this AIR's record (its shapes, seeds and spot checks, with a
note on why those heights)."""
from builtin_airs import gpu_tests, memory

pytestmark, test_witness_matches_oracle, test_quotient_eval_matches_oracle, test_table_proof_bit_exact, \
    test_wrong_shapes_for_the_air_are_refused = gpu_tests(memory)
