// tune.hpp -- every run-time knob of the library (the bp_tune_* entry points of bpg.h, tune.cpp) in one struct.
// A member's initialiser IS its default: bp_tune_reset() stores those, nothing else names them.  The decisions that
// read a knob (use_ntt_mx, use_split, quad_threshold, mx_sets, device_loaded, ...) stay next to the kernels they choose
// between; here are the values and the measurements that set the defaults.  Results never depend on a knob.
#pragma once
#include <atomic>
#include <cstdint>

namespace bpg {

struct Tune {
  // ---- Poseidon / Merkle (hash_kernels.hip)
  // Launches with fewer permutations than this use the small-launch kernels (4x the waves).  0 = automatic: the quad
  // form (4x the waves, 1.22x the instructions) pays while the chip is not full, so the threshold follows the number of
  // provers at work: few -> 2^17 (measured alone: quad wins up to there), many -> 2^13 (under 24-stream load the
  // instruction count decides; 2^11..2^13 measured best by ~1 %).  See quad_threshold().
  std::atomic<uint64_t> quad_threshold{0};
  // The load-dependent choices (kernel forms, one-pass K5 / FRI combination): -1 = by the count of provers at work
  // (six or more = loaded); 0 / 1 = stated by the caller.
  std::atomic<int> assume_loaded{-1};
  // Levels near the root are each one latency-bound launch (a lone txn proof spends ~30 % of its kernel time in them,
  // and under the 24-stream load they are 40 % of all launches, each stretched from 19 to ~120 us by sharing:
  // profiles/r2b_kernel_stats_4txn_1stream.csv, r3_kernel_stats_64txn_24streams.csv).  merkle_subtree_mx_kernel hands
  // up to seven levels of at most 2048 nodes down through LDS in one launch, in the one-set matrix-core form.
  // Measured in round 3 (profiles/r3_small_shards.txt), fused against one launch per level: 256 txns 36.2 against 35.2
  // txn-proofs/s, 32 txns 33.6 against 32.5, 16 txns 33.1 against 31.6, a lone pair of txns 150.8 against 148.2 ms.
  // (With the quad-cooperative permutation -- round 2's fused kernel, still used when the matrix-core forms are switched
  // off -- the fused form lost 0-4 %: ~12 us per level cost what the launch gaps saved.)
  // 1 = fused, 0 = one launch per level, -1 = fused only while fewer than six provers are at work.
  std::atomic<int> merkle_fused{1};
  std::atomic<int> merkle_wide{0};  // levels of up to 2^k parents go to merkle_subtree_wide_kernel (0: none)
  // launches at or above the quad threshold: 1 = matrix-core form (poseidon_mx.cuh), 0 = one lane per state
  std::atomic<int> poseidon_mx{1};
  // Sets of 16 states per wave for an mx launch: 0 = by size (mx_sets()), else 1 / 2 / 4
  std::atomic<int> poseidon_mx_sets{0};
  // the four-set kernels' 22 partial rounds: 1 = in three groups (8 + 8 + 6: 38.0-39.4 txn-proofs/s against two groups,
  // profiles/r3_poseidon_three_groups.txt), 0 = every round by itself
  std::atomic<int> poseidon_grouped{1};

  // ---- NTT (ntt.hip)
  // Matrix-core form of the block kernels (ntt_mx.cuh).  0: never; 1: 2^12- and 2^13-point blocks; 2: 2^14-point blocks
  // too (tests); 3: 2^13-point blocks -- where it wins a little -- while the device is not loaded (fewer than six
  // provers at work).  Measured (bench.py --ntt-mx 1 / 0 back to back on one box; HISTORY.md, round 2):
  //   first version, MFMA constants in 96 VGPRs, 224-240 VGPRs = two waves per SIMD (profiles/r2_ntt_mx_probe.txt,
  //   r2_ntt_mx_block_ab.txt): alone level at 2^12 points, +7 % LDE / +17 % inverse at 2^13 x 135 rate 8, -25 % at 2^14
  //   (spills); under the 24-stream block run 29.8 against 34.1 txn-proofs/s -- its fat waves crowd out the Poseidon
  //   kernels' waves;
  //   this version, constants cut to 32 VGPRs (chunk 1 = +-chunk 0, C operands in LDS), 136-168 VGPRs = three waves per
  //   SIMD (profiles/r2_ntt_mx_lean_ab.txt): alone level at 2^12, +3..4 % at 2^13 x 135, still behind at 2^14; under
  //   load 34.7 against 35.3.
  // It issues half the VALU instructions of the butterfly kernels, but every 16 elements of a pass cost one MFMA, which
  // blocks its SIMD for ~12 cycles (tools/mfma_probe.hip), and the kernel stays latency-bound at three waves: no win
  // over the VALU kernels on this workload, so it is used only where it measures ahead.
  std::atomic<int> ntt_mx{3};
  // Split form of the inverse (DIF) block kernels (Ntt16Args), out of place only: 0 = automatic, 1 = never,
  // 2 = wherever a split form exists.  See use_split().
  std::atomic<int> ntt_split{0};

  // ---- prover (prover.cpp, proofgen.cpp)
  std::atomic<int> k5_spread{0};      // measurement knob: the loaded-device spreading rule for the synthetic AIR too
  std::atomic<int> host_wait{0};      // 0: by the device's mode; 1: always the runtime's wait; 2: always poll + sleep
  std::atomic<int> host_poseidon{0};  // 0 = by the CPU, 1 = scalar form (tests)
  std::atomic<int> rec_batch{8};      // recursion proofs proved in lock-step (MAX_BATCH); 1 = one proof at a time
  std::atomic<int> witness_threads{7};  // host threads a lone prover makes its Poseidon-row witness on
  std::atomic<int> side_lanes{1};     // 0 = no side lanes, n = while at most n provers are at work

  // ---- shard scheduler (gi.cpp, rec_pool.hpp)
  // 1 = inside bp_prove_shard / bp_prove_shard_gi / bp_aggregate_proofs the root proof of a transaction and the
  // aggregation proofs are jobs that ride in the spare slot of other transactions' lock-step batches, and what is left
  // at the end of the tree is proved a batch at a time; 0 = every node is proved where it is started, one proof per
  // chain of launches (the scheduling up to this knob).  Read once per call.  Measurements: profiles/rec_riders_ab.txt.
  std::atomic<int> rec_riders{1};
  // Transactions a thread of bp_prove_shard / bp_prove_shard_gi starts at a time: it leases that many provers whose
  // arenas are neighbours (proofgen.cpp: ProverLease) and proves table t of all of them in lock-step batches wherever
  // their shapes agree (prove_tables), t = 0..6, each transaction on its own transcript; the recursion chains
  // follow (Tune::rec_group).  1 = one transaction per thread (the schedule up to this knob).  0 = by the
  // state: 3 where bp_state_build saw fewer hardware queues than the state has prover streams, else 1.  Measured on the
  // 256-txn block, 20 streams, three alternating runs each (profiles/txn_groups_ab.txt): at 4 queues 35.22 (1) / 35.39
  // (2) / 37.97 (3) txn-proofs/s -- 3 is +7.8 %, 7.8 x the parent's spread, 2 is inside it --; at 32 queues, where every
  // stream has a queue of its own, 40.04 (1) against 39.39 (3): halving the streams at work costs more there than the
  // launches save.  Read once per call.
  std::atomic<int> txn_group{0};
  // How the recursion of a group follows its table proofs (proofgen.cpp: group_recursion).  0 = level k of the seven
  // chains of ALL the group's transactions is one lock-step batch (7 g proofs and the riders that fit, MAX_LOCKSTEP at
  // most), then level k + 1: the recursion of a group costs the launches and host waits of one transaction's.  1 = one
  // transaction's recursion after the other, batches of seven and a rider (the schedule up to this knob; A/B runs and
  // tests).  A group of one is the same either way.  Read once per call.  Measurements: profiles/rec_group_ab.txt.
  std::atomic<int> rec_group{0};

  // ---- range-check multiplicities (range_mult.hip)
  // bp_range_multiplicities counts in a per-workgroup LDS histogram up to 2^k values (1 .. 14: 32-bit counters, 64 KiB at
  // 14) and with global 64-bit atomics above.  13 = 32 KiB a workgroup keeps four workgroups on a CU; the flush costs up
  // to 2^k atomics per workgroup, so the LDS form stops paying where a chunk of rows no longer outnumbers the bins.  Not
  // yet swept on hardware (profiles/air_program_log_ports.txt has the one point measured).
  std::atomic<int> range_lds_log{13};
};

Tune& tune();  // the process's one instance (tune.cpp)

}  // namespace bpg
