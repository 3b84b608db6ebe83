// txn_tables.hpp -- the seven tables of a transaction as DATA, and the host-only code that reads it (txn_tables.cpp): the
// IR encoder and its flag setters, parse_ir, the plan of a transaction's traces, the lookup check, the table proofs' verifier.
#pragma once
#include <vector>
#include "prover.hpp"

namespace bpg {
namespace txn {

// a table's position in a transaction: upstream's order (prover_state.rs:85-93)
enum : int { T_ARITHMETIC = 0, T_BYTE_PACKING, T_CPU, T_KECCAK, T_KECCAK_SPONGE, T_LOGIC, T_MEMORY };

// one AIR that can prove a table instead of the synthetic one: the bit of IR word 1 that selects it (0: no such AIR, the
// list ends here), what messages call it, its public setter (include/bpg.h)
struct TableAir { uint32_t air_id; uint64_t ir_mask; const char *noun, *setter; };
// One row per table: everything about it that is data, once.  Its width under an AIR is air::DESC[air_id].n_cols.
// air::ctl::pairs() (air.hpp) names tables and their AIRs by the same positions and ids in literals of its own: the two
// must agree (tests/test_txn_tables.py holds each pair's sides against these rows).
struct Table {
  const char* name;
  TableAir airs[2];  // airs[0]: the table's AIR, the one witness data and the BP_GI_* flag go with
  uint32_t item_words, rows_per_item;  // a witness item; a table of N rows holds ceil(N / rows_per_item) of them
  const uint64_t* bp_txn_witness::*data; size_t bp_txn_witness::*n; int bp_txn_witness::*has;  // the members that carry its items
  uint32_t gi_flag;  // the BP_GI_* flag that asks for airs[0], or 0
};
constexpr Table TABLES[BP_NUM_TABLES] = {
    {"arithmetic", {{air::ARITHMETIC, 0x800, "arithmetic", "bp_ir_set_arithmetic_air"},
                    {air::ARITHMETIC_MUL, 0x4000, "multiplication", "bp_ir_set_arithmetic_mul_air"}},
     9, 1, &bp_txn_witness::arithmetic_ops, &bp_txn_witness::n_arithmetic_ops, &bp_txn_witness::has_arithmetic, 0},
    {"byte_packing", {{air::BYTE_PACKING, 0x1000, "byte-packing", "bp_ir_set_byte_packing_air"}},
     6, 1, &bp_txn_witness::byte_sequences, &bp_txn_witness::n_byte_sequences, &bp_txn_witness::has_byte_packing, BP_GI_BYTE_PACKING_AIR},
    {"cpu", {}, 0, 1, nullptr, nullptr, nullptr, 0},
    {"keccak", {{air::KECCAK_F, 0x100, "Keccak-f", "bp_ir_set_keccak_air"}},
     25, 24, &bp_txn_witness::keccak_inputs, &bp_txn_witness::n_perms, &bp_txn_witness::has_keccak, BP_GI_KECCAK_AIR},
    {"keccak_sponge", {{air::KECCAK_SPONGE, 0x2000, "Keccak sponge", "bp_ir_set_keccak_sponge_air"}},
     44, 1, &bp_txn_witness::sponge_rows, &bp_txn_witness::n_sponge_rows, &bp_txn_witness::has_keccak_sponge, BP_GI_KECCAK_SPONGE_AIR},
    {"logic", {{air::LOGIC, 0x200, "logic", "bp_ir_set_logic_air"}},
     9, 1, &bp_txn_witness::logic_ops, &bp_txn_witness::n_logic_ops, &bp_txn_witness::has_logic, BP_GI_LOGIC_AIR},
    {"memory", {{air::MEMORY, 0x400, "memory", "bp_ir_set_memory_air"}},
     11, 1, &bp_txn_witness::memory_log, &bp_txn_witness::n_memory_ops, &bp_txn_witness::has_memory, BP_GI_MEMORY_AIR},
};
// the AIR of table t that IR word 1 selects, or nullptr
constexpr const TableAir* air_selected(int t, uint64_t ir_word1) {
  for (const TableAir& a : TABLES[t].airs)
    if (a.ir_mask & ir_word1) return &a;
  return nullptr;
}
constexpr bool table_has_air(int t, uint32_t air_id) {
  for (const TableAir& a : TABLES[t].airs)
    if (a.ir_mask && a.air_id == air_id) return true;
  return false;
}
// items a table of N rows holds (the last Keccak permutation may be cut)
constexpr size_t witness_capacity(int t, uint64_t N) { return (size_t)((N + TABLES[t].rows_per_item - 1) / TABLES[t].rows_per_item); }

constexpr uint64_t IR_MAGIC = 0x52494E5854475042ULL;      // "BPGTXNIR"
constexpr uint64_t TABLES_MAGIC = 0x534C424154475042ULL;  // "BPGTABLS"

inline StarkCfg table_cfg_of(const bp_config& c, uint32_t log_n, uint32_t width) {
  return StarkCfg{log_n, width, 0, 1, c.stark_rate_bits, c.stark_cap_height, c.stark_num_queries,
                  c.stark_pow_bits, c.arity_bits, c.final_poly_bits};
}
void root_after(const uint64_t root_before[4], uint64_t seed, uint64_t txn_number, uint64_t out[4]);
// one setter for all: airs[which] of table t, on or off
int ir_set_air(uint64_t ir[BP_IR_WORDS], int t, int which, int on);

// Witness data given by the caller instead of drawn from the seed, per table (bp_txn_witness): in[t] nullable, n[t]
// items of TABLES[t].item_words words; the table must carry its AIR flag.
struct TxnWitness {
  const uint64_t* in[BP_NUM_TABLES] = {};
  size_t n[BP_NUM_TABLES] = {};
  void give(int t, const uint64_t* p, size_t count);  // p nullable when count is 0
};
int witness_of(const bp_txn_witness* data /*nullable: nothing is given*/, TxnWitness* wit);
// The table's full input array (capacity x words): the caller's items, then padding -- permutations of the all-zero state
// (as upstream pads its Keccak table), rows without an operation, and for the memory log reads of the last address at
// later and later times (a memory that is left alone).
void fill_table_inputs(int t, uint64_t N, const uint64_t* in, size_t n, uint64_t* dst);
// whether table t is made from the caller's data (its AIR flag set and data given)
bool given_table(const TxnWitness* wit, const StarkCfg tcfg[BP_NUM_TABLES], int t);
int parse_ir(const bp_config& cfg, const uint64_t* I, const TxnWitness* wit, StarkCfg tcfg[BP_NUM_TABLES], std::vector<uint64_t>* pv_out);

// air::ctl::pairs() by index
enum : uint32_t { L_SPONGE_KECCAK = 0, L_PACKING_MEMORY = 1, L_SPONGE_LOGIC = 2 };
// a lookup exists where both of its tables are proven with their AIRs (a synthetic table has nothing to look up)
inline bool pair_active(const StarkCfg tcfg[BP_NUM_TABLES], const air::ctl::Pair& p) {
  return tcfg[p.looking_table].air_id == p.looking_air && tcfg[p.looked_table].air_id == p.looked_air;
}
// What build_traces (proofgen.cpp) decides before it allocates, stages or launches anything, with the refusals of witness
// combinations that cannot be one statement.  given[t] as given_table says, n_given[t] the items of a given table (else 0).
struct TracePlan {
  bool lookup[air::ctl::N_PAIRS];
  uint32_t logic_covered;     // sponge rows whose five XORs are the logic table's first rows
  uint32_t sponge_row_limit;  // rows the seeded sponge table may absorb a block in (~0u: all of them)
};
int plan_traces(const StarkCfg tcfg[BP_NUM_TABLES], const bool given[BP_NUM_TABLES], const size_t n_given[BP_NUM_TABLES], TracePlan* out);

// The active lookups as links over the table indices 0 .. 6 -- the form a table set's links have (caller_table.hpp) --
// in pairs() order; pair[k]: the pair that link k is.  Returns how many.  (A lookup that is not active leaves its
// sponge ports unlinked: legal here, refused for a public set.)
uint32_t links_of(const StarkCfg tcfg[BP_NUM_TABLES], bp_set_link links[air::ctl::N_PAIRS], uint32_t pair[air::ctl::N_PAIRS]);
int check_lookups(const StarkCfg tcfg[BP_NUM_TABLES], const std::vector<uint64_t> proof[BP_NUM_TABLES]);

}  // namespace txn
}  // namespace bpg
