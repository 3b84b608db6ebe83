// set_check.hpp -- the device side of both pre-flights (set_check.hip; check_tables_and_links, table_set.cpp): the balance of one link.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bpg {

// One end of a link: a port of a member's trace.
struct SetEnd {
  uint32_t air_id, port;
  const uint64_t *trace, *consts;  // as the member's bp_set_table gives them
  uint64_t stride;
  uint32_t log_n;
  uint64_t pub[4];
  uint32_t end;        // its index into link.looking; n_looking for the looked end
  bool looked;
  bool wants_bit;      // a registered program's product port or kind-1 log port: f outside {0, 1} is a bad filter
};

// A slot of the open-addressed table is 8 words: key, S (lo, hi), S1 (lo, hi), min looking (end << 40 | row), min looked
// row, one unused.  The result of a link is 8 words (SET_RES_*).
constexpr uint32_t SET_SLOT_WORDS = 8, SET_RESULT_WORDS = 8;
enum { SET_RES_UNBALANCED = 0, SET_RES_MIN_LOOKING = 1, SET_RES_MIN_LOOKED = 2, SET_RES_N_LOOKING = 3, SET_RES_N_LOOKED = 4,
       SET_RES_BAD_FILTER = 5, SET_RES_OVERFLOW = 6, SET_RES_BAD_VALUE = 7 };
constexpr uint32_t SET_LOC_ROW_BITS = 40;  // a packed (end, row): end << 40 | row
// log2 of the slots a link whose ends have `rows` rows in all gets: a power of two, at least twice the rows
uint32_t set_check_log_slots(uint64_t rows);
// The whole balance of one link into d_result (SET_RESULT_WORDS words): the table is cleared, every end inserts its rows,
// one scan reduces the slots.  ctl = beta0, gamma0, beta1, gamma1.  Nothing waits for the stream.
int launch_set_link(const SetEnd* ends, uint32_t n_ends, const uint64_t ctl[4], uint64_t* d_table, uint32_t log_slots, uint64_t* d_result,
                    hipStream_t st);
// d_result[SET_RES_BAD_VALUE] = the filter of end `e` at `row`
int launch_set_filter_at(const SetEnd& e, uint64_t row, const uint64_t ctl[4], uint64_t* d_result, hipStream_t st);

}  // namespace bpg
