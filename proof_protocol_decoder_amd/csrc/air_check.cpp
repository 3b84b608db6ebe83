// air_check.cpp -- the AIR trace checker's host pass and C ABI (include/bpg.h, bp_air_check_trace*).
//
// The device pass (air_check.hip) says WHICH rows of a trace violate the AIR; this file says which constraints: rows
// i and i + 1 (and the constants of row i) are re-evaluated with the host instantiation of air::eval_unit -- the
// verifier's field policy (air.hpp, Ops<gl::Ext>) on base-field words, whose second coordinate stays zero -- into a
// consumer that ACCUMULATES BY CONSTRAINT INDEX: a unit may emit partial sums of one constraint several times, so only
// the per-index sum is a constraint's value.  Every non-zero index of the AIR's own list is a violation.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>
#include "air_check.hpp"
#include "air_program.hpp"
#include "caller_table.hpp"

using namespace bpg;
using gl::Ext;

namespace {

struct HostRow {  // one row on the host; the auxiliary columns read as zero (the AIR's own values do not use them)
  const uint64_t *loc_, *nxt_, *cst_;
  uint64_t xv;
  const uint64_t* pub_;
  Ext x() const { return gl::ext(xv); }
  uint64_t pub(uint32_t j) const { return pub_[j]; }
  Ext loc(uint32_t c) const { return gl::ext(loc_[c]); }
  Ext nxt(uint32_t c) const { return gl::ext(nxt_[c]); }
  Ext cst(uint32_t k) const { return gl::ext(cst_[k]); }
  Ext aux(uint32_t) const { return gl::ext(0); }
  Ext aux_nxt(uint32_t) const { return gl::ext(0); }
};
struct IndexEmit {  // per-index sums of the AIR's own constraints, the trace domain's selectors as 0 / 1
  std::vector<Ext>& v;
  uint32_t T;
  bool tr, fi, la;
  void all(uint32_t idx, Ext c) {
    if (idx < T) v[idx] = gl::add(v[idx], c);
  }
  void transition(uint32_t idx, Ext c) { if (tr) all(idx, c); }
  void first(uint32_t idx, Ext c) { if (fi) all(idx, c); }
  void last(uint32_t idx, Ext c) { if (la) all(idx, c); }
  void emit(uint32_t kind, uint32_t idx, Ext c) {  // the four by a run-time kind (air_program.hpp)
    kind == 0 ? all(idx, c) : kind == 1 ? transition(idx, c) : kind == 2 ? first(idx, c) : last(idx, c);
  }
};

struct Checker {
  air::Shape shape;
  uint32_t log_n, T, n_units;
  uint64_t pub[4] = {0, 0, 0, 0};
  bp_air_desc desc;
  std::shared_ptr<const air::prog::Program> program;  // a registered id: its program, interpreted (air_program.hpp)
  // v[idx] = the value of constraint idx at row i (loc = row i, nxt = row i + 1, cst = constants of row i)
  void eval_row(uint32_t i, const uint64_t* loc, const uint64_t* nxt, const uint64_t* cst, std::vector<Ext>& v) const {
    const uint32_t last = (1u << log_n) - 1;
    v.assign(T, gl::ext(0));
    IndexEmit e{v, T, i != last, i == 0, i == last};
    const HostRow row{loc, nxt, cst, shape.air_id == air::PLONK || program ? gl::pow(gl::root(log_n), i) : 0, pub};
    const uint64_t ctl[4] = {0, 0, 0, 0};
    if (program)
      for (uint32_t u = 0; u < n_units; u++) program->eval_unit<Ext>(u, row, e);
    else
      for (uint32_t u = 0; u < n_units; u++) air::eval_unit<Ext>(shape, u, T, ctl, row, e);
  }
  void family_of(uint32_t idx, uint32_t* family, uint32_t* kind) const {
    if (shape.air_id == air::SYNTHETIC) {  // interleaved: 3g all rows, 3g + 1 transition, 3g + 2 first row
      *family = *kind = idx % 3;
      return;
    }
    for (uint32_t f = 0; f < desc.n_families; f++)
      if (idx >= desc.families[f].first_index && idx < desc.families[f].first_index + desc.families[f].count) {
        *family = f;
        *kind = desc.families[f].kind;
        return;
      }
    *family = *kind = ~0u;
  }
  // the violations of row i, appended (at most max_viol in `out`); returns how many the row has
  uint32_t report_row(uint32_t i, const uint64_t* loc, const uint64_t* nxt, const uint64_t* cst, bp_air_violation* out,
                      uint32_t max_viol, uint32_t* n_out) const {
    std::vector<Ext> v;
    eval_row(i, loc, nxt, cst, v);
    uint32_t found = 0;
    for (uint32_t idx = 0; idx < T; idx++) {
      if (v[idx].c0 == 0 && v[idx].c1 == 0) continue;
      found++;
      if (*n_out < max_viol) {
        bp_air_violation& w = out[(*n_out)++];
        w.row = i;
        w.constraint = idx;
        family_of(idx, &w.family, &w.kind);
        w.value = v[idx].c0;
      }
    }
    return found;
  }
};

int make_checker(const char* who, uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* trace, uint64_t stride,
                 const uint64_t* consts, const uint64_t pub[4], uint32_t max_rows, const uint64_t* n_violated_rows,
                 const uint32_t* rows_out, const bp_air_violation* viol_out, uint32_t max_viol, const uint32_t* n_viol,
                 Checker* k) {
  if (!shape) return fail(BP_ERR_INVALID_INPUT, "%s: null shape", who);
  // the shape is validated exactly as bp_quotient_eval's
  const StarkCfg c = to_cfg(*shape, air_id);
  int rc = check_cfg(c);
  if (rc) return rc;
  if (!n_violated_rows || !n_viol || (max_rows && !rows_out) || (max_viol && !viol_out))
    return fail(BP_ERR_INVALID_INPUT, "%s: null argument", who);
  CallerTable t = caller_table(c, trace, stride, consts, pub);
  if (air::prog::is_registered(air_id) && !t.program) return fail(BP_ERR_INVALID_INPUT, "%s: AIR program 0x%08x was unregistered", who, air_id);
  if (!t.reads_public()) t.pub = nullptr;  // public inputs the AIR does not read are not looked at
  if ((rc = check_caller_table(who, "", t))) return rc;
  k->program = t.program;
  if (t.pub)
    for (int j = 0; j < 4; j++) k->pub[j] = t.pub[j];
  k->shape = air::Shape{air_id, c.n_cols, c.n_const, c.deg_pow};
  k->log_n = c.log_n;
  k->T = air::any_n_constraints(k->shape);
  k->n_units = air::any_n_units(k->shape);
  if ((rc = bp_air_describe(air_id, c.n_cols, c.n_const, c.deg_pow, &k->desc))) return rc;
  return BP_OK;
}

}  // namespace

extern "C" {

int bp_air_check_trace_host(uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* trace, uint64_t stride,
                            const uint64_t* consts, const uint64_t pub[4], uint32_t max_rows, uint64_t* n_violated_rows,
                            uint32_t* rows_out, bp_air_violation* viol_out, uint32_t max_viol, uint32_t* n_viol) try {
  Checker k;
  int rc = make_checker("bp_air_check_trace_host", air_id, shape, trace, stride, consts, pub, max_rows, n_violated_rows,
                        rows_out, viol_out, max_viol, n_viol, &k);
  if (rc) return rc;
  const uint32_t n = 1u << k.log_n, C = k.shape.n_cols, K = k.shape.n_const;
  // every row, per index (exact: no fold), on up to 16 threads
  std::vector<uint8_t> bad(n, 0);
  const uint32_t n_thr = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), n / 64 + 1}));
  auto work = [&](uint32_t t) {
    std::vector<uint64_t> loc(C), nxt(C), cst(K);
    std::vector<Ext> v;
    for (uint32_t i = t; i < n; i += n_thr) {
      const uint32_t j = (i + 1) & (n - 1);
      for (uint32_t col = 0; col < C; col++) {
        loc[col] = trace[(uint64_t)col * stride + i];
        nxt[col] = trace[(uint64_t)col * stride + j];
      }
      for (uint32_t q = 0; q < K; q++) cst[q] = consts[(uint64_t)q * n + i];
      k.eval_row(i, loc.data(), nxt.data(), cst.data(), v);
      for (const Ext& e : v)
        if (e.c0 | e.c1) {
          bad[i] = 1;
          break;
        }
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < n_thr; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  uint64_t total = 0;
  uint32_t n_rows = 0, nv = 0, found = 0;
  std::vector<uint64_t> loc(C), nxt(C), cst(K);
  for (uint32_t i = 0; i < n; i++) {
    if (!bad[i]) continue;
    total++;
    if (n_rows >= max_rows) continue;
    rows_out[n_rows++] = i;
    const uint32_t j = (i + 1) & (n - 1);
    for (uint32_t col = 0; col < C; col++) {
      loc[col] = trace[(uint64_t)col * stride + i];
      nxt[col] = trace[(uint64_t)col * stride + j];
    }
    for (uint32_t q = 0; q < K; q++) cst[q] = consts[(uint64_t)q * n + i];
    found += k.report_row(i, loc.data(), nxt.data(), cst.data(), viol_out, max_viol, &nv);
  }
  *n_violated_rows = total;
  *n_viol = found;
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_check_trace_host")

int bp_air_check_trace(uint32_t air_id, const bp_stark_cfg* shape, const uint64_t* d_trace, uint64_t stride,
                       const uint64_t* d_consts, const uint64_t pub[4], uint32_t max_rows, uint64_t* n_violated_rows,
                       uint32_t* rows_out, bp_air_violation* viol_out, uint32_t max_viol, uint32_t* n_viol, void* stream) try {
  Checker k;
  int rc = make_checker("bp_air_check_trace", air_id, shape, d_trace, stride, d_consts, pub, max_rows, n_violated_rows,
                        rows_out, viol_out, max_viol, n_viol, &k);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const uint32_t n = 1u << k.log_n, C = k.shape.n_cols, K = k.shape.n_const, words = (n + 63) / 64;
  CheckArgs a{};
  a.trace = d_trace; a.consts = K ? d_consts : nullptr; a.stride = stride;
  a.air_id = air_id; a.log_n = k.log_n; a.n_cols = C; a.n_const = K; a.deg_pow = k.shape.deg_pow; a.T = k.T;
  for (int j = 0; j < 4; j++) a.pub[j] = k.pub[j];
  FreshChallenges fresh;
  a.alpha0 = fresh();
  a.alpha1 = fresh();
  const uint64_t partial = air_check_partial_words(a);
  // (a test / integration entry: its scratch is a buffer of its own) apow | count | bitmap | partial folds
  const uint64_t scratch_words = 2 * (uint64_t)k.T + 1 + words + partial;
  DeviceBuf scratch, rows_buf, out_buf;
  BPG_HIP(hipMalloc(&scratch.p, scratch_words * 8));
  uint64_t* d_s = scratch.as<uint64_t>();
  a.apow = d_s;
  a.count = reinterpret_cast<unsigned long long*>(d_s + 2 * (uint64_t)k.T);
  a.bitmap = d_s + 2 * (uint64_t)k.T + 1;
  a.partial = partial ? a.bitmap + words : nullptr;
  if ((rc = launch_air_check(a, st))) return rc;
  unsigned long long count = 0;
  BPG_HIP(hipMemcpyAsync(&count, a.count, 8, hipMemcpyDeviceToHost, st));
  BPG_HIP(hipStreamSynchronize(st));
  *n_violated_rows = count;
  *n_viol = 0;
  if (!count || !max_rows) return BP_OK;
  // the first max_rows violated rows in row order, then their rows i, i + 1 (and constants of row i) to the host
  std::vector<uint64_t> bitmap(words);
  BPG_HIP(hipMemcpy(bitmap.data(), a.bitmap, (size_t)words * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> rows;
  for (uint32_t w = 0; w < words && rows.size() < max_rows; w++)
    for (uint64_t b = bitmap[w]; b && rows.size() < max_rows; b &= b - 1) rows.push_back(64 * w + (uint32_t)__builtin_ctzll(b));
  uint32_t nv = 0, found = 0;
  constexpr uint32_t BATCH = 256;  // rows per gather (grid.y)
  std::vector<uint32_t> want;
  std::vector<uint64_t> got;
  BPG_HIP(hipMalloc(&rows_buf.p, 2 * BATCH * 4));
  BPG_HIP(hipMalloc(&out_buf.p, (size_t)2 * BATCH * (C + K) * 8));
  uint32_t* d_rows = rows_buf.as<uint32_t>();
  uint64_t* d_out = out_buf.as<uint64_t>();
  for (size_t r0 = 0; r0 < rows.size(); r0 += BATCH) {
    const uint32_t m = (uint32_t)std::min<size_t>(BATCH, rows.size() - r0);
    want.clear();
    for (uint32_t j = 0; j < m; j++) want.push_back(rows[r0 + j]);
    for (uint32_t j = 0; j < m; j++) want.push_back((rows[r0 + j] + 1) & (n - 1));
    BPG_HIP(hipMemcpyAsync(d_rows, want.data(), want.size() * 4, hipMemcpyHostToDevice, st));
    if ((rc = launch_gather_rows(d_trace, stride, C, d_rows, 2 * m, d_out, st))) return rc;
    if (K && (rc = launch_gather_rows(d_consts, n, K, d_rows, m, d_out + (size_t)2 * m * C, st))) return rc;
    got.resize((size_t)2 * m * C + (size_t)m * K);
    BPG_HIP(hipMemcpyAsync(got.data(), d_out, got.size() * 8, hipMemcpyDeviceToHost, st));
    BPG_HIP(hipStreamSynchronize(st));
    for (uint32_t j = 0; j < m; j++)
      found += k.report_row(want[j], got.data() + (size_t)j * C, got.data() + (size_t)(m + j) * C,
                            got.data() + (size_t)2 * m * C + (size_t)j * K, viol_out, max_viol, &nv);
  }
  const uint32_t n_rows = (uint32_t)rows.size();
  std::memcpy(rows_out, rows.data(), (size_t)n_rows * 4);
  *n_viol = found;
  return BP_OK;
}
BPG_ABI_CATCH("bp_air_check_trace")

}  // extern "C"
