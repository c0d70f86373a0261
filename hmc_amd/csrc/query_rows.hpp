// query_rows.hpp — the map between a posterior query's caller rows and the
// individuals of the rank's shard (ctx_query.cpp).  Free of HIP and of the
// context so that the host sanitizer program (tests/sanitize/dosage_main.cpp)
// can drive it.
#pragma once
#include <cstdint>
#include <vector>

namespace hmc {

// Rows are the caller's: entry q asks for individual indiv[q] of the shard
// [i0, i1), or for individual i0 + q when no list is given (the whole shard).
// An individual asked for twice is computed once and copied to both rows.
struct QueryRows {
  const int32_t *indiv = nullptr;
  int i0 = 0;
  std::vector<int64_t> row_off, rows;  // CSR over the shard's individuals: the caller's rows that ask for each
  std::vector<char> asked;             // [shard] the individual has rows
  std::vector<int32_t> status;         // [shard] 1 until the individual's group has run

  // The map of n entries (n >= 0; list NULL: n is the shard's size).  -1, or
  // the position of the first entry outside the shard; the map is then not built.
  int64_t build(int64_t n, const int32_t *list, int shard_i0, int shard_i1) {
    for (int64_t q = 0; list && q < n; ++q)
      if (list[q] < shard_i0 || list[q] >= shard_i1) return q;
    indiv = list;
    i0 = shard_i0;
    const int nl = shard_i1 - shard_i0;
    row_off.assign((size_t)nl + 1, 0);
    for (int64_t q = 0; q < n; ++q) ++row_off[(size_t)local(q) + 1];
    for (int i = 0; i < nl; ++i) row_off[(size_t)i + 1] += row_off[(size_t)i];
    rows.assign((size_t)n, 0);
    std::vector<int64_t> at(row_off.begin(), row_off.end() - 1);
    for (int64_t q = 0; q < n; ++q) rows[(size_t)at[(size_t)local(q)]++] = q;
    asked.assign((size_t)nl, 0);  // the passes run over the individuals asked for, not the whole shard
    for (int i = 0; i < nl; ++i) asked[(size_t)i] = row_off[(size_t)i + 1] > row_off[(size_t)i];
    status.assign((size_t)nl, 1);
    return -1;
  }
  int64_t size() const { return (int64_t)rows.size(); }
  int local(int64_t q) const { return indiv ? indiv[q] - i0 : (int)q; }  // the shard individual of caller row q
  // the caller rows of shard individual i: rows[begin(i) .. end(i)), ascending
  int64_t begin(int i) const { return row_off[(size_t)i]; }
  int64_t end(int i) const { return row_off[(size_t)i + 1]; }
};

}  // namespace hmc
