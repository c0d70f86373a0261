// dosage_plan.hpp — the host plan of hmc_haplotype_dosages (exact_query.hip,
// exact_haplotype_dosages).  Free of HIP and of the context so that the host
// sanitizer program (tests/sanitize/dosage_main.cpp) can drive it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <vector>

namespace hmc {

// Codes of a pattern's rows, one byte per locus of the window: an allele-table
// index of the locus (at most 43 on the exact path), "any allele", or "a symbol
// the locus's table does not hold: matches nothing".
constexpr uint32_t DOSE_ANY = 254u, DOSE_ABSENT = 255u;
enum : int32_t { DOSE_EV_EVAL = 0, DOSE_EV_ANCHOR = 2 };
struct DoseEvent {
  int32_t rec;    // the record the event happens at (head_len for loci inside the head)
  int32_t op;     // kind | slot << 2
  int32_t pat;    // the pattern: its codes, and on evaluation its output column
  int32_t start;  // the pattern's first locus
  int32_t len;    // its length
};
struct DosePlan {
  std::vector<DoseEvent> ev;
  int need = 0, rounds = 0;  // most patterns live at once; sweeps over the records
};

// Patterns (start[p], len[p]) with 0 <= start, 1 <= len, start + len <= L
// (checked by the caller), sorted by (start, end, p).  The record of locus k is
// k + 1, or head_len for k < head_len; a pattern is anchored at the record of
// its first locus and evaluated at the record of its last, which frees its
// slot.  Slots by greedy interval colouring in sorted order: the lowest of ns
// whose holder's last record is at most the pattern's first, else the first
// later round with one.  Events per round by ascending record; at a record the
// evaluations of the patterns carried in come before the anchors that start
// there, and a pattern that starts and ends at one record (length 1, or wholly
// inside the head) is evaluated right after its own anchor.
inline void dose_plan(int P, const int32_t *start, const int32_t *len, int head_len, int ns, DosePlan &pl) {
  pl.ev.clear();
  pl.need = pl.rounds = 0;
  auto rec_of = [&](int k) { return k < head_len ? head_len : k + 1; };
  std::vector<int> ord((size_t)P);
  for (int p = 0; p < P; ++p) ord[(size_t)p] = p;
  std::sort(ord.begin(), ord.end(), [&](int x, int y) {
    return std::make_tuple(start[x], start[x] + len[x], x) < std::make_tuple(start[y], start[y] + len[y], y);
  });
  struct Keyed {
    int rec, phase, at, kind, round;
    DoseEvent ev;
  };
  std::vector<Keyed> evs;
  std::vector<std::vector<int>> busy;  // [round][slot]: the record at which the slot's holder is evaluated
  std::vector<int> ends;               // the live patterns' last records
  for (size_t o = 0; o < ord.size(); ++o) {
    const int p = ord[o], ja = rec_of(start[p]), jend = rec_of(start[p] + len[p] - 1);
    ends.erase(std::remove_if(ends.begin(), ends.end(), [&](int e) { return e <= ja; }), ends.end());
    ends.push_back(jend);
    pl.need = std::max(pl.need, (int)ends.size());
    int round = -1, slot = -1;
    for (size_t r = 0; slot < 0; ++r) {
      if (r == busy.size()) busy.push_back(std::vector<int>((size_t)ns, 0));
      for (int sl = 0; sl < ns && slot < 0; ++sl)
        if (busy[r][(size_t)sl] <= ja) {
          busy[r][(size_t)sl] = jend;
          round = (int)r;
          slot = sl;
        }
    }
    pl.rounds = std::max(pl.rounds, round + 1);
    evs.push_back({ja, 1, (int)o, 0, round, {ja, DOSE_EV_ANCHOR | slot << 2, p, start[p], len[p]}});
    evs.push_back({jend, jend == ja ? 1 : 0, (int)o, 1, round, {jend, DOSE_EV_EVAL | slot << 2, p, start[p], len[p]}});
  }
  std::sort(evs.begin(), evs.end(), [](const Keyed &x, const Keyed &y) {
    return std::tie(x.round, x.rec, x.phase, x.at, x.kind) < std::tie(y.round, y.rec, y.phase, y.at, y.kind);
  });
  pl.ev.reserve(evs.size());
  for (const Keyed &k : evs) pl.ev.push_back(k.ev);
}

}  // namespace hmc
