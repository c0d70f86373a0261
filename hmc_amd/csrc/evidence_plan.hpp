// evidence_plan.hpp — the host plan of hmc_map_phase_given (exact_query.hip,
// exact_map_phase_given) and the evidence file reader of hmc_resolve
// --evidence.  Free of HIP and of the context so that the host sanitizer
// program (tests/sanitize/evidence_main.cpp) can drive it.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <istream>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

namespace hmc {

// One constrained locus of an individual: the allele with table index
// code >> 8 lies on the first haplotype of the phase set the locus belongs to.
// GIVEN_EV_ANCHOR marks a set's first locus, GIVEN_EV_LAST its last.
enum : int32_t { GIVEN_EV_ANCHOR = 1, GIVEN_EV_LAST = 2 };
struct GivenEvent {
  int32_t locus;
  int32_t code;  // flags | allele index << 8
};
struct EvidencePlan {
  std::vector<unsigned long long> off;  // [i1 - i0 + 1] over the shard's individuals
  std::vector<GivenEvent> ev;           // per individual ascending in locus
  int n_constrained = 0;                // individuals with at least one event
};
enum : int { EVP_OK = 0, EVP_EARG = 1, EVP_EUNSUPPORTED = 2 };

// The caller's entries (ev_indiv, ev_locus, ev_set, ev_first)[n_ev] against
// the panel al[N][2][L] (symbols, -1 missing).  Every ev_indiv must lie in
// [0, N); beyond that, entries of individuals outside the shard [i0, i1) or not
// asked for (asked[i - i0] == 0; asked may be NULL: all) are ignored.  The
// others are checked in entry order, so that msg names the first offending
// one: locus in [0, L), both input alleles present and different there,
// ev_first one of the two, no earlier entry for the same (individual, locus).
// Then per individual: sets of one locus constrain nothing and are dropped; the
// others sorted by first locus must not overlap in [first locus, last locus]
// (EVP_EUNSUPPORTED, msg names the individual and the two sets).  The events are
// the remaining entries by ascending locus — a set's are consecutive.
// index_of(locus, symbol): the allele-table index of a symbol present at the locus.
template <class IndexOf>
inline int evidence_plan(int N, int L, const int32_t *al, int i0, int i1, const char *asked, int64_t n_ev, const int32_t *ev_indiv,
                         const int32_t *ev_locus, const int32_t *ev_set, const int32_t *ev_first, IndexOf index_of,
                         EvidencePlan &pl, std::string &msg) {
  const int n = std::max(0, i1 - i0);
  pl.off.assign((size_t)n + 1, 0);
  pl.ev.clear();
  pl.n_constrained = 0;
  msg.clear();
  auto entry = [](int64_t e) { return "evidence entry " + std::to_string((long long)e) + ": "; };
  struct Kept {
    int32_t indiv, locus, set, first;
  };
  std::vector<Kept> kept;
  std::set<std::pair<int32_t, int32_t>> seen;
  for (int64_t e = 0; e < n_ev; ++e) {
    const int32_t i = ev_indiv[e], k = ev_locus[e], f = ev_first[e];
    if (i < 0 || i >= N) {
      msg = entry(e) + "individual " + std::to_string(i) + " is outside the panel [0, " + std::to_string(N) + ")";
      return EVP_EARG;
    }
    if (i < i0 || i >= i1 || (asked && !asked[i - i0])) continue;
    if (k < 0 || k >= L) {
      msg = entry(e) + "locus " + std::to_string(k) + " is outside [0, " + std::to_string(L) + ")";
      return EVP_EARG;
    }
    const int32_t a0 = al[((size_t)i * 2) * L + k], a1 = al[((size_t)i * 2 + 1) * L + k];
    if (a0 < 0 || a1 < 0 || a0 == a1) {
      msg = entry(e) + "locus " + std::to_string(k) + " of individual " + std::to_string(i) + " is not heterozygous in the input";
      return EVP_EARG;
    }
    if (f != a0 && f != a1) {
      msg = entry(e) + "allele " + std::to_string(f) + " is neither input allele (" + std::to_string(a0) + ", " + std::to_string(a1) +
            ") of individual " + std::to_string(i) + " at locus " + std::to_string(k);
      return EVP_EARG;
    }
    if (!seen.insert({i, k}).second) {
      msg = entry(e) + "locus " + std::to_string(k) + " of individual " + std::to_string(i) + " has an earlier entry";
      return EVP_EARG;
    }
    kept.push_back({i, k, ev_set[e], f});
  }
  std::sort(kept.begin(), kept.end(), [](const Kept &x, const Kept &y) { return std::tie(x.indiv, x.locus) < std::tie(y.indiv, y.locus); });
  struct Span {
    int32_t first, last, set, count;
  };
  std::vector<Span> spans;
  std::map<int32_t, size_t> by_name;
  size_t p = 0;
  for (int i = 0; i < n; ++i) {
    const size_t b = p;
    while (p < kept.size() && kept[p].indiv == i0 + i) ++p;
    spans.clear();
    by_name.clear();
    for (size_t q = b; q < p; ++q) {  // loci ascending: a set's first entry is its first locus
      auto it = by_name.find(kept[q].set);
      if (it == by_name.end()) {
        by_name[kept[q].set] = spans.size();
        spans.push_back({kept[q].locus, kept[q].locus, kept[q].set, 1});
      } else {
        spans[it->second].last = kept[q].locus;
        ++spans[it->second].count;
      }
    }
    spans.erase(std::remove_if(spans.begin(), spans.end(), [](const Span &s) { return s.count < 2; }), spans.end());
    for (size_t s = 1; s < spans.size(); ++s)  // (in order of first locus already)
      if (spans[s].first < spans[s - 1].last) {
        msg = "individual " + std::to_string(i0 + i) + ": phase sets " + std::to_string(spans[s - 1].set) + " and " +
              std::to_string(spans[s].set) + " interleave (loci [" + std::to_string(spans[s - 1].first) + ", " +
              std::to_string(spans[s - 1].last) + "] and [" + std::to_string(spans[s].first) + ", " + std::to_string(spans[s].last) + "])";
        pl.ev.clear();
        return EVP_EUNSUPPORTED;
      }
    for (size_t q = b; q < p; ++q) {
      const auto it = by_name.find(kept[q].set);
      const Span *sp = nullptr;
      for (const Span &s : spans)
        if (s.set == it->first) sp = &s;
      if (!sp) continue;  // a set of one locus
      const int32_t flags = (kept[q].locus == sp->first ? GIVEN_EV_ANCHOR : 0) | (kept[q].locus == sp->last ? GIVEN_EV_LAST : 0);
      pl.ev.push_back({kept[q].locus, flags | (int32_t)index_of((int)kept[q].locus, kept[q].first) << 8});
    }
    pl.off[(size_t)i + 1] = pl.ev.size();
    pl.n_constrained += pl.off[(size_t)i + 1] > pl.off[(size_t)i];
  }
  return EVP_OK;
}

// The evidence file of hmc_resolve --evidence: empty lines and '#' lines are
// skipped; any other line reads, tab-separated,
//     Id  Marker  Set  Allele
// with the individual's id and the marker's name as the genotype files give
// them, an integer naming the phase set, and the allele on the set's first
// haplotype spelled as the genotype files spell alleles (one character at an
// 'S' locus, an integer at an 'M' locus).  PHASE files give ids that start
// with '#': a line of four fields whose first is an individual's id is an
// entry even then, so '#' starts a comment on every other line.
struct EvidenceTable {
  std::vector<int32_t> indiv, locus, set, first;
};
// 0 on success; otherwise err names the line.
inline int parse_evidence(std::istream &in, const std::vector<std::string> &ids, const std::vector<std::string> &markers,
                          const std::string &types, EvidenceTable &out, std::string &err) {
  std::map<std::string, int32_t> id_of, marker_of;
  for (size_t i = ids.size(); i-- > 0;) id_of[ids[i]] = (int32_t)i;  // (the first of equal names wins)
  for (size_t k = markers.size(); k-- > 0;) marker_of[markers[k]] = (int32_t)k;
  std::string line;
  int lineno = 0;
  auto bad = [&](const std::string &what) {
    err = "evidence file line " + std::to_string(lineno) + ": " + what;
    return 1;
  };
  while (std::getline(in, line)) {
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    std::vector<std::string> tok;
    size_t b = 0;
    while (true) {
      const size_t t = line.find('\t', b);
      tok.push_back(line.substr(b, t == std::string::npos ? std::string::npos : t - b));
      if (t == std::string::npos) break;
      b = t + 1;
    }
    if (line[0] == '#' && !(tok.size() == 4 && id_of.count(tok[0]))) continue;
    if (tok.size() != 4) return bad("expected four tab-separated fields: Id Marker Set Allele");
    const auto ii = id_of.find(tok[0]);
    if (ii == id_of.end()) return bad("no individual '" + tok[0] + "'");
    const auto mi = marker_of.find(tok[1]);
    if (mi == marker_of.end()) return bad("no marker '" + tok[1] + "'");
    errno = 0;
    char *end = nullptr;
    const long long sv = tok[2].empty() ? 0 : strtoll(tok[2].c_str(), &end, 10);
    if (tok[2].empty() || *end || errno || sv < INT32_MIN || sv > INT32_MAX) return bad("set '" + tok[2] + "' is no 32-bit integer");
    const int32_t k = mi->second;
    int32_t sym;
    if ((size_t)k < types.size() && types[(size_t)k] == 'S') {
      if (tok[3].size() != 1) return bad("allele '" + tok[3] + "' at marker '" + tok[1] + "' is not one character");
      sym = (int32_t)(unsigned char)tok[3][0];
    } else {
      errno = 0;
      const long long v = tok[3].empty() ? -1 : strtoll(tok[3].c_str(), &end, 10);
      if (tok[3].empty() || *end || errno || v < 0 || v > INT32_MAX) return bad("allele '" + tok[3] + "' at marker '" + tok[1] + "' is no integer");
      sym = (int32_t)v;
    }
    out.indiv.push_back(ii->second);
    out.locus.push_back(k);
    out.set.push_back((int32_t)sv);
    out.first.push_back(sym);
  }
  return 0;
}

}  // namespace hmc
