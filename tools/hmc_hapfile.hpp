// hmc_hapfile.hpp — the haplotype list of hmc_resolve --haplotypes HAPFILE: the
// patterns of hmc_haplotype_dosages as text.  Header-only and free of the
// C-ABI so that the host sanitizer program can drive it.
//
// '#' lines and empty lines are skipped; any other line reads
//     name start a a a ... [| b b b ...]
// start is the 0-based first locus; alleles are spelled as the genotype files
// spell them (one character at an 'S' locus, an integer at an 'M' locus), '?'
// means any allele; the optional B row after '|' has the length of the A row.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <istream>
#include <sstream>
#include <string>
#include <vector>

namespace hmc_cli {

struct HapList {
  std::vector<std::string> names;
  std::vector<int32_t> start, len;
  std::vector<std::vector<int32_t>> a, b;  // symbols, -1 = any
  bool two_sided = false;                  // some line has a B row
  int maxlen = 1;
  // [P][maxlen] padded with -1
  std::vector<int32_t> padded(bool row_b) const {
    std::vector<int32_t> out(names.size() * (size_t)maxlen, -1);
    for (size_t p = 0; p < names.size(); ++p) {
      const std::vector<int32_t> &r = row_b ? b[p] : a[p];
      for (size_t k = 0; k < r.size(); ++k) out[p * (size_t)maxlen + k] = r[k];
    }
    return out;
  }
};

// types[L]: 'S' or 'M' per locus.  0 on success; otherwise err names the line.
inline int parse_hapfile(std::istream &in, const std::string &types, HapList &out, std::string &err) {
  const int L = (int)types.size();
  std::string line;
  int lineno = 0;
  auto bad = [&](const std::string &what) {
    err = "haplotype file line " + std::to_string(lineno) + ": " + what;
    return 1;
  };
  while (std::getline(in, line)) {
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty() || tok[0][0] == '#') continue;
    if (tok.size() < 3) return bad("expected: name start allele ... [| allele ...]");
    errno = 0;
    char *end = nullptr;
    const long st = strtol(tok[1].c_str(), &end, 10);
    if (*end || errno || st < 0 || st >= L) return bad("start '" + tok[1] + "' is no locus in [0, " + std::to_string(L) + ")");
    std::vector<int32_t> rows[2];
    int side = 0;
    for (size_t i = 2; i < tok.size(); ++i) {
      const std::string &t = tok[i];
      if (t == "|") {
        if (side == 1) return bad("more than one '|'");
        side = 1;
        continue;
      }
      const long k = st + (long)rows[side].size();
      if (k >= L) return bad("the window passes the last locus " + std::to_string(L - 1));
      int32_t sym;
      if (t == "?") sym = -1;
      else if (types[(size_t)k] == 'S') {
        if (t.size() != 1) return bad("allele '" + t + "' at locus " + std::to_string(k) + " is not one character");
        sym = (int32_t)(unsigned char)t[0];
      } else {
        errno = 0;
        const long v = strtol(t.c_str(), &end, 10);
        if (*end || errno || v < 0 || v > INT32_MAX) return bad("allele '" + t + "' at locus " + std::to_string(k) + " is no integer");
        sym = (int32_t)v;
      }
      rows[side].push_back(sym);
    }
    if (rows[0].empty()) return bad("no alleles before '|'");
    if (side == 1 && rows[1].size() != rows[0].size()) return bad("the B row has " + std::to_string(rows[1].size()) + " alleles, the A row " + std::to_string(rows[0].size()));
    if (side == 0) rows[1].assign(rows[0].size(), -1);
    out.two_sided = out.two_sided || side == 1;
    out.names.push_back(tok[0]);
    out.start.push_back((int32_t)st);
    out.len.push_back((int32_t)rows[0].size());
    out.maxlen = std::max(out.maxlen, (int)rows[0].size());
    out.a.push_back(rows[0]);
    out.b.push_back(rows[1]);
  }
  return 0;
}

}  // namespace hmc_cli
