// hmc_winfile.hpp — the window list of hmc_resolve --windows WINFILE: the
// windows of hmc_window_phasings as text.  Header-only and free of the C-ABI so
// that the host sanitizer program can drive it.
//
// '#' lines and empty lines are skipped; any other line reads
//     name start len
// start is the 0-based first locus and len the number of loci, start + len at
// most the panel's loci.  Windows may overlap and repeat.
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

struct WinList {
  std::vector<std::string> names;
  std::vector<int32_t> start, len;
  int maxlen = 1;
};

// L: the panel's loci.  0 on success; otherwise err names the line.
inline int parse_winfile(std::istream &in, int L, WinList &out, std::string &err) {
  std::string line;
  int lineno = 0;
  auto bad = [&](const std::string &what) {
    err = "window file line " + std::to_string(lineno) + ": " + what;
    return 1;
  };
  auto number = [](const std::string &t, long &v) {
    errno = 0;
    char *end = nullptr;
    v = strtol(t.c_str(), &end, 10);
    return !t.empty() && !*end && !errno;
  };
  while (std::getline(in, line)) {
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty() || tok[0][0] == '#') continue;
    if (tok.size() != 3) return bad("expected: name start len");
    long st = 0, n = 0;
    if (!number(tok[1], st) || st < 0 || st >= L) return bad("start '" + tok[1] + "' is no locus in [0, " + std::to_string(L) + ")");
    if (!number(tok[2], n) || n < 1) return bad("len '" + tok[2] + "' is no length of at least 1");
    if (n > L - st) return bad("the window passes the last locus " + std::to_string(L - 1));
    out.names.push_back(tok[0]);
    out.start.push_back((int32_t)st);
    out.len.push_back((int32_t)n);
    out.maxlen = std::max(out.maxlen, (int)n);
  }
  return 0;
}

}  // namespace hmc_cli
