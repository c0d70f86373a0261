// window_main.cpp — host sanitizer program for the GPU-free host code of
// hmc_window_phasings: the configuration plan (hmc_amd/csrc/window_plan.hpp:
// branching loci, radices, C, code <-> haplotype, swap, the canonical order)
// and hmc_resolve's window-list parser (tools/hmc_winfile.hpp).  Built with
// -fsanitize=address,undefined by tests/test_window_host.py; every check aborts
// with a message.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../hmc_amd/csrc/window_plan.hpp"
#include "../../tools/hmc_winfile.hpp"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

using Hap = std::vector<uint8_t>;

// Every ordered pair of allele strings the genotype allows over the window, by brute force.
static std::set<std::pair<Hap, Hap>> brute(const uint8_t *g0, const uint8_t *g1, const uint8_t *nall, int len, size_t stop) {
  std::set<std::pair<Hap, Hap>> cur{{Hap(), Hap()}};
  for (int k = 0; k < len && cur.size() <= stop; ++k) {
    std::set<std::pair<uint8_t, uint8_t>> opts;
    const uint8_t a = g0[k], b = g1[k], M = hmc::WIN_MISSING;
    for (int x = 0; x < nall[k]; ++x)
      for (int y = 0; y < nall[k]; ++y) {
        const bool ok = (a == M && b == M) || (a == M && (x == b || y == b)) || (b == M && (x == a || y == a)) ||
                        (a != M && b != M && ((x == a && y == b) || (x == b && y == a)));
        if (ok) opts.insert({(uint8_t)x, (uint8_t)y});
      }
    std::set<std::pair<Hap, Hap>> next;
    for (const auto &p : cur)
      for (const auto &o : opts) {
        auto q = p;
        q.first.push_back(o.first);
        q.second.push_back(o.second);
        next.insert(q);
      }
    cur.swap(next);
  }
  return cur;
}

static void check_window(const Hap &g0, const Hap &g1, const Hap &nall, int cap) {
  const int len = (int)g0.size();
  std::vector<hmc::WinDigit> dig{{7, 0, 0, 0, 0}};  // an entry of an earlier window stays
  const long long C = hmc::win_plan(g0.data(), g1.data(), nall.data(), len, cap, dig);
  const auto all = brute(g0.data(), g1.data(), nall.data(), len, (size_t)cap);
  if (C > cap) {
    CHECK(C == (long long)cap + 1 && dig.size() == 1 && all.size() > (size_t)cap);
    return;
  }
  CHECK((long long)all.size() == C && C >= 1 && dig[0].rel == 7);
  const hmc::WinDigit *g = dig.data() + 1;
  const int nd = (int)dig.size() - 1;
  CHECK(nd <= hmc::WIN_DIGITS_MAX);
  long long prod = 1;
  for (int i = 0; i < nd; ++i) {
    CHECK(g[i].rel >= 0 && g[i].rel < len && (i == 0 || g[i - 1].rel < g[i].rel) && hmc::win_radix(g[i]) >= 2);
    prod *= hmc::win_radix(g[i]);
    for (int d = 0; d < hmc::win_radix(g[i]); ++d) {  // digits ascend as (a, b) does
      uint32_t xa, xb, ya, yb;
      hmc::win_decode(g[i], d, xa, xb);
      CHECK(hmc::win_encode(g[i], xa, xb) == d);
      if (d) {
        hmc::win_decode(g[i], d - 1, ya, yb);
        CHECK(std::make_pair(ya, yb) < std::make_pair(xa, xb));
      }
      const int sd = hmc::win_swap_digit(g[i], d);
      CHECK(sd >= 0 && sd < hmc::win_radix(g[i]) && hmc::win_swap_digit(g[i], sd) == d);
    }
    CHECK(hmc::win_encode(g[i], 200, 0) < 0 && hmc::win_encode(g[i], 0, 200) < 0);
  }
  CHECK(prod == C);
  Hap xa((size_t)len), xb((size_t)len), ya((size_t)len), yb((size_t)len);
  std::set<std::pair<Hap, Hap>> seen;
  std::vector<int> canon;
  for (int c = 0; c < (int)C; ++c) {
    hmc::win_spell(g, nd, c, g0.data(), g1.data(), len, xa.data(), xb.data());
    CHECK(all.count({xa, xb}) == 1 && seen.insert({xa, xb}).second);       // decode: onto the brute-force set
    CHECK(hmc::win_code_of(g, nd, xa.data(), xb.data()) == c);                // encode o decode = identity
    const int s = hmc::win_swap_code(g, nd, c);
    CHECK(s >= 0 && s < (int)C && hmc::win_swap_code(g, nd, s) == c);         // swap is an involution
    hmc::win_spell(g, nd, s, g0.data(), g1.data(), len, ya.data(), yb.data());
    CHECK(ya == xb && yb == xa);
    CHECK(hmc::win_canonical(g, nd, c) == (xa <= xb));                        // the smaller code has the smaller a side
    CHECK((c == s) == (xa == xb));
    for (int i = 0; i < nd; ++i) {
      uint32_t da, db;
      hmc::win_decode(g[i], hmc::win_digit_of(g, nd, c, i), da, db);
      CHECK(da == xa[(size_t)g[i].rel] && db == xb[(size_t)g[i].rel]);
    }
    if (hmc::win_canonical(g, nd, c)) canon.push_back(c);
  }
  // the canonical order is total and is (a string, b string) ascending
  const size_t step = canon.size() > 40 ? canon.size() / 40 : 1;
  for (size_t i = 0; i < canon.size(); i += step)
    for (size_t j = 0; j < canon.size(); j += step) {
      const int c = canon[i], d = canon[j];
      hmc::win_spell(g, nd, c, g0.data(), g1.data(), len, xa.data(), xb.data());
      hmc::win_spell(g, nd, d, g0.data(), g1.data(), len, ya.data(), yb.data());
      const bool less = hmc::win_order_less(g, nd, c, d);
      CHECK(less == (std::make_pair(xa, xb) < std::make_pair(ya, yb)));
      CHECK(!(less && hmc::win_order_less(g, nd, d, c)) && (c == d || less || hmc::win_order_less(g, nd, d, c)));
    }
}

static void plans() {
  std::mt19937 rng(20263);
  for (int it = 0; it < 600; ++it) {
    const int len = 1 + (int)(rng() % 12);
    Hap g0((size_t)len), g1((size_t)len), nall((size_t)len);
    for (int k = 0; k < len; ++k) {
      const int A = 1 + (int)(rng() % (it % 5 == 0 ? 6 : 3));
      nall[(size_t)k] = (uint8_t)A;
      const unsigned miss = rng() % 10;  // 0: both missing, 1, 2: one missing
      g0[(size_t)k] = miss == 0 || miss == 1 ? hmc::WIN_MISSING : (uint8_t)(rng() % (unsigned)A);
      g1[(size_t)k] = miss == 0 || miss == 2 ? hmc::WIN_MISSING : rng() % 2 ? g0[(size_t)k] : (uint8_t)(rng() % (unsigned)A);
      if (g1[(size_t)k] == hmc::WIN_MISSING && miss > 2) g1[(size_t)k] = (uint8_t)(rng() % (unsigned)A);
    }
    for (int cap : {1024, 64, 7, 1}) check_window(g0, g1, nall, cap);
  }
  // ten heterozygous loci fill the cap exactly; an eleventh passes it
  Hap g0(11, 0), g1(11, 1), nall(11, 2);
  std::vector<hmc::WinDigit> dig;
  CHECK(hmc::win_plan(g0.data(), g1.data(), nall.data(), 10, 1024, dig) == 1024 && dig.size() == 10);
  CHECK(hmc::win_plan(g0.data(), g1.data(), nall.data(), 11, 1024, dig) == 1025 && dig.size() == 10);
  CHECK(hmc::win_swap_code(dig.data(), 10, 0) == 1023 && hmc::win_swap_code(dig.data(), 10, 0x155) == 0x2AA);
  // the widest digit the exact path supports: 44 alleles, both missing
  const uint8_t m = hmc::WIN_MISSING, a44 = 44;
  dig.clear();
  CHECK(hmc::win_plan(&m, &m, &a44, 1, 1024, dig) == 1025 && dig.empty());
  const uint8_t a32 = 32;
  CHECK(hmc::win_plan(&m, &m, &a32, 1, 1024, dig) == 1024 && dig.size() == 1 && hmc::win_swap_code(dig.data(), 1, 31) == 31 * 32);
}

static int parse(const std::string &text, int L, hmc_cli::WinList &out, std::string &err) {
  std::istringstream in(text);
  return hmc_cli::parse_winfile(in, L, out, err);
}

static void winfiles() {
  hmc_cli::WinList w;
  std::string err;
  CHECK(parse("# comment\n\n  \ngeneA 0 4\nB\t2 1\r\nall 0 10\ngeneA 0 4\nlast 9 1\n", 10, w, err) == 0);
  CHECK(w.names.size() == 5 && w.names[1] == "B" && w.maxlen == 10);
  CHECK(w.start[0] == 0 && w.len[0] == 4 && w.start[1] == 2 && w.len[1] == 1 && w.start[4] == 9 && w.len[4] == 1);
  hmc_cli::WinList e;
  CHECK(parse("", 3, e, err) == 0 && e.names.empty() && e.maxlen == 1);
  const struct {
    const char *text;
    int line;
  } bad[] = {{"ok 0 1\nx 0\n", 2},  {"x 10 1\n", 1},     {"x -1 2\n", 1},   {"\n\nx 8 3\n", 3},       {"x 0 0\n", 1},
             {"x 0 -2\n", 1},       {"x 0 1 extra\n", 1}, {"# c\nx zero 1\n", 2}, {"x\n", 1},           {"x 1x 1\n", 1},
             {"x 0 1x\n", 1},       {"x 0 11\n", 1},     {"x 99999999999999999999 1\n", 1}, {"x 0 99999999999999999999\n", 1}};
  for (const auto &b : bad) {
    hmc_cli::WinList o;
    err.clear();
    CHECK(parse(b.text, 10, o, err) == 1);
    CHECK(err.find("line " + std::to_string(b.line) + ":") != std::string::npos);
  }
}

int main() {
  plans();
  winfiles();
  printf("sanitized window host checks ok\n");
  return 0;
}
