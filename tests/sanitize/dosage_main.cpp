// dosage_main.cpp — host sanitizer program for the GPU-free host code of
// hmc_haplotype_dosages: the plan builder (hmc_amd/csrc/dosage_plan.hpp: slot
// assignment, event order), hmc_resolve's haplotype-list parser
// (tools/hmc_hapfile.hpp) and the queries' map between caller rows and shard
// individuals (hmc_amd/csrc/query_rows.hpp).  Built with -fsanitize=address,undefined by
// tests/test_dosage_host.py; every check aborts with a message.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../hmc_amd/csrc/dosage_plan.hpp"
#include "../../hmc_amd/csrc/query_rows.hpp"
#include "../../tools/hmc_hapfile.hpp"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// Replays a plan as the kernel does and checks it against the patterns.
static void check_plan(const std::vector<int32_t> &start, const std::vector<int32_t> &len, int L, int hl, int ns) {
  const int P = (int)start.size();
  hmc::DosePlan pl;
  hmc::dose_plan(P, start.data(), len.data(), hl, ns, pl);
  auto rec_of = [&](int k) { return k < hl ? hl : k + 1; };
  CHECK((int)pl.ev.size() == 2 * P);
  std::vector<int> holder((size_t)ns, -1), anchored((size_t)P, 0), evaluated((size_t)P, 0);
  int live = 0, j = hl, rounds = P ? 1 : 0, most = 0;
  for (size_t e = 0; e < pl.ev.size(); ++e) {
    const hmc::DoseEvent &ev = pl.ev[e];
    const int kind = ev.op & 3, slot = ev.op >> 2;
    CHECK(slot >= 0 && slot < ns && ev.pat >= 0 && ev.pat < P);
    CHECK(ev.start == start[(size_t)ev.pat] && ev.len == len[(size_t)ev.pat]);
    CHECK(ev.rec >= hl && ev.rec <= L);
    if (ev.rec < j) {  // a later round starts again: nothing is carried
      CHECK(live == 0);
      ++rounds;
    }
    if (live == 0 || ev.rec < j) j = ev.rec;
    CHECK(ev.rec >= j);
    j = ev.rec;
    if (kind == hmc::DOSE_EV_ANCHOR) {
      CHECK(holder[(size_t)slot] < 0 && !anchored[(size_t)ev.pat]);
      CHECK(ev.rec == rec_of(ev.start));
      holder[(size_t)slot] = ev.pat;
      anchored[(size_t)ev.pat] = 1;
      ++live;
      most = std::max(most, live);
    } else {
      CHECK(kind == hmc::DOSE_EV_EVAL);
      CHECK(holder[(size_t)slot] == ev.pat && anchored[(size_t)ev.pat] && !evaluated[(size_t)ev.pat]);
      CHECK(ev.rec == rec_of(ev.start + ev.len - 1));
      holder[(size_t)slot] = -1;
      evaluated[(size_t)ev.pat] = 1;
      --live;
    }
  }
  CHECK(live == 0);
  for (int p = 0; p < P; ++p) CHECK(anchored[(size_t)p] && evaluated[(size_t)p]);
  CHECK(most <= ns);
  CHECK(pl.rounds >= rounds);  // (rounds that start past the previous one's end do not show as a step back)
  // need: the most patterns live at once — when p is anchored, p and those before it in (start, end, index) order that
  // are evaluated at a later record
  int need = 0;
  for (int p = 0; p < P; ++p) {
    const int ja = rec_of(start[(size_t)p]);
    int open = 1;
    for (int q = 0; q < P; ++q) {
      const bool before = std::make_tuple(start[(size_t)q], start[(size_t)q] + len[(size_t)q], q) <
                          std::make_tuple(start[(size_t)p], start[(size_t)p] + len[(size_t)p], p);
      if (before && rec_of(start[(size_t)q] + len[(size_t)q] - 1) > ja) ++open;
    }
    need = std::max(need, open);
  }
  CHECK(pl.need == need);
  CHECK((pl.rounds <= 1) == (need <= ns));
}

static void plans() {
  std::mt19937 rng(20261);
  for (int it = 0; it < 400; ++it) {
    const int L = 1 + (int)(rng() % 40), hl = 1 + (int)(rng() % std::min(3, L)), P = (int)(rng() % 60);
    std::vector<int32_t> start, len;
    for (int p = 0; p < P; ++p) {
      const int s = (int)(rng() % (unsigned)L);
      const int kind = (int)(rng() % 4);
      const int n = kind == 0 ? 1 : kind == 1 ? L - s : 1 + (int)(rng() % (unsigned)(L - s));
      start.push_back(s);
      len.push_back(n);
    }
    for (int ns : {1, 2, 4, 8}) check_plan(start, len, L, hl, ns);
  }
  check_plan({}, {}, 5, 1, 8);
  check_plan({0, 0, 0}, {5, 5, 5}, 5, 2, 1);  // duplicates: a round each
  hmc::DosePlan pl;
  const std::vector<int32_t> s{0, 0, 0}, n{5, 5, 5};
  hmc::dose_plan(3, s.data(), n.data(), 2, 1, pl);
  CHECK(pl.rounds == 3 && pl.need == 3);
}

static int parse(const std::string &text, const std::string &types, hmc_cli::HapList &out, std::string &err) {
  std::istringstream in(text);
  return hmc_cli::parse_hapfile(in, types, out, err);
}

static void hapfiles() {
  hmc_cli::HapList h;
  std::string err;
  CHECK(parse("# comment\n\n  \nh1 0 A C ? G\nh2\t2 1 2 | ? 1\r\nlast 4 12\n", "SSSSM", h, err) == 0);
  CHECK(h.names.size() == 3 && h.names[1] == "h2" && h.two_sided && h.maxlen == 4);
  CHECK(h.start[0] == 0 && h.len[0] == 4 && h.a[0][0] == 'A' && h.a[0][2] == -1 && h.b[0][3] == -1);
  CHECK(h.start[1] == 2 && h.len[1] == 2 && h.a[1][0] == '1' && h.b[1][0] == -1 && h.b[1][1] == '1');
  CHECK(h.start[2] == 4 && h.a[2][0] == 12);
  const std::vector<int32_t> pa = h.padded(false), pb = h.padded(true);
  CHECK(pa.size() == 12 && pa[4] == '1' && pa[6] == -1 && pb[5] == '1' && pa[8] == 12 && pa[9] == -1);
  hmc_cli::HapList e;
  CHECK(parse("", "SS", e, err) == 0 && e.names.empty() && !e.two_sided && e.padded(true).empty());
  const struct {
    const char *text;
    int line;
  } bad[] = {{"ok 0 A\nx 0\n", 2},          {"x 5 A\n", 1},       {"x -1 A\n", 1},      {"\n\nx 1 A C\n", 3},
             {"x 0 AC\n", 1},               {"x 0 A | C G\n", 1}, {"x 0 A | C | G\n", 1}, {"x 0 | A\n", 1},
             {"# c\nx zero A\n", 2},        {"x 0 A |\n", 1},     {"x\n", 1},           {"x 1x A\n", 1},
             {"x 99999999999999999999 A\n", 1}};
  for (const auto &b : bad) {
    hmc_cli::HapList o;
    err.clear();
    CHECK(parse(b.text, "SS", o, err) == 1);
    CHECK(err.find("line " + std::to_string(b.line) + ":") != std::string::npos);
  }
  hmc_cli::HapList o;
  CHECK(parse("x 0 7 x\n", "MM", o, err) == 1 && err.find("line 1") != std::string::npos);
  CHECK(parse("x 0 -3\n", "MM", o, err) == 1);
  CHECK(parse("x 0 99999999999\n", "MM", o, err) == 1);
}

// One map: every caller row exactly once, under the individual it asks for; asked exactly where there are rows.
static void check_rows(int64_t n, const int32_t *list, int i0, int i1) {
  hmc::QueryRows r;
  CHECK(r.build(n, list, i0, i1) == -1);
  const int nl = i1 - i0;
  CHECK(r.size() == n && (int)r.asked.size() == nl && (int)r.status.size() == nl && (int)r.row_off.size() == nl + 1);
  std::vector<int> seen((size_t)n, 0);
  for (int i = 0; i < nl; ++i) {
    CHECK(r.begin(i) <= r.end(i) && r.status[(size_t)i] == 1);
    CHECK((r.asked[(size_t)i] != 0) == (r.end(i) > r.begin(i)));
    for (int64_t w = r.begin(i); w < r.end(i); ++w) {
      const int64_t q = r.rows[(size_t)w];
      CHECK(q >= 0 && q < n && !seen[(size_t)q]++);
      CHECK(r.local(q) == i && (list ? list[q] : i0 + (int)q) == i0 + i);
      CHECK(w == r.begin(i) || r.rows[(size_t)w - 1] < q);  // ascending: the first row is the caller's first
    }
  }
  CHECK(r.begin(0) == 0 && r.end(nl - 1) == n);
  for (int64_t q = 0; q < n; ++q) CHECK(seen[(size_t)q] == 1);
}

static void query_rows() {
  std::mt19937 rng(20262);
  for (int it = 0; it < 400; ++it) {
    const int i0 = it % 3 == 0 ? 0 : (int)(rng() % 50), nl = 1 + (int)(rng() % 30), i1 = i0 + nl;
    check_rows(nl, nullptr, i0, i1);  // the whole shard
    const int64_t n = (int64_t)(rng() % 80);
    std::vector<int32_t> list((size_t)n);
    const int narrow = 1 + (int)(rng() % (unsigned)nl);  // few distinct individuals: repeats
    for (auto &v : list) v = i0 + (int)(rng() % (unsigned)(it % 2 ? narrow : nl));
    check_rows(n, list.data(), i0, i1);
    check_rows(0, list.data(), i0, i1);  // an empty list
    // an entry outside the shard, below or above it, is reported with its position; at 0 and at 1 every time
    for (int64_t at : {(int64_t)0, (int64_t)1, n ? (int64_t)(rng() % (uint64_t)n) : (int64_t)0}) {
      if (at >= n) continue;
      std::vector<int32_t> bad = list;
      bad[(size_t)at] = rng() % 2 ? i0 - 1 : i1;
      hmc::QueryRows r;
      CHECK(r.build(n, bad.data(), i0, i1) == at);
      bad[(size_t)n - 1] = i1 + 7;  // a second one later: the first is named
      CHECK(r.build(n, bad.data(), i0, i1) == at);
    }
  }
  const std::vector<int32_t> two{9, 3};
  hmc::QueryRows r;
  CHECK(r.build(2, two.data(), 4, 9) == 0 && r.build(2, two.data(), 5, 10) == 1 && r.build(2, two.data(), 3, 10) == -1);
}

int main() {
  plans();
  hapfiles();
  query_rows();
  printf("sanitized dosage host checks ok\n");
  return 0;
}
