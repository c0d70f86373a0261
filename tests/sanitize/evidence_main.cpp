// evidence_main.cpp — host sanitizer program for the GPU-free host code of
// hmc_map_phase_given: the plan builder and the evidence file reader
// (hmc_amd/csrc/evidence_plan.hpp).  Built with -fsanitize=address,undefined by
// tests/test_evidence_host.py; every check aborts with a message.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../hmc_amd/csrc/evidence_plan.hpp"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct Table {
  std::vector<int32_t> i, k, s, f;
  void add(int ii, int kk, int ss, int ff) {
    i.push_back(ii);
    k.push_back(kk);
    s.push_back(ss);
    f.push_back(ff);
  }
  int64_t n() const { return (int64_t)i.size(); }
};

struct Panel {
  int N, L;
  std::vector<int32_t> al;  // [N][2][L]
  int32_t &at(int i, int h, int k) { return al[((size_t)i * 2 + h) * L + k]; }
};

static int run(Panel &p, const Table &t, int i0, int i1, const char *asked, hmc::EvidencePlan &pl, std::string &msg) {
  auto index_of = [&](int k, int32_t a) {  // symbols 10 + j: index j
    CHECK(k >= 0 && k < p.L && a >= 10);
    return (int)(a - 10);
  };
  return hmc::evidence_plan(p.N, p.L, p.al.data(), i0, i1, asked, t.n(), t.i.data(), t.k.data(), t.s.data(), t.f.data(), index_of, pl, msg);
}

// Replays an individual's events as the sweep does (record of locus k: k + 1, or
// hl below it) and returns the number of span records; checks what the kernel
// relies on: loci ascending and in range, allele indices of the individual, an
// anchor only while no set is open, a last only while one is, none left open.
static int replay(Panel &p, const hmc::EvidencePlan &pl, int i0, int i, int hl) {
  const hmc::GivenEvent *ev = pl.ev.data() + pl.off[(size_t)i];
  const int ne = (int)(pl.off[(size_t)i + 1] - pl.off[(size_t)i]);
  for (int e = 0; e < ne; ++e) {
    CHECK(ev[e].locus >= 0 && ev[e].locus < p.L);
    CHECK(e == 0 || ev[e].locus > ev[e - 1].locus);
    const int idx = ev[e].code >> 8;
    CHECK(idx == p.at(i0 + i, 0, ev[e].locus) - 10 || idx == p.at(i0 + i, 1, ev[e].locus) - 10);
  }
  int ec = 0, spans = 0;
  bool open = false;
  for (; ec < ne && ev[ec].locus < hl; ++ec) {
    if (ev[ec].code & hmc::GIVEN_EV_ANCHOR) {
      CHECK(!open);
      open = true;
    }
    CHECK(open);
    if (ev[ec].code & hmc::GIVEN_EV_LAST) open = false;
  }
  spans += open;
  for (int j = hl + 1; j <= p.L; ++j) {
    const bool has = ec < ne && ev[ec].locus == j - 1;
    const int code = has ? ev[ec].code : 0;
    if (code & hmc::GIVEN_EV_ANCHOR) CHECK(!open);
    if (has && !(code & hmc::GIVEN_EV_ANCHOR)) CHECK(open);
    const bool labels = open || (code & hmc::GIVEN_EV_ANCHOR);
    spans += labels;
    open = labels && !(code & hmc::GIVEN_EV_LAST);
    if (has) ++ec;
  }
  CHECK(ec == ne && !open);
  return spans;
}

static void plan_checks() {
  // 4 individuals, 8 loci; individual 0 and 1 heterozygous everywhere (10 / 11), 2 homozygous at locus 3 and
  // missing at locus 5, 3 heterozygous 11 / 12
  Panel p{4, 8, std::vector<int32_t>(4 * 2 * 8)};
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 8; ++k) {
      p.at(i, 0, k) = i == 3 ? 11 : 10;
      p.at(i, 1, k) = i == 3 ? 12 : 11;
    }
  p.at(2, 1, 3) = 10;
  p.at(2, 0, 5) = -1;
  hmc::EvidencePlan pl;
  std::string msg;
  {  // empty evidence
    Table t;
    CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_OK && pl.ev.empty() && pl.off.size() == 5 && pl.n_constrained == 0);
    CHECK(hmc::evidence_plan(4, 8, p.al.data(), 0, 4, nullptr, 0, nullptr, nullptr, nullptr, nullptr, [](int, int32_t) { return 0; }, pl,
                             msg) == hmc::EVP_OK);
    CHECK(run(p, t, 2, 2, nullptr, pl, msg) == hmc::EVP_OK && pl.off.size() == 1);  // an empty shard
  }
  {  // single-locus sets constrain nothing, also inside another set's range
    Table t;
    t.add(0, 2, 1, 10);
    t.add(0, 4, 2, 11);
    t.add(1, 1, 5, 10);
    t.add(1, 3, 6, 11);
    t.add(1, 6, 5, 11);
    CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_OK);
    CHECK(pl.off[1] == 0 && pl.off[2] == 2 && pl.n_constrained == 1);
    CHECK(pl.ev[0].locus == 1 && pl.ev[0].code == (hmc::GIVEN_EV_ANCHOR | 0 << 8));
    CHECK(pl.ev[1].locus == 6 && pl.ev[1].code == (hmc::GIVEN_EV_LAST | 1 << 8));
    for (int hl = 1; hl <= 3; ++hl) CHECK(replay(p, pl, 0, 1, hl) == 7 - std::max(2, hl) + 1);
  }
  {  // adjacent spans, a span that starts below head_len, one wholly inside the head; entries in any order
    Table t;
    t.add(0, 5, 9, 11);
    t.add(0, 0, -3, 10);
    t.add(0, 1, -3, 11);
    t.add(0, 2, 9, 10);
    t.add(0, 3, 9, 10);
    t.add(0, 6, 4, 10);
    t.add(0, 7, 4, 10);
    t.add(3, 1, 0, 12);
    t.add(3, 4, 0, 11);
    CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_OK && pl.n_constrained == 2);
    CHECK(pl.off[1] == 7 && pl.off[3] == 7 && pl.off[4] == 9);
    CHECK(pl.ev[7].code == (hmc::GIVEN_EV_ANCHOR | 2 << 8) && pl.ev[8].code == (hmc::GIVEN_EV_LAST | 1 << 8));
    CHECK(replay(p, pl, 0, 0, 1) == 2 + 4 + 2);
    CHECK(replay(p, pl, 0, 0, 2) == 0 + 4 + 2);  // loci 0 and 1 inside the head: a filter, no span record
    CHECK(replay(p, pl, 0, 0, 3) == 4 + 2);      // the second set starts inside the head: the head record carries it
    CHECK(replay(p, pl, 0, 3, 3) == 3);
    // the shard and the asked individuals
    CHECK(run(p, t, 1, 4, nullptr, pl, msg) == hmc::EVP_OK && pl.off.size() == 4 && pl.ev.size() == 2 && pl.off[2] == 0);
    const char asked[4] = {1, 0, 0, 0};
    CHECK(run(p, t, 0, 4, asked, pl, msg) == hmc::EVP_OK && pl.ev.size() == 7 && pl.n_constrained == 1);
  }
  {  // interleaving and nesting
    Table t;
    t.add(1, 0, 1, 10);
    t.add(1, 2, 1, 10);
    t.add(1, 1, 2, 10);
    t.add(1, 3, 2, 10);
    CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_EUNSUPPORTED && msg.find("individual 1:") == 0 && pl.ev.empty());
    const char asked[4] = {1, 0, 1, 1};  // (not asked for: ignored)
    CHECK(run(p, t, 0, 4, asked, pl, msg) == hmc::EVP_OK && pl.ev.empty());
    Table u;
    u.add(0, 0, 1, 10);
    u.add(0, 7, 1, 10);
    u.add(0, 3, 2, 10);
    u.add(0, 4, 2, 10);
    CHECK(run(p, u, 0, 4, nullptr, pl, msg) == hmc::EVP_EUNSUPPORTED && msg.find("individual 0:") == 0);
  }
  {  // every HMC_EARG case names its entry; the first offending entry wins
    struct Bad {
      int i, k, f;
    } bad[] = {{4, 0, 10}, {-1, 0, 10}, {0, 8, 10}, {0, -1, 10}, {2, 3, 10}, {2, 5, 11}, {0, 1, 12}, {0, 0, 11}};
    for (const Bad &b : bad) {
      Table t;
      t.add(0, 0, 1, 10);
      t.add(0, 2, 1, 10);
      t.add(b.i, b.k, 1, b.f);
      t.add(9, 0, 0, 0);
      CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_EARG && msg.find("evidence entry 2:") == 0);
    }
    Table t;  // an individual outside the panel is refused even when nobody is asked for
    t.add(7, 0, 0, 10);
    const char none[4] = {0, 0, 0, 0};
    CHECK(run(p, t, 0, 4, none, pl, msg) == hmc::EVP_EARG && msg.find("evidence entry 0:") == 0);
  }
  // seeded tables: a valid plan replays, whatever the order of the entries
  std::mt19937 rng(20261021);
  for (int trial = 0; trial < 300; ++trial) {
    Table t;
    for (int i = 0; i < 2; ++i) {
      int k = 0, set = 0;
      while (k < 8) {
        const int len = 1 + (int)(rng() % 4);
        for (int q = 0; q < len && k < 8; ++q) {
          if (rng() % 3) t.add(i, k, set * 7 - 5, 10 + (int)(rng() % 2));
          k += 1 + (int)(rng() % 2);
        }
        ++set;
      }
    }
    for (size_t e = t.i.size(); e > 1; --e) {  // shuffle the entries
      const size_t o = rng() % e;
      std::swap(t.i[e - 1], t.i[o]);
      std::swap(t.k[e - 1], t.k[o]);
      std::swap(t.s[e - 1], t.s[o]);
      std::swap(t.f[e - 1], t.f[o]);
    }
    CHECK(run(p, t, 0, 4, nullptr, pl, msg) == hmc::EVP_OK);
    for (int hl = 1; hl <= 3; ++hl)
      for (int i = 0; i < 4; ++i) replay(p, pl, 0, i, hl);
  }
}

static void parser_checks() {
  const std::vector<std::string> ids{"a", "b", "#3"}, markers{"m0", "m1", "rs2"};
  const std::string types = "SMS";
  hmc::EvidenceTable t;
  std::string err;
  {
    // (an id that starts with '#', as PHASE files give them, is an id on a line of four fields)
    std::istringstream in("# a comment\n\na\tm0\t5\tA\r\nb\tm1\t-7\t12\nb\trs2\t2147483647\t?\n#3\tm0\t0\tC\n#3\tm0\t0\n#Id\tMarker\tSet\tAllele\n");
    CHECK(hmc::parse_evidence(in, ids, markers, types, t, err) == 0);
    CHECK(t.indiv == (std::vector<int32_t>{0, 1, 1, 2}) && t.locus == (std::vector<int32_t>{0, 1, 2, 0}));
    CHECK(t.set == (std::vector<int32_t>{5, -7, 2147483647, 0}) && t.first == (std::vector<int32_t>{'A', 12, '?', 'C'}));
  }
  {
    std::istringstream in("");
    hmc::EvidenceTable e;
    CHECK(hmc::parse_evidence(in, ids, markers, types, e, err) == 0 && e.indiv.empty());
  }
  const char *bad[] = {"a\tm0\t5",          "a\tm0\t5\tA\tx", "z\tm0\t5\tA",  "a\tm9\t5\tA",  "a\tm0\tx\tA", "a\tm0\t\tA",
                       "a\tm0\t99999999999\tA", "a\tm0\t5\tAB",   "a\tm0\t5\t",   "a\tm1\t5\tA",  "a\tm1\t5\t-2", "a m0 5 A",
                       "a\tm1\t5\t1x",      "\t\t\t"};
  for (const char *line : bad) {
    std::istringstream in(std::string("a\tm0\t1\tA\n") + line + "\n");
    hmc::EvidenceTable e;
    CHECK(hmc::parse_evidence(in, ids, markers, types, e, err) == 1);
    CHECK(err.find("evidence file line 2:") == 0);
  }
}

int main() {
  plan_checks();
  parser_checks();
  printf("sanitized evidence host checks ok\n");
  return 0;
}
