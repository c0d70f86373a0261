// ctx_query.cpp — Ctx members: the posterior queries on the exact lattice (genotype, switch and pair posteriors,
// posterior draws, genotype likelihoods, haplotype dosages, MAP and ranked phasings, MAP phasing given phase sets, window phasings).  Each runs the shard through
// estep_split(order, true) like a round of the exact M-step (xp_pass) with a kernel of its own per group in place of
// the trie walk (exact_group, ctx_exact.cpp).  The kernels differ; the host code around them is written once here.
#include "ctx.hpp"

namespace hmc {

// the query kinds' nouns in messages, by XpMode
static const char *const QUERY_NOUN[] = {"",
                                         "genotype posteriors",
                                         "switch posteriors",
                                         "pair posteriors",
                                         "posterior draws",
                                         "genotype likelihoods",
                                         "haplotype dosages",
                                         "MAP phasing",
                                         "ranked phasings",
                                         "MAP phasing given evidence",
                                         "window phasings"};

int Ctx::query_ready(XpMode kind) {
  const char *noun = QUERY_NOUN[kind];
  if (!have_estep) return fail(HMC_EARG, "%s need%s an E-step first (hmc_resolve_all)", noun, kind == XP_MAP || kind == XP_GIVEN ? "s" : "");
  // P(genotype) of the last E-step is the divisor: the table must still be the one it ran on
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "%s: the model changed since the last E-step (hmc_resolve_all again)", noun);
  if (pan.amax > 44)  // the records pack a locus's allele pairs (amax (amax + 1) / 2) in 10 bits
    return fail(HMC_EUNSUPPORTED, "%s with more than 44 alleles per locus", noun);
  return HMC_OK;
}

int Ctx::query_rows(XpMode kind, int64_t n, const int32_t *indiv) {
  if (!indiv) n = nloc();
  if (n < 0) return fail(HMC_EARG, "%s: n = %lld is negative", QUERY_NOUN[kind], (long long)n);
  const int64_t bad = qr.build(n, indiv, i0, i1);
  if (bad >= 0)
    return fail(HMC_EARG, "%s: entry %lld: individual %d is outside this rank's shard [%d, %d)", QUERY_NOUN[kind],
                (long long)bad, indiv[bad], i0, i1);
  return HMC_OK;
}

int Ctx::timed_sweep(const char *what, const std::function<int()> &launch) {
  hipEventRecord(ev[0], st);
  if (int rc = launch()) return rc;
  hipEventRecord(ev[1], st);
  if (hipError_t e = sync_st()) return hipfail(e, what);
  float ms = 0;
  hipEventElapsedTime(&ms, ev[0], ev[1]);
  qstats[xp_mode].ms_sweep += ms;
  return HMC_OK;
}

hipError_t Ctx::spill_scratch(int NS, int fmax, int &grid, DevBuf<double> &buf) {  // (the grid does not change the bits)
  grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)1 << 30) / ((size_t)32 * NS * fmax)));
  return buf.ensure((size_t)grid * 4 * NS * fmax);
}

std::vector<int32_t> Ctx::asked_in(const int32_t *ids, int k) const {
  std::vector<int32_t> sel;  // the group's individuals that the caller asked for
  for (int q = 0; q < k; ++q)
    if (qr.asked[ids[q]]) sel.push_back(ids[q]);
  return sel;
}

int Ctx::query_batches(const char *what, const ExactArgs &x, const std::vector<int32_t> &sel, DevBuf<int32_t> &d_ord,
                       DevBuf<int32_t> &d_st, const std::function<int(size_t, int &)> &next,
                       const std::function<int(const ExactArgs &, size_t, int)> &run,
                       const std::function<hipError_t(int, int64_t, int64_t)> &scatter) {
  hipError_t e;
  int rc;
  std::vector<int32_t> h_st;
  for (size_t pos = 0; pos < sel.size();) {
    int nb = 0;
    if ((rc = next(pos, nb))) return rc;
    if ((e = d_ord.ensure(nb)) || (e = d_st.ensure(nb)) ||
        (e = hipMemsetAsync(d_st.p, 0, (size_t)nb * 4, st)))  // the kernel writes the non-zero ones
      return hipfail(e, what);
    if ((rc = upload_order(d_ord, sel.data() + pos, nb))) return rc;
    ExactArgs xb = x;
    xb.order = d_ord.p;
    xb.n_order = nb;
    if ((rc = run(xb, pos, nb))) return rc;
    h_st.resize(nb);
    if ((e = hipMemcpyAsync(h_st.data(), d_st.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) || (e = sync_st()))
      return hipfail(e, what);
    // An unresolved individual's rows are left to the caller's fallback.  First rows first: a scatter may copy
    // device-to-host straight into them (draws), and a repeated individual's other rows copy from there.
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      qr.status[bi] = h_st[u];
      const int64_t first = qr.rows[qr.begin(bi)];
      if (h_st[u] == 0 && (e = scatter(u, first, first))) return hipfail(e, what);
    }
    if ((e = sync_st())) return hipfail(e, what);
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      for (int64_t w = qr.begin(bi) + 1; h_st[u] == 0 && w < qr.end(bi); ++w)
        if ((e = scatter(u, qr.rows[w], qr.rows[qr.begin(bi)]))) return hipfail(e, what);
    }
    pos += (size_t)nb;
  }
  return HMC_OK;
}

int Ctx::upload_symtab(const char *what) {
  const int L = pan.L, A = pan.amax;
  std::vector<int32_t> symtab((size_t)L * A, -1);
  for (int l = 0; l < L; ++l)
    for (size_t j = 0; j < pan.sym[l].size(); ++j) symtab[(size_t)l * A + j] = pan.sym[l][j].first;
  hipError_t e;
  if ((e = d_dr_sym.ensure(symtab.size())) ||
      (e = hipMemcpyAsync(d_dr_sym.p, symtab.data(), symtab.size() * 4, hipMemcpyHostToDevice, st)) ||
      (e = sync_st()))  // (before the host vector dies)
    return hipfail(e, what);
  return HMC_OK;
}

void Ctx::input_genotype_rows(int64_t q, int i, int from, int rows, int32_t *hap, double *prob) const {
  const int L = pan.L;
  for (int r = from; r < rows; ++r) {
    if (prob) prob[(size_t)q * rows + r] = 0.0;
    if (hap)
      for (int side = 0; side < 2; ++side)
        for (int l = 0; l < L; ++l)
          hap[(((size_t)q * rows + r) * 2 + side) * L + l] = pan.symbol(l, pan.idx[((size_t)(i0 + i) * 2 + side) * L + l]);
  }
}

int Ctx::switch_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  SwitchArgs s;
  s.site_off = d_site_off.p;
  s.locus_a = d_sw_a.p;
  s.locus_b = d_sw_b.p;
  s.post = d_site_post.p;
  s.site_status = d_site_status.p;
  s.tier = sw_tier > 0 ? sw_tier : SWITCH_TIER_DEFAULT;
  int grid = std::max(1, std::min(k, dev_cu * 8));
  hipError_t e;
  int spilled = 0;
  for (int q = 0; q < k; ++q) spilled += fm[ids[q]] > s.tier;
  qstats[XP_SWITCH].spilled += spilled;
  if (spilled) {
    if ((e = spill_scratch(1, x.fmax, grid, d_sw_scratch))) return hipfail(e, "exact_switch_posteriors");
    s.scratch = d_sw_scratch.p;
    s.scratch_states = x.fmax;
  }
  return timed_sweep("exact_switch_posteriors", [&]() {
    return (e = launch_exact_switch_posteriors(x, s, grid, st)) ? hipfail(e, "exact_switch_posteriors") : HMC_OK;
  });
}

void Ctx::switch_list(SwitchList &sl) const {
  const int n = nloc(), L = pan.L;
  sl.off.assign((size_t)n + 1, 0);
  sl.locus_a.clear();
  sl.locus_b.clear();
  for (int i = 0; i < n; ++i) {
    const uint8_t *g0 = pan.idx.data() + ((size_t)(i0 + i) * 2) * L, *g1 = g0 + L;
    int last = -1;  // the heterozygous locus before k
    for (int k = 0; k < L; ++k) {
      if (g0[k] == MISSING || g1[k] == MISSING || g0[k] == g1[k]) continue;
      if (last >= 0) {
        sl.locus_a.push_back(last);
        sl.locus_b.push_back(k);
      }
      last = k;
    }
    sl.off[i + 1] = sl.locus_a.size();
  }
}

int Ctx::switch_posteriors(int32_t *indiv, int32_t *locus_a, int32_t *locus_b, int32_t *status, double *post,
                           const SwitchList *pre) {
  if (int rc = query_ready(XP_SWITCH)) return rc;
  const int n = nloc();
  SwitchList own;
  if (!pre) switch_list(own);
  const SwitchList &sl = pre ? *pre : own;
  const size_t ns = sl.locus_a.size();
  n_switch_last = ns;
  qstats[XP_SWITCH] = QueryStats();
  if (indiv)
    for (int i = 0; i < n; ++i)
      for (unsigned long long q = sl.off[i]; q < sl.off[i + 1]; ++q) indiv[q] = i0 + i;
  if (locus_a && ns) std::copy(sl.locus_a.begin(), sl.locus_a.end(), locus_a);
  if (locus_b && ns) std::copy(sl.locus_b.begin(), sl.locus_b.end(), locus_b);
  if (ns == 0) return HMC_OK;
  hipError_t er;
  if ((er = d_site_off.ensure((size_t)n + 1)) || (er = d_sw_a.ensure(ns)) || (er = d_sw_b.ensure(ns)) ||
      (er = d_site_status.ensure(ns)) || (er = d_site_post.ensure(ns * 2)) || (er = d_xstatus.ensure(n)) ||
      (er = d_xre.ensure(n)) || (er = d_xfmax.ensure(n)) ||
      (er = hipMemcpyAsync(d_site_off.p, sl.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_sw_a.p, sl.locus_a.data(), ns * 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_sw_b.p, sl.locus_b.data(), ns * 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemsetAsync(d_site_post.p, 0, ns * 2 * 8, st)) || (er = hipMemsetAsync(d_site_status.p, 0, ns * 4, st)))
    return hipfail(er, "switch posteriors");
  if (int rc = xp_pass(XP_SWITCH, "switch posteriors")) return rc;
  if ((status && (er = hipMemcpyAsync(status, d_site_status.p, ns * 4, hipMemcpyDeviceToHost, st))) ||
      (post && (er = hipMemcpyAsync(post, d_site_post.p, ns * 2 * 8, hipMemcpyDeviceToHost, st))) || (er = sync_st()))
    return hipfail(er, "switch posteriors");
  return HMC_OK;
}

int Ctx::pair_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  const int NS = qstats[XP_PAIR].slots;
  PairArgs s;
  s.row_off = d_site_off.p;
  s.ev_off = d_pr_evoff.p;
  s.ev = d_pr_ev.p;
  s.post = d_site_post.p;
  s.row_status = d_site_status.p;
  s.tier = pr_tier > 0 ? pr_tier : PAIR_TIER_DEFAULT;
  s.lds_states = std::max(1, std::min(s.tier, x.fmax));  // no more LDS than the group's largest record asks for
  int grid = std::max(1, std::min(k, dev_cu * 8));
  hipError_t e;
  int spilled = 0;
  for (int q = 0; q < k; ++q) spilled += fm[ids[q]] > s.tier;
  qstats[XP_PAIR].spilled += spilled;
  if (spilled) {
    if ((e = spill_scratch(NS, x.fmax, grid, d_pr_scratch))) return hipfail(e, "exact_pair_posteriors");
    s.scratch = d_pr_scratch.p;
    s.scratch_states = x.fmax;
  }
  return timed_sweep("exact_pair_posteriors", [&]() {
    return (e = launch_exact_pair_posteriors(x, s, NS, grid, st)) ? hipfail(e, "exact_pair_posteriors") : HMC_OK;
  });
}

void Ctx::pair_span_list(int span, std::vector<int32_t> &indiv, std::vector<int32_t> &locus_a,
                         std::vector<int32_t> &locus_b) const {
  const int n = nloc(), L = pan.L;
  indiv.clear();
  locus_a.clear();
  locus_b.clear();
  std::vector<int32_t> het;
  for (int i = 0; i < n; ++i) {
    const uint8_t *g0 = pan.idx.data() + ((size_t)(i0 + i) * 2) * L, *g1 = g0 + L;
    het.clear();
    for (int k = 0; k < L; ++k)
      if (g0[k] != MISSING && g1[k] != MISSING && g0[k] != g1[k]) het.push_back(k);
    for (size_t q = 0; q < het.size(); ++q)
      for (size_t d = 1; d <= (size_t)span && q + d < het.size(); ++d) {
        indiv.push_back(i0 + i);
        locus_a.push_back(het[q]);
        locus_b.push_back(het[q + d]);
      }
  }
}

int Ctx::pair_plan(int64_t nq, const int32_t *indiv, const int32_t *locus_a, const int32_t *locus_b, int ns, PairPlan &pl) {
  const int n = nloc(), L = pan.L, hl = head_len;
  for (int64_t q = 0; q < nq; ++q) {
    const int i = indiv[q], a = locus_a[q], b = locus_b[q];
    if (i < i0 || i >= i1)
      return fail(HMC_EARG, "pair posteriors: query %lld: individual %d is outside this rank's shard [%d, %d)", (long long)q, i,
                  i0, i1);
    if (a < 0 || a >= L || b < 0 || b >= L)
      return fail(HMC_EARG, "pair posteriors: query %lld: loci (%d, %d) outside [0, %d)", (long long)q, a, b, L);
    if (a >= b) return fail(HMC_EARG, "pair posteriors: query %lld: locus_a %d is not below locus_b %d", (long long)q, a, b);
    const uint8_t *g0 = pan.idx.data() + ((size_t)i * 2) * L, *g1 = g0 + L;
    for (int k : {a, b})
      if (g0[k] == MISSING || g1[k] == MISSING || g0[k] == g1[k])
        return fail(HMC_EARG, "pair posteriors: query %lld: locus %d of individual %d is not heterozygous in the input",
                    (long long)q, k, i);
  }
  // the caller's queries sorted by (individual, a, b); the distinct ones are the rows
  std::vector<size_t> ord((size_t)nq);
  for (size_t q = 0; q < ord.size(); ++q) ord[q] = q;
  auto key_less = [&](size_t x, size_t y) {
    if (indiv[x] != indiv[y]) return indiv[x] < indiv[y];
    if (locus_a[x] != locus_a[y]) return locus_a[x] < locus_a[y];
    return locus_b[x] < locus_b[y];
  };
  std::sort(ord.begin(), ord.end(), key_less);
  pl.row_off.assign((size_t)n + 1, 0);
  pl.ev_off.assign((size_t)n + 1, 0);
  pl.row_a.clear();
  pl.row_b.clear();
  pl.row_of.assign((size_t)nq, 0);
  pl.ev.clear();
  pl.need = pl.rounds = 0;
  auto rec_of = [&](int k) { return k < hl ? hl : k + 1; };
  struct Anchor {
    int a, ja, jend, round, slot;
    size_t r0, r1;  // its rows
  };
  struct Keyed {  // execution order within a round (exact.hpp, PairEvent)
    int rec, phase, a, kind, b;
    PairEvent ev;
  };
  std::vector<Anchor> anchors;
  std::vector<std::vector<int>> busy;  // [round][slot]: the record at which the slot's holder is freed
  std::vector<int> ends;               // the intervals' last records, for the number of anchors live at once
  std::vector<Keyed> evs;
  size_t p = 0;
  for (int i = 0; i < n; ++i) {
    const size_t row0 = pl.row_a.size();
    anchors.clear();
    for (; p < ord.size() && indiv[ord[p]] == i0 + i; ++p) {
      const int a = locus_a[ord[p]], b = locus_b[ord[p]];
      if (pl.row_a.size() == row0 || pl.row_a.back() != a || pl.row_b.back() != b) {
        pl.row_a.push_back(a);
        pl.row_b.push_back(b);
        if (anchors.empty() || anchors.back().a != a) anchors.push_back({a, rec_of(a), 0, 0, 0, pl.row_a.size() - 1, 0});
        anchors.back().jend = rec_of(b);  // rows ascend in b: the last one is the farthest
        anchors.back().r1 = pl.row_a.size();
      }
      pl.row_of[ord[p]] = pl.row_a.size() - 1;
    }
    pl.row_off[i + 1] = pl.row_a.size();
    // a slot is free for an anchor at record ja when its holder's last record is at most ja: at a record the
    // carried-in anchors are evaluated and freed before new ones start, and head-only anchors end in turn
    busy.clear();
    ends.clear();
    int rounds = 0;
    for (Anchor &an : anchors) {
      ends.erase(std::remove_if(ends.begin(), ends.end(), [&](int e) { return e <= an.ja; }), ends.end());
      ends.push_back(an.jend);
      pl.need = std::max(pl.need, (int)ends.size());
      bool placed = false;
      for (size_t r = 0; !placed; ++r) {
        if (r == busy.size()) busy.push_back(std::vector<int>((size_t)ns, 0));
        for (int sl = 0; sl < ns && !placed; ++sl)
          if (busy[r][sl] <= an.ja) {
            busy[r][sl] = an.jend;
            an.round = (int)r;
            an.slot = sl;
            placed = true;
          }
      }
      rounds = std::max(rounds, an.round + 1);
    }
    pl.rounds = std::max(pl.rounds, rounds);
    for (int r = 0; r < rounds; ++r) {
      evs.clear();
      for (const Anchor &an : anchors) {
        if (an.round != r) continue;
        evs.push_back({an.ja, 1, an.a, 0, 0, {an.ja, PAIR_EV_ANCHOR | an.slot << 2, an.a, -1}});
        for (size_t w = an.r0; w < an.r1; ++w) {
          const int b = pl.row_b[w], jb = rec_of(b);
          const PairEvent e{jb, PAIR_EV_EVAL | an.slot << 2, b, (int32_t)(w - row0)};
          if (jb == an.ja) evs.push_back({jb, 1, an.a, 1, b, e});  // both inside the head
          else evs.push_back({jb, 0, 0, 0, b, e});
        }
        const PairEvent f{an.jend, PAIR_EV_FREE | an.slot << 2, an.a, -1};
        if (an.jend == an.ja) evs.push_back({an.jend, 1, an.a, 2, 0, f});
        else evs.push_back({an.jend, 0, 0, 1, an.a, f});
      }
      std::sort(evs.begin(), evs.end(), [](const Keyed &x, const Keyed &y) {
        return std::tie(x.rec, x.phase, x.a, x.kind, x.b, x.ev.op) < std::tie(y.rec, y.phase, y.a, y.kind, y.b, y.ev.op);
      });
      for (const Keyed &k : evs) pl.ev.push_back(k.ev);
    }
    pl.ev_off[i + 1] = pl.ev.size();
  }
  return HMC_OK;
}

int Ctx::pair_posteriors(int64_t nq, const int32_t *indiv, const int32_t *locus_a, const int32_t *locus_b, int32_t *status,
                         double *post) {
  int rc;
  if ((rc = query_ready(XP_PAIR))) return rc;
  if (nq < 0 || (nq > 0 && (!indiv || !locus_a || !locus_b))) return fail(HMC_EARG, "pair posteriors: no queries given");
  QueryStats &qs = qstats[XP_PAIR];
  qs = QueryStats();
  if (nq == 0) return HMC_OK;
  const int n = nloc();
  PairPlan pl;
  // NS: as asked, else the smallest instantiated that holds every individual's anchors in one round (8 at most)
  int NS = pr_slots;
  if (NS == 0) {
    if ((rc = pair_plan(nq, indiv, locus_a, locus_b, PAIR_SLOTS_MAX, pl))) return rc;
    NS = pl.need <= 1 ? 1 : pl.need <= 2 ? 2 : pl.need <= 4 ? 4 : 8;
  }
  if (NS != PAIR_SLOTS_MAX || pr_slots) {
    if ((rc = pair_plan(nq, indiv, locus_a, locus_b, NS, pl))) return rc;
  }
  qs.slots = NS;
  qs.rounds = pl.rounds;
  const size_t nr = pl.row_a.size(), ne = pl.ev.size();
  hipError_t er;
  if ((er = d_site_off.ensure((size_t)n + 1)) || (er = d_pr_evoff.ensure((size_t)n + 1)) || (er = d_pr_ev.ensure(ne)) ||
      (er = d_site_status.ensure(nr)) || (er = d_site_post.ensure(nr * 2)) || (er = d_xstatus.ensure(n)) ||
      (er = d_xre.ensure(n)) || (er = d_xfmax.ensure(n)) ||
      (er = hipMemcpyAsync(d_site_off.p, pl.row_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_pr_evoff.p, pl.ev_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_pr_ev.p, pl.ev.data(), ne * sizeof(PairEvent), hipMemcpyHostToDevice, st)) ||
      (er = hipMemsetAsync(d_site_post.p, 0, nr * 2 * 8, st)) || (er = hipMemsetAsync(d_site_status.p, 0, nr * 4, st)))
    return hipfail(er, "pair posteriors");
  if ((rc = xp_pass(XP_PAIR, "pair posteriors"))) return rc;
  std::vector<int32_t> rst(nr);
  std::vector<double> rpost(nr * 2);
  if ((er = hipMemcpyAsync(rst.data(), d_site_status.p, nr * 4, hipMemcpyDeviceToHost, st)) ||
      (er = hipMemcpyAsync(rpost.data(), d_site_post.p, nr * 2 * 8, hipMemcpyDeviceToHost, st)) || (er = sync_st()))
    return hipfail(er, "pair posteriors");
  for (int64_t q = 0; q < nq; ++q) {  // rows in the caller's order
    const size_t r = pl.row_of[(size_t)q];
    if (status) status[q] = rst[r];
    if (post) {
      post[2 * q] = rpost[2 * r];
      post[2 * q + 1] = rpost[2 * r + 1];
    }
  }
  return HMC_OK;
}

int Ctx::draw_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) {
  const int L = pan.L, D = dr.draws, A = pan.amax;
  const size_t per = (size_t)2 * L * D;   // haplotype entries of one individual
  // device output of one individual: prob, the draw-minor bytes and the symbols
  const size_t dev_bytes = (size_t)D * 8 + (dr.hap ? per * 5 : 0);
  const size_t cap = std::max<size_t>(1, DRAW_OUT_BYTES / dev_bytes);
  const int ndc = (D + DRAW_BLOCK - 1) / DRAW_BLOCK;
  const int nchunks = (std::max(x.fmax, 1) + WAVE - 1) / WAVE;
  const int lds_chunks = dr_lds_chunks < 0 ? DRAW_LDS_CHUNKS : std::min(dr_lds_chunks, DRAW_LDS_CHUNKS);
  const std::vector<int32_t> sel = asked_in(ids, k);
  std::vector<double> h_prob;
  return query_batches(
      "exact_posterior_draws", x, sel, d_dr_order, d_dr_status,
      [&](size_t pos, int &nb) {
        nb = (int)std::min(cap, sel.size() - pos);
        return HMC_OK;
      },
      [&](const ExactArgs &xb, size_t, int nb) {
        const int grid = (int)std::max<long long>(1, std::min<long long>((long long)nb * ndc, (long long)dev_cu * 8));
        hipError_t e;
        if ((e = d_dr_prob.ensure((size_t)nb * D)) || (dr.hap && (e = d_dr_al.ensure((size_t)nb * per))) ||
            (dr.hap && (e = d_dr_hap.ensure((size_t)nb * per))) ||
            (nchunks > lds_chunks && (e = d_dr_csum.ensure((size_t)grid * nchunks))))
          return hipfail(e, "exact_posterior_draws");
        DrawArgs s;
        s.draws = D;
        s.seed = dr.seed;
        s.indiv0 = i0;
        s.al = dr.hap ? d_dr_al.p : nullptr;
        s.prob = d_dr_prob.p;
        s.status = d_dr_status.p;
        s.lds_chunks = lds_chunks;
        if (nchunks > lds_chunks) {
          s.csum = d_dr_csum.p;
          s.csum_stride = nchunks;
        }
        if (int rc = timed_sweep("exact_posterior_draws", [&]() {
              if ((e = launch_exact_posterior_draws(xb, s, grid, st))) return hipfail(e, "exact_posterior_draws");
              if (dr.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, D, A, st)))
                return hipfail(e, "draws_to_symbols");
              return (int)HMC_OK;
            }))
          return rc;
        h_prob.resize((size_t)nb * D);
        if ((e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * D * 8, hipMemcpyDeviceToHost, st)))
          return hipfail(e, "exact_posterior_draws");
        return (int)HMC_OK;
      },
      [&](int u, int64_t row, int64_t first) {
        if (dr.prob) std::copy(h_prob.begin() + (size_t)u * D, h_prob.begin() + (size_t)(u + 1) * D, dr.prob + row * D);
        if (!dr.hap) return hipSuccess;
        // each individual's symbols straight into the first of the caller's rows that ask for it: with many draws
        // no host staging buffer of the whole batch
        if (row == first)
          return hipMemcpyAsync(dr.hap + (size_t)row * per, d_dr_hap.p + (size_t)u * per, per * 4, hipMemcpyDeviceToHost, st);
        std::copy(dr.hap + (size_t)first * per, dr.hap + (size_t)(first + 1) * per, dr.hap + (size_t)row * per);  // a repeated individual
        return hipSuccess;
      });
}

// MAP and ranked phasings: batch member u's staged probabilities and symbols to a caller row
static void copy_staged(int u, int64_t row, int D, size_t per, const std::vector<double> &h_prob,
                        const std::vector<int32_t> &h_hap, double *prob, int32_t *hap) {
  if (prob) std::copy(h_prob.begin() + (size_t)u * D, h_prob.begin() + (size_t)(u + 1) * D, prob + (size_t)row * D);
  if (hap) std::copy(h_hap.begin() + (size_t)u * per, h_hap.begin() + (size_t)(u + 1) * per, hap + (size_t)row * per);
}

int Ctx::map_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) { return map_sel(x, asked_in(ids, k), dev_cu); }

int Ctx::map_sel(const ExactArgs &x, const std::vector<int32_t> &sel, int dev_cu) {
  const int L = pan.L, A = pan.amax;
  const size_t per = (size_t)2 * L;  // haplotype entries of one individual
  const size_t cap = std::max<size_t>(1, DRAW_OUT_BYTES / (8 + (dr.hap ? per * 5 : 0)));
  std::vector<int32_t> h_hap;
  std::vector<double> h_prob;
  return query_batches(
      "exact_map_phase", x, sel, d_dr_order, d_dr_status,
      [&](size_t pos, int &nb) {
        nb = (int)std::min(cap, sel.size() - pos);
        return HMC_OK;
      },
      [&](const ExactArgs &xb, size_t, int nb) {
        const int grid = std::max(1, std::min(nb, dev_cu * 8));
        hipError_t e;
        if ((e = d_dr_prob.ensure(nb)) || (dr.hap && (e = d_dr_al.ensure((size_t)nb * per))) ||
            (dr.hap && (e = d_dr_hap.ensure((size_t)nb * per))) ||
            (dr.hap && (e = hipMemsetAsync(d_dr_al.p, 0xFF, (size_t)nb * per, st))))
          return hipfail(e, "exact_map_phase");
        MapArgs s;
        s.al = dr.hap ? d_dr_al.p : nullptr;
        s.prob = d_dr_prob.p;
        s.status = d_dr_status.p;
        if (int rc = timed_sweep("exact_map_phase", [&]() {
              if ((e = launch_exact_map_phase(xb, s, grid, st))) return hipfail(e, "exact_map_phase");
              if (dr.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, 1, A, st)))
                return hipfail(e, "draws_to_symbols");
              return (int)HMC_OK;
            }))
          return rc;
        h_prob.resize(nb);
        h_hap.resize(dr.hap ? (size_t)nb * per : 0);
        if ((e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st)) ||
            (dr.hap && (e = hipMemcpyAsync(h_hap.data(), d_dr_hap.p, (size_t)nb * per * 4, hipMemcpyDeviceToHost, st))))
          return hipfail(e, "exact_map_phase");
        return (int)HMC_OK;
      },
      [&](int u, int64_t row, int64_t) {
        copy_staged(u, row, 1, per, h_prob, h_hap, dr.prob, dr.hap);
        if (gv.evidence) gv.evidence[row] = 1.0;  // (hmc_map_phase_given: an individual without events)
        return hipSuccess;
      });
}

int Ctx::given_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) {
  const int L = pan.L, A = pan.amax;
  const size_t per = (size_t)2 * L;
  const size_t cap = std::max<size_t>(1, DRAW_OUT_BYTES / (16 + (dr.hap ? per * 5 : 0)));
  std::vector<int32_t> plain, sel;  // the group's asked individuals without and with events
  for (int32_t bi : asked_in(ids, k)) (gv.plan.off[(size_t)bi + 1] > gv.plan.off[(size_t)bi] ? sel : plain).push_back(bi);
  if (int rc = map_sel(x, plain, dev_cu)) return rc;
  qstats[XP_GIVEN].constrained += (int)sel.size();
  std::vector<int32_t> h_hap;
  std::vector<double> h_prob, h_evid;
  return query_batches(
      "exact_map_phase_given", x, sel, d_dr_order, d_dr_status,
      [&](size_t pos, int &nb) {
        nb = (int)std::min(cap, sel.size() - pos);
        return HMC_OK;
      },
      [&](const ExactArgs &xb, size_t, int nb) {
        const int grid = gv_grid > 0 ? gv_grid : std::max(1, std::min(nb, dev_cu * 8));
        hipError_t e;
        if ((e = d_dr_prob.ensure(nb)) || (e = d_gv_evid.ensure(nb)) || (dr.hap && (e = d_dr_al.ensure((size_t)nb * per))) ||
            (dr.hap && (e = d_dr_hap.ensure((size_t)nb * per))) || (e = hipMemsetAsync(d_dr_prob.p, 0, (size_t)nb * 8, st)) ||
            (e = hipMemsetAsync(d_gv_evid.p, 0, (size_t)nb * 8, st)) ||
            (dr.hap && (e = hipMemsetAsync(d_dr_al.p, 0xFF, (size_t)nb * per, st))))
          return hipfail(e, "exact_map_phase_given");
        GivenArgs s;
        s.ev_off = d_gv_off.p;
        s.ev = d_gv_ev.p;
        s.al = dr.hap ? d_dr_al.p : nullptr;
        s.prob = d_dr_prob.p;
        s.evidence = d_gv_evid.p;
        s.status = d_dr_status.p;
        if (int rc = timed_sweep("exact_map_phase_given", [&]() {
              if ((e = launch_exact_map_phase_given(xb, s, grid, st, gv_block))) return hipfail(e, "exact_map_phase_given");
              if (dr.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, 1, A, st)))
                return hipfail(e, "draws_to_symbols");
              return (int)HMC_OK;
            }))
          return rc;
        h_prob.resize(nb);
        h_evid.resize(nb);
        h_hap.resize(dr.hap ? (size_t)nb * per : 0);
        if ((e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st)) ||
            (e = hipMemcpyAsync(h_evid.data(), d_gv_evid.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st)) ||
            (dr.hap && (e = hipMemcpyAsync(h_hap.data(), d_dr_hap.p, (size_t)nb * per * 4, hipMemcpyDeviceToHost, st))))
          return hipfail(e, "exact_map_phase_given");
        return (int)HMC_OK;
      },
      [&](int u, int64_t row, int64_t) {
        copy_staged(u, row, 1, per, h_prob, h_hap, dr.prob, dr.hap);
        if (gv.evidence) gv.evidence[row] = h_evid[u];
        return hipSuccess;
      });
}

int Ctx::map_phase_given(int64_t n, const int32_t *indiv, int64_t n_ev, const int32_t *ev_indiv, const int32_t *ev_locus,
                         const int32_t *ev_set, const int32_t *ev_first, int32_t *hap, double *prob, double *evidence,
                         int32_t *status) {
  int rc;
  if ((rc = query_ready(XP_GIVEN))) return rc;
  if (n_ev < 0 || (n_ev > 0 && (!ev_indiv || !ev_locus || !ev_set || !ev_first)))
    return fail(HMC_EARG, "MAP phasing given evidence: n_ev = %lld with an evidence array missing", (long long)n_ev);
  if ((rc = query_rows(XP_GIVEN, n, indiv))) return rc;
  n = qr.size();
  std::string msg;
  const int er = evidence_plan(pan.N, pan.L, pan.al.data(), i0, i1, qr.asked.data(), n_ev, ev_indiv, ev_locus, ev_set, ev_first,
                               [&](int k, int32_t a) { return pan.index_of(k, a); }, gv.plan, msg);
  if (er) return fail(er == EVP_EARG ? HMC_EARG : HMC_EUNSUPPORTED, "MAP phasing given evidence: %s", msg.c_str());
  if (n > 0) {
    const std::vector<GivenEvent> &ev = gv.plan.ev;
    hipError_t e;
    if ((e = d_gv_off.ensure(gv.plan.off.size())) || (e = d_gv_ev.ensure(std::max<size_t>(1, ev.size()))) ||
        (e = hipMemcpyAsync(d_gv_off.p, gv.plan.off.data(), gv.plan.off.size() * 8, hipMemcpyHostToDevice, st)) ||
        (!ev.empty() && (e = hipMemcpyAsync(d_gv_ev.p, ev.data(), ev.size() * sizeof(GivenEvent), hipMemcpyHostToDevice, st))) ||
        (e = sync_st()))
      return hipfail(e, "MAP phasing given evidence");
  }
  gv.evidence = evidence;
  rc = hap_query(XP_GIVEN, n, indiv, 1, 0, hap, prob, nullptr, status);
  gv.evidence = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; evidence && q < n; ++q)
    if (qr.status[qr.local(q)] != 0) evidence[q] = 0.0;
  return HMC_OK;
}

int Ctx::ranked_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) {
  const int L = pan.L, A = pan.amax, K = dr.draws, KL = rank_width(K);
  const std::vector<int32_t> sel = asked_in(ids, k);
  if (sel.empty()) return HMC_OK;
  QueryStats &qs = qstats[XP_RANK];
  qs.built = KL;
  const size_t per = (size_t)2 * L * K;  // haplotype entries of one individual
  const size_t out_cap = std::max<size_t>(1, DRAW_OUT_BYTES / ((size_t)K * 8 + (dr.hap ? per * 5 : 0)));
  hipError_t e;
  int rc;
  // the list store every individual needs: 24 KL bytes per state of its records and 8 per record
  const int ns = (int)sel.size();
  std::vector<unsigned long long> need(ns);
  {
    ExactArgs xt = x;
    if ((e = d_dr_order.ensure(ns)) || (e = d_rk_total.ensure(ns))) return hipfail(e, "exact_ranked_phasings");
    if ((rc = upload_order(d_dr_order, sel.data(), ns))) return rc;
    xt.order = d_dr_order.p;
    xt.n_order = ns;
    if ((e = launch_exact_state_totals(xt, d_rk_total.p, st)) ||
        (e = hipMemcpyAsync(need.data(), d_rk_total.p, (size_t)ns * 8, hipMemcpyDeviceToHost, st)) || (e = sync_st()))
      return hipfail(e, "exact_ranked_phasings");
    for (int u = 0; u < ns; ++u) need[u] = rank_store_bytes(KL, need[u], L + 1 - head_len);
  }
  // An individual's lists are 1.5 KL times its values, which fit the value store: alone in a batch it may take
  // that multiple of the budget, so that no individual the forward pass held is refused for its lists.
  const uint64_t budget = rank_budget_bytes(), alone = budget / 2 * 3 * (uint64_t)KL;
  uint64_t bytes = 0;
  std::vector<int32_t> h_cnt, h_hap;
  std::vector<double> h_prob;
  std::vector<unsigned long long> sbase;
  return query_batches(
      "exact_ranked_phasings", x, sel, d_dr_order, d_dr_status,
      [&](size_t pos, int &nb) {
        // a batch: individuals in order while their lists fit the budget (and the outputs theirs)
        bytes = 0;
        sbase.clear();
        while (pos + nb < sel.size() && (size_t)nb < out_cap && (nb == 0 || bytes + need[pos + nb] <= budget)) {
          if (need[pos + nb] > alone)
            return fail(HMC_ENOMEM, "ranked phasings: the lists of individual %d need %llu bytes at width %d (list store budget %llu)",
                        i0 + sel[pos + nb], (unsigned long long)need[pos + nb], KL, (unsigned long long)budget);
          sbase.push_back(bytes);
          bytes += need[pos + nb];
          ++nb;
        }
        return (int)HMC_OK;
      },
      [&](const ExactArgs &xb, size_t, int nb) {
        const int grid = std::max(1, std::min(nb, dev_cu * 8));
        if ((e = d_rk_count.ensure(nb)) || (e = d_rk_base.ensure(nb)) || (e = d_dr_prob.ensure((size_t)nb * K)) ||
            (e = d_rk_store.ensure(std::max<size_t>(bytes, 8))) || (dr.hap && (e = d_dr_al.ensure((size_t)nb * per))) ||
            (dr.hap && (e = d_dr_hap.ensure((size_t)nb * per))) || (e = hipMemsetAsync(d_rk_count.p, 0, (size_t)nb * 4, st)) ||
            (e = hipMemsetAsync(d_dr_prob.p, 0, (size_t)nb * K * 8, st)) ||  // rows past an individual's count: prob 0
            (dr.hap && (e = hipMemsetAsync(d_dr_al.p, 0xFF, (size_t)nb * per, st))) ||
            (e = hipMemcpyAsync(d_rk_base.p, sbase.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st)))
          return hipfail(e, "exact_ranked_phasings");
        RankArgs s;
        s.k = K;
        s.al = dr.hap ? d_dr_al.p : nullptr;
        s.prob = d_dr_prob.p;
        s.count = d_rk_count.p;
        s.status = d_dr_status.p;
        s.store = d_rk_store.p;
        s.store_base = d_rk_base.p;
        if ((rc = timed_sweep("exact_ranked_phasings", [&]() {
               if ((e = launch_exact_ranked_phasings(xb, s, KL, grid, st))) return hipfail(e, "exact_ranked_phasings");
               if (dr.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, K, A, st)))
                 return hipfail(e, "draws_to_symbols");
               return (int)HMC_OK;
             })))
          return rc;
        ++qs.batches;
        h_cnt.resize(nb);
        h_prob.resize((size_t)nb * K);
        h_hap.resize(dr.hap ? (size_t)nb * per : 0);
        if ((e = hipMemcpyAsync(h_cnt.data(), d_rk_count.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
            (e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * K * 8, hipMemcpyDeviceToHost, st)) ||
            (dr.hap && (e = hipMemcpyAsync(h_hap.data(), d_dr_hap.p, (size_t)nb * per * 4, hipMemcpyDeviceToHost, st))))
          return hipfail(e, "exact_ranked_phasings");
        return (int)HMC_OK;
      },
      [&](int u, int64_t row, int64_t) {
        dr.count[qr.local(row)] = h_cnt[u];
        copy_staged(u, row, K, per, h_prob, h_hap, dr.prob, dr.hap);
        return hipSuccess;
      });
}

int Ctx::dosage_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  QueryStats &qs = qstats[XP_DOSE];
  const int NS = qs.slots, P = ds.P;
  const std::vector<int32_t> sel = asked_in(ids, k);
  const size_t cap = std::max<size_t>(1, DOSE_OUT_BYTES / ((size_t)P * 8));  // individuals per batch of output rows
  DoseArgs s;
  s.ev = d_ds_ev.p;
  s.n_events = ds.n_events;
  s.codes = d_ds_codes.p;
  s.n_patterns = P;
  s.maxlen = ds.maxlen;
  s.tier = ds_tier > 0 ? ds_tier : PAIR_TIER_DEFAULT;
  s.lds_states = std::max(1, std::min(s.tier, x.fmax));  // no more LDS than the group's largest record asks for
  int spilled = 0;
  for (int bi : sel) spilled += fm[bi] > s.tier;
  qs.spilled += spilled;
  std::vector<double> h_out;
  return query_batches(
      "exact_haplotype_dosages", x, sel, d_ds_order, d_ds_status,
      [&](size_t pos, int &nb) {
        nb = (int)std::min(cap, sel.size() - pos);
        return HMC_OK;
      },
      [&](const ExactArgs &xb, size_t, int nb) {
        int grid = std::max(1, std::min(nb, dev_cu * 8));
        hipError_t e;
        if (spilled) {
          if ((e = spill_scratch(NS, x.fmax, grid, d_ds_scratch))) return hipfail(e, "exact_haplotype_dosages");
          s.scratch = d_ds_scratch.p;
          s.scratch_states = x.fmax;
        }
        if ((e = d_ds_out.ensure((size_t)nb * P)) || (e = hipMemsetAsync(d_ds_out.p, 0, (size_t)nb * P * 8, st)))
          return hipfail(e, "exact_haplotype_dosages");
        s.dosage = d_ds_out.p;
        s.status = d_ds_status.p;
        if (int rc = timed_sweep("exact_haplotype_dosages", [&]() {
              return (e = launch_exact_haplotype_dosages(xb, s, NS, grid, st)) ? hipfail(e, "exact_haplotype_dosages") : HMC_OK;
            }))
          return rc;
        h_out.resize((size_t)nb * P);
        if ((e = hipMemcpyAsync(h_out.data(), d_ds_out.p, (size_t)nb * P * 8, hipMemcpyDeviceToHost, st)))
          return hipfail(e, "exact_haplotype_dosages");
        return (int)HMC_OK;
      },
      [&](int u, int64_t row, int64_t) {  // (an unresolved individual's rows keep their zeros)
        if (ds.dosage) std::copy(h_out.begin() + (size_t)u * P, h_out.begin() + (size_t)(u + 1) * P, ds.dosage + (size_t)row * P);
        return hipSuccess;
      });
}

int Ctx::haplotype_dosages(int64_t n, const int32_t *indiv, int n_patterns, const int32_t *start, const int32_t *len, int maxlen,
                           const int32_t *alleles_a, const int32_t *alleles_b, double *dosage, int32_t *status) {
  int rc;
  if ((rc = query_ready(XP_DOSE))) return rc;
  const int nl = nloc(), L = pan.L, P = n_patterns;
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "haplotype dosages: n = %lld is negative", (long long)n);
  if (P < 0 || (P > 0 && (!start || !len || !alleles_a))) return fail(HMC_EARG, "haplotype dosages: no patterns given");
  if ((rc = query_rows(XP_DOSE, n, indiv))) return rc;
  for (int p = 0; p < P; ++p)
    if (start[p] < 0 || len[p] < 1 || len[p] > maxlen || (long long)start[p] + len[p] > L)
      return fail(HMC_EARG, "haplotype dosages: pattern %d: window start %d, length %d is outside [0, %d) or longer than maxlen %d",
                  p, start[p], len[p], L, maxlen);
  QueryStats &qs = qstats[XP_DOSE];
  qs = QueryStats();
  if (n == 0 || P == 0) return HMC_OK;
  // symbols to allele-table indices, one byte each
  std::vector<uint8_t> codes((size_t)P * 2 * maxlen, (uint8_t)DOSE_ANY);
  for (int p = 0; p < P; ++p)
    for (int side = 0; side < 2; ++side) {
      const int32_t *row = side ? alleles_b : alleles_a;
      if (!row) continue;  // (row B not given: any allele everywhere)
      for (int q = 0; q < len[p]; ++q) {
        const int32_t sy = row[(size_t)p * maxlen + q];
        if (sy == -1) continue;
        const auto &tab = pan.sym[start[p] + q];
        uint8_t c = (uint8_t)DOSE_ABSENT;
        for (size_t j = 0; j < tab.size(); ++j)
          if (tab[j].first == sy) c = (uint8_t)j;
        codes[((size_t)p * 2 + side) * maxlen + q] = c;
      }
    }
  // NS: as asked, else the smallest of 1, 2, 4 that runs the call in one round, else 4: on cfg 2 the sweep measured
  // faster at NS = 4 in twice the rounds than at NS = 8 (14.1-14.7 against 14.6-15.3 ms on windows stepping 8,
  // 47.8-48.2 against 56.5-57.1 ms on windows stepping 2; profiles/haplotype_dosages/README.md)
  DosePlan pl;
  int NS = ds_slots;
  if (NS == 0) {
    dose_plan(P, start, len, head_len, DOSE_SLOTS_AUTO_MAX, pl);
    NS = pl.need <= 1 ? 1 : pl.need <= 2 ? 2 : DOSE_SLOTS_AUTO_MAX;
  }
  if (NS != DOSE_SLOTS_AUTO_MAX || ds_slots) dose_plan(P, start, len, head_len, NS, pl);
  qs.slots = NS;
  qs.rounds = pl.rounds;
  ds.P = P;
  ds.maxlen = maxlen;
  ds.n_events = (int)pl.ev.size();
  ds.dosage = dosage;
  if (dosage) std::fill(dosage, dosage + (size_t)n * P, 0.0);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl)) || (er = d_ds_ev.ensure(pl.ev.size())) ||
      (er = d_ds_codes.ensure(codes.size())) ||
      (er = hipMemcpyAsync(d_ds_ev.p, pl.ev.data(), pl.ev.size() * sizeof(DoseEvent), hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_ds_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, st)) || (er = sync_st()))
    return hipfail(er, "haplotype dosages");
  rc = xp_pass(XP_DOSE, "haplotype dosages", &qr.asked);
  ds.dosage = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int stt = qr.status[qr.local(q)];
    if (status) status[q] = stt;
    // (a restarted pass may have left an earlier attempt's numbers in a row that ended unresolved)
    if (stt != 0 && dosage) std::fill(dosage + (size_t)q * P, dosage + (size_t)(q + 1) * P, 0.0);
  }
  return HMC_OK;
}

int Ctx::window_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  QueryStats &qs = qstats[XP_WINDOW];
  const int W = wn.W, K = wn.K, L = pan.L, ML = wn.maxlen;
  const std::vector<int32_t> asked = asked_in(ids, k);
  // device bytes of one individual: its rows' codes and probs, the two counts and the plan items of every window
  const size_t cap = std::max<size_t>(1, WIN_OUT_BYTES / ((size_t)W * ((size_t)K * 12 + 8 + sizeof(WinItem))));
  std::vector<WinItem> h_item;
  std::vector<int32_t> h_code, h_cnt, h_ncfg;
  std::vector<double> h_prob;
  std::vector<uint8_t> xa(ML), xb(ML);
  // sorted by the width their largest C needs: small individuals do not pay for wide ones
  for (int nc : {4, 16, 64, 256, 1024}) {
    std::vector<int32_t> sel;
    for (int32_t bi : asked)
      if (win_width(std::max(1, wn.maxc[wn.slot[bi]])) == nc) sel.push_back(bi);
    if (sel.empty()) continue;
    WindowArgs s;
    s.n_windows = W;
    s.k = K;
    s.start = d_wn_start.p;
    s.len = d_wn_len.p;
    s.dig = d_wn_dig.p;
    s.tier = wn_tier > 0 ? std::min(wn_tier, win_tier_max(nc)) : win_tier_max(nc);
    s.lds_states = std::max(1, std::min(s.tier, x.fmax));  // no more LDS than the group's largest record asks for
    // An individual past the tier gets a scratch slice of its own for its two frontiers at its widest window's
    // stride (the kernel's: C + 1 made odd); a batch takes individuals while their slices fit the budget.
    int spilled = 0;
    std::vector<unsigned long long> need(sel.size(), 0), sbase;  // doubles
    for (size_t u = 0; u < sel.size(); ++u) {
      const int bi = sel[u];
      if (fm[bi] <= s.tier) continue;
      need[u] = 2ull * (unsigned)fm[bi] * (unsigned)((std::max(1, wn.maxc[wn.slot[bi]]) + 1) | 1);
      if (need[u] * 8 > WIN_SCRATCH_BYTES)
        return fail(HMC_ENOMEM, "window phasings: the frontiers of individual %d (%d states, %d configurations) need %llu bytes (scratch budget %llu)",
                    i0 + bi, fm[bi], wn.maxc[wn.slot[bi]], need[u] * 8, (unsigned long long)WIN_SCRATCH_BYTES);
      ++spilled;
    }
    qs.spilled += spilled;
    qs.built = std::max(qs.built, nc);
    const int rc = query_batches(
        "exact_window_phasings", x, sel, d_wn_order, d_wn_status,
        [&](size_t pos, int &nb) {
          sbase.assign(1, 0);
          while (pos + nb < sel.size() && (size_t)nb < cap && (nb == 0 || (sbase.back() + need[pos + nb]) * 8 <= WIN_SCRATCH_BYTES)) {
            sbase.push_back(sbase.back() + need[pos + nb]);
            ++nb;
          }
          return HMC_OK;
        },
        [&](const ExactArgs &xb_, size_t pos, int nb) {
          const int grid = std::max(1, std::min(nb, dev_cu * 8));
          hipError_t e;
          if (spilled) {
            if ((e = d_wn_scratch.ensure(std::max<size_t>(1, sbase.back()))) || (e = d_wn_sbase.ensure(sbase.size())) ||
                (e = hipMemcpyAsync(d_wn_sbase.p, sbase.data(), sbase.size() * 8, hipMemcpyHostToDevice, st)))
              return hipfail(e, "exact_window_phasings");
            s.scratch = d_wn_scratch.p;
            s.scratch_off = d_wn_sbase.p;
          }
          const size_t nw = (size_t)nb * W;
          h_item.resize(nw);
          for (int u = 0; u < nb; ++u)
            std::copy(wn.item.begin() + (size_t)wn.slot[sel[pos + u]] * W, wn.item.begin() + ((size_t)wn.slot[sel[pos + u]] + 1) * W,
                      h_item.begin() + (size_t)u * W);
          if ((e = d_wn_item.ensure(nw)) || (e = d_wn_code.ensure(nw * K)) || (e = d_wn_prob.ensure(nw * K)) ||
              (e = d_wn_count.ensure(nw)) || (e = d_wn_ncfg.ensure(nw)) ||
              (e = hipMemcpyAsync(d_wn_item.p, h_item.data(), nw * sizeof(WinItem), hipMemcpyHostToDevice, st)) ||
              (e = hipMemsetAsync(d_wn_code.p, 0xFF, nw * K * 4, st)) || (e = hipMemsetAsync(d_wn_prob.p, 0, nw * K * 8, st)) ||
              (e = hipMemsetAsync(d_wn_count.p, 0, nw * 4, st)) || (e = hipMemsetAsync(d_wn_ncfg.p, 0, nw * 4, st)))
            return hipfail(e, "exact_window_phasings");
          s.item = d_wn_item.p;
          s.code = d_wn_code.p;
          s.prob = d_wn_prob.p;
          s.count = d_wn_count.p;
          s.n_config = d_wn_ncfg.p;
          s.status = d_wn_status.p;
          if (int rc2 = timed_sweep("exact_window_phasings", [&]() {
                return (e = launch_exact_window_phasings(xb_, s, nc, grid, st)) ? hipfail(e, "exact_window_phasings") : HMC_OK;
              }))
            return rc2;
          ++qs.batches;
          h_code.resize(nw * K);
          h_prob.resize(nw * K);
          h_cnt.resize(nw);
          h_ncfg.resize(nw);
          if ((e = hipMemcpyAsync(h_code.data(), d_wn_code.p, nw * K * 4, hipMemcpyDeviceToHost, st)) ||
              (e = hipMemcpyAsync(h_prob.data(), d_wn_prob.p, nw * K * 8, hipMemcpyDeviceToHost, st)) ||
              (e = hipMemcpyAsync(h_cnt.data(), d_wn_count.p, nw * 4, hipMemcpyDeviceToHost, st)) ||
              (e = hipMemcpyAsync(h_ncfg.data(), d_wn_ncfg.p, nw * 4, hipMemcpyDeviceToHost, st)))
            return hipfail(e, "exact_window_phasings");
          return (int)HMC_OK;
        },
        [&](int u, int64_t row, int64_t) {
          // the rows the kernel found: codes to symbols (the rows past the count are written when the pass is over)
          const int bi = qr.local(row), sl = wn.slot[bi];
          const uint8_t *g0 = pan.idx.data() + ((size_t)(i0 + bi) * 2) * L, *g1 = g0 + L;
          for (int w = 0; w < W; ++w) {
            const size_t b = (size_t)u * W + w, o = (size_t)row * W + w;
            const WinItem &it = wn.item[(size_t)sl * W + w];
            const int c = std::max(0, std::min(h_cnt[b], K)), k0 = wn.start[w], len = wn.len[w];
            wn.cnt[(size_t)sl * W + w] = c;
            wn.ncfg[(size_t)sl * W + w] = h_ncfg[b];
            for (int r = 0; r < c; ++r) {
              if (wn.prob) wn.prob[o * K + r] = h_prob[b * K + r];
              if (!wn.hap) continue;
              const int code = h_code[b * K + r];
              if (code < 0 || code >= it.C) continue;  // (the kernel writes none such)
              win_spell(wn.dig.data() + it.dig0, it.nd, code, g0 + k0, g1 + k0, len, xa.data(), xb.data());
              int32_t *h0 = wn.hap + ((o * K + r) * 2) * ML, *h1 = h0 + ML;
              for (int l = 0; l < len; ++l) {
                h0[l] = pan.symbol(k0 + l, xa[l]);
                h1[l] = pan.symbol(k0 + l, xb[l]);
              }
            }
          }
          return hipSuccess;
        });
    if (rc) return rc;
  }
  return HMC_OK;
}

int Ctx::window_phasings(int64_t n, const int32_t *indiv, int n_windows, const int32_t *start, const int32_t *len, int maxlen, int k,
                         int32_t *hap, double *prob, int32_t *count, int32_t *n_config, int32_t *status) {
  int rc;
  if ((rc = query_ready(XP_WINDOW))) return rc;
  const int nl = nloc(), L = pan.L, W = n_windows, K = k;
  if (W < 0 || (W > 0 && (!start || !len))) return fail(HMC_EARG, "window phasings: no windows given");
  if (k < 1 || k > WIN_K_MAX) return fail(HMC_EARG, "window phasings: k = %d is outside [1, %d]", k, WIN_K_MAX);
  if ((rc = query_rows(XP_WINDOW, n, indiv))) return rc;
  for (int w = 0; w < W; ++w)
    if (start[w] < 0 || len[w] < 1 || len[w] > maxlen || (long long)start[w] + len[w] > L)
      return fail(HMC_EARG, "window phasings: window %d: start %d, length %d is outside [0, %d) or longer than maxlen %d", w, start[w],
                  len[w], L, maxlen);
  n = qr.size();
  QueryStats &qs = qstats[XP_WINDOW];
  qs = QueryStats();
  if (n == 0 || W == 0) return HMC_OK;
  // the plan: per asked individual and window its branching loci and C
  const int cap = wn_cap > 0 ? wn_cap : WIN_CAP_MAX;
  std::vector<uint8_t> nall(L);
  for (int l = 0; l < L; ++l) nall[l] = (uint8_t)pan.sym[l].size();
  wn.W = W;
  wn.K = K;
  wn.maxlen = maxlen;
  wn.start = start;
  wn.len = len;
  wn.over_cap = 0;
  wn.slot.assign(nl, -1);
  int na = 0;
  for (int i = 0; i < nl; ++i)
    if (qr.asked[i]) wn.slot[i] = na++;
  wn.item.assign((size_t)na * W, WinItem{0, 0, 0});
  wn.dig.clear();
  wn.maxc.assign(na, 0);
  wn.cnt.assign((size_t)na * W, 0);
  wn.ncfg.assign((size_t)na * W, 0);
  for (int i = 0; i < nl; ++i) {
    if (!qr.asked[i]) continue;
    const uint8_t *g0 = pan.idx.data() + ((size_t)(i0 + i) * 2) * L, *g1 = g0 + L;
    const int sl = wn.slot[i];
    for (int w = 0; w < W; ++w) {
      const size_t d0 = wn.dig.size();
      const long long C = win_plan(g0 + start[w], g1 + start[w], nall.data() + start[w], len[w], cap, wn.dig);
      WinItem &it = wn.item[(size_t)sl * W + w];
      it.dig0 = (uint32_t)d0;
      it.nd = (int32_t)(wn.dig.size() - d0);
      it.C = C > cap ? 0 : (int32_t)C;
      wn.over_cap += C > cap;
      wn.maxc[sl] = std::max(wn.maxc[sl], it.C);
    }
  }
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl)) ||
      (er = d_wn_dig.ensure(std::max<size_t>(1, wn.dig.size()))) || (er = d_wn_start.ensure(W)) || (er = d_wn_len.ensure(W)) ||
      (!wn.dig.empty() &&
       (er = hipMemcpyAsync(d_wn_dig.p, wn.dig.data(), wn.dig.size() * sizeof(WinDigit), hipMemcpyHostToDevice, st))) ||
      (er = hipMemcpyAsync(d_wn_start.p, start, (size_t)W * 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_wn_len.p, len, (size_t)W * 4, hipMemcpyHostToDevice, st)) || (er = sync_st()))
    return hipfail(er, "window phasings");
  wn.hap = hap;
  wn.prob = prob;
  rc = xp_pass(XP_WINDOW, "window phasings", &qr.asked);
  wn.hap = nullptr;
  wn.prob = nullptr;
  wn.start = wn.len = nullptr;
  qs.constrained = wn.over_cap;
  if (rc) return rc;
  // statuses and counts; rows past the count (all of them at status 1, 2 or 4): the input genotype over the window
  // at probability 0; -1 past the window's length
  for (int64_t q = 0; q < n; ++q) {
    const int i = qr.local(q), sl = wn.slot[i];
    for (int w = 0; w < W; ++w) {
      const size_t o = (size_t)q * W + w, pi = (size_t)sl * W + w;
      const int stt = wn.item[pi].C == 0 ? 4 : qr.status[i], c = stt == 0 ? wn.cnt[pi] : 0;
      if (status) status[o] = stt;
      if (count) count[o] = c;
      if (n_config) n_config[o] = stt == 0 ? wn.ncfg[pi] : 0;
      for (int r = 0; r < K; ++r) {
        if (prob && r >= c) prob[o * K + r] = 0.0;
        if (!hap) continue;
        for (int side = 0; side < 2; ++side) {
          int32_t *h = hap + ((o * K + r) * 2 + side) * maxlen;
          for (int l = 0; l < len[w] && r >= c; ++l) h[l] = pan.symbol(start[w] + l, pan.idx[((size_t)(i0 + i) * 2 + side) * L + start[w] + l]);
          for (int l = len[w]; l < maxlen; ++l) h[l] = -1;
        }
      }
    }
  }
  return HMC_OK;
}

int Ctx::hap_query(XpMode kind, int64_t n, const int32_t *indiv, int draws, uint64_t seed, int32_t *hap, double *prob,
                   int32_t *count, int32_t *status) {
  const char *noun = QUERY_NOUN[kind];
  int rc;
  if ((rc = query_rows(kind, n, indiv))) return rc;
  n = qr.size();
  qstats[kind] = QueryStats();
  if (n == 0) return HMC_OK;
  const int nl = nloc();
  dr.draws = draws;
  dr.seed = seed;
  dr.hap = hap;
  dr.prob = prob;
  dr.count.assign(nl, draws);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, noun);
  if (hap && (rc = upload_symtab(noun))) return rc;
  rc = xp_pass(kind, noun, &qr.asked);
  dr.hap = nullptr;
  dr.prob = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = qr.local(q), stt = qr.status[i], cnt = stt == 0 ? dr.count[i] : 0;
    if (status) status[q] = stt;
    if (count) count[q] = cnt;
    // rows past the count (all of them for an unresolved individual or a subnormal P(genotype)): the input
    // genotype, as hmc_get_resolutions gives it, at probability 0
    input_genotype_rows(q, i, cnt, draws, hap, prob);
  }
  return HMC_OK;
}

int Ctx::posterior_draws(int64_t n, const int32_t *indiv, int draws, uint64_t seed, int32_t *hap, double *prob, int32_t *status) {
  if (int rc = query_ready(XP_DRAW)) return rc;
  if (draws < 1) return fail(HMC_EARG, "posterior draws: draws = %d is below 1", draws);
  return hap_query(XP_DRAW, n, indiv, draws, seed, hap, prob, nullptr, status);
}

int Ctx::map_phase(int64_t n, const int32_t *indiv, int32_t *hap, double *prob, int32_t *status) {
  if (int rc = query_ready(XP_MAP)) return rc;
  return hap_query(XP_MAP, n, indiv, 1, 0, hap, prob, nullptr, status);
}

int Ctx::ranked_phasings(int64_t n, const int32_t *indiv, int k, int32_t *hap, double *prob, int32_t *count, int32_t *status) {
  if (int rc = query_ready(XP_RANK)) return rc;
  if (k < 1 || k > RANK_K_MAX) return fail(HMC_EARG, "ranked phasings: k = %d is outside [1, %d]", k, RANK_K_MAX);
  return hap_query(XP_RANK, n, indiv, k, 0, hap, prob, count, status);
}

int Ctx::genotype_likelihoods(int64_t n, const int32_t *indiv, double *mantissa, int32_t *exponent, int32_t *status) {
  int rc;
  if ((rc = query_ready(XP_LIK)) || (rc = query_rows(XP_LIK, n, indiv))) return rc;
  n = qr.size();
  qstats[XP_LIK] = QueryStats();
  if (n == 0) return HMC_OK;
  const int nl = nloc();
  lk.mantissa.assign(nl, 0.0);
  lk.exponent.assign(nl, 0);
  lk.status.assign(nl, 1);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, "genotype likelihoods");
  if ((rc = xp_pass(XP_LIK, "genotype likelihoods", &qr.asked))) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = qr.local(q);
    if (mantissa) mantissa[q] = lk.mantissa[i];
    if (exponent) exponent[q] = lk.exponent[i];
    if (status) status[q] = lk.status[i];
  }
  return HMC_OK;
}

int Ctx::site_group(const ExactArgs &x, int k, int dev_cu) {
  SiteArgs s;
  s.site_off = d_site_off.p;
  s.site_locus = d_site_locus.p;
  s.post = d_site_post.p;
  s.site_status = d_site_status.p;
  s.n_pairs = pan.amax * (pan.amax + 1) / 2;
  return timed_sweep("exact_site_posteriors", [&]() {
    const hipError_t e = launch_exact_site_posteriors(x, s, std::max(1, std::min(k, dev_cu * 8)), st);
    return e ? hipfail(e, "exact_site_posteriors") : HMC_OK;
  });
}

void Ctx::site_list(SiteList &sl) const {
  std::vector<unsigned long long> &off = sl.off;
  std::vector<int32_t> &locus = sl.locus;
  const int n = nloc(), L = pan.L;
  off.assign((size_t)n + 1, 0);
  locus.clear();
  for (int i = 0; i < n; ++i) {
    const uint8_t *g0 = pan.idx.data() + ((size_t)(i0 + i) * 2) * L, *g1 = g0 + L;
    for (int k = 0; k < L; ++k)
      if (g0[k] == MISSING || g1[k] == MISSING) locus.push_back(k);
    off[i + 1] = locus.size();
  }
}

int Ctx::xp_pass(XpMode mode, const char *what, const std::vector<char> *only) {
  hipError_t er;
  // What the exact-mode structure pass shares with the E-step and a later call
  // can see is put back afterwards: the last E-step's pass times and counts,
  // its per-individual status (hmc_get_estep), the frontier statistic and the
  // structure stamps, and the capacities a restart may have grown.  The stores
  // (records, traces) are dead between an E-step and the next M- or E-step.
  const double s1_0 = ms_s1, fb_0 = ms_fb;
  const int passes_0 = n_struct_passes, pruned_0 = exact_pruned, fcap_0 = fcap, ccap_0 = ccap_mult;
  const uint64_t rec_words_0 = rec_words;
  const std::vector<int32_t> status_0 = h_status;
  uint32_t maxst_0 = 0;
  unsigned long long stamps_0[20] = {};
  if ((er = hipMemcpyAsync(&maxst_0, d_maxst.p, 4, hipMemcpyDeviceToHost, st)) ||
      (er = hipMemcpyAsync(stamps_0, d_stamps.p + 20, sizeof stamps_0, hipMemcpyDeviceToHost, st)) || (er = sync_st()))
    return hipfail(er, what);
  const int n = nloc();
  std::vector<int32_t> order;
  for (int q = 0; q < n; ++q)
    if (!only || (*only)[q]) order.push_back(q);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return h_cost[x] > h_cost[y]; });
  // The records of a cached exact M-step group are overwritten here, and the
  // posteriors' own group must never be taken for one: no reuse on either side.
  xc_reuse = false;
  xp_mode = mode;
  exact_pruned = 0;
  ms_s1 = ms_fb = 0;
  QueryStats &qs = qstats[mode];  // the groups add to the running kind's record
  int rc;
  while (true) {  // a capacity overflow restarts the pass; every site is written again
    xc_groups = 0;
    qs.ms_fb = qs.ms_sweep = 0;
    qs.spilled = qs.constrained = 0;
    rc = estep_split(order, true);
    if (rc != ESTEP_RESTART) break;
  }
  xp_mode = XP_OFF;
  xc_reuse = false;
  qs.ms_struct = ms_s1 + ms_fb;  // (ms_fb: the pruned structure re-runs of underflowing individuals)
  qs.groups = xc_groups;
  qs.pruned = exact_pruned;
  ms_s1 = s1_0;
  ms_fb = fb_0;
  n_struct_passes = passes_0;
  exact_pruned = pruned_0;
  fcap = fcap_0;
  ccap_mult = ccap_0;
  rec_words = rec_words_0;
  h_status = status_0;
  if ((er = hipMemcpyAsync(d_maxst.p, &maxst_0, 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_stamps.p + 20, stamps_0, sizeof stamps_0, hipMemcpyHostToDevice, st)) || (er = sync_st()))
    return rc ? rc : hipfail(er, what);
  return rc;
}

int Ctx::site_posteriors(int32_t *indiv, int32_t *locus, int32_t *status, double *post, const SiteList *pre) {
  if (int rc = query_ready(XP_GENOTYPE)) return rc;
  const int n = nloc(), NP = pan.amax * (pan.amax + 1) / 2;
  SiteList own;
  if (!pre) site_list(own);
  const std::vector<unsigned long long> &off = pre ? pre->off : own.off;
  const std::vector<int32_t> &loc = pre ? pre->locus : own.locus;
  const size_t ns = loc.size();
  n_sites_last = ns;
  qstats[XP_GENOTYPE] = QueryStats();
  if (indiv)
    for (int i = 0; i < n; ++i)
      for (unsigned long long q = off[i]; q < off[i + 1]; ++q) indiv[q] = i0 + i;
  if (locus && ns) std::copy(loc.begin(), loc.end(), locus);
  if (ns == 0) return HMC_OK;
  hipError_t er;
  if ((er = d_site_off.ensure((size_t)n + 1)) || (er = d_site_locus.ensure(ns)) || (er = d_site_status.ensure(ns)) ||
      (er = d_site_post.ensure(ns * NP)) || (er = d_xstatus.ensure(n)) || (er = d_xre.ensure(n)) || (er = d_xfmax.ensure(n)) ||
      (er = hipMemcpyAsync(d_site_off.p, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_site_locus.p, loc.data(), ns * 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemsetAsync(d_site_post.p, 0, ns * NP * 8, st)) || (er = hipMemsetAsync(d_site_status.p, 0, ns * 4, st)))
    return hipfail(er, "posteriors");
  if (int rc = xp_pass(XP_GENOTYPE, "posteriors")) return rc;
  if ((status && (er = hipMemcpyAsync(status, d_site_status.p, ns * 4, hipMemcpyDeviceToHost, st))) ||
      (post && (er = hipMemcpyAsync(post, d_site_post.p, ns * NP * 8, hipMemcpyDeviceToHost, st))) || (er = sync_st()))
    return hipfail(er, "posteriors");
  return HMC_OK;
}

}  // namespace hmc
