// ctx_exact.cpp — Ctx members: the exact M-step (--exact-estimate): PatternManager::estimatePatterns.
#include "ctx.hpp"

namespace hmc {

int Ctx::spell_table(const std::vector<int32_t> &ln, std::vector<int64_t> &off, std::vector<uint8_t> &al) {
  const int P = this->P;
  std::vector<int32_t> pp(P), node;
  std::vector<uint8_t> last(P);
  hipError_t e;
  if ((e = hipMemcpyAsync(pp.data(), t_ppat.p, (size_t)P * 4, hipMemcpyDeviceToHost, st)) ||
      (e = hipMemcpyAsync(last.data(), t_last.p, (size_t)P, hipMemcpyDeviceToHost, st)) ||
      (e = sync_st()))
    return hipfail(e, "table strings");
  off.assign((size_t)P + 1, 0);
  for (int i = 0; i < P; ++i) off[i + 1] = off[i] + ln[i];
  al.assign((size_t)off[P], 0);
  std::vector<int32_t> par;
  std::vector<uint8_t> alc;
  bool tree_loaded = false;
  for (int i = 0; i < P; ++i) {
    uint8_t *o = al.data() + off[i];
    o[ln[i] - 1] = last[i];
    const int32_t q = pp[i];
    if (ln[i] == 1) continue;
    if (q >= 0 && q < i && ln[q] == ln[i] - 1) {
      std::copy(al.data() + off[q], al.data() + off[q] + ln[q], o);
      continue;
    }
    if (!tree_ok()) return fail(HMC_EUNSUPPORTED, "allele strings of this table are unknown (a table set from outside)");
    if (!tree_loaded) {
      node.resize(P);
      if ((e = hipMemcpyAsync(node.data(), t_node.p, (size_t)P * 4, hipMemcpyDeviceToHost, st)) ||
          (e = sync_st()))
        return hipfail(e, "table strings");
      int nmax = 0;
      for (int k = 0; k < P; ++k) nmax = std::max(nmax, node[k] + 1);
      par.resize(nmax);
      alc.resize(nmax);
      if (nmax && ((e = hipMemcpyAsync(par.data(), n_parent.p, (size_t)nmax * 4, hipMemcpyDeviceToHost, st)) ||
                   (e = hipMemcpyAsync(alc.data(), n_allele.p, (size_t)nmax, hipMemcpyDeviceToHost, st)) ||
                   (e = sync_st())))
        return hipfail(e, "table strings");
      tree_loaded = true;
    }
    int32_t v = node[i];
    for (int k = ln[i] - 1; k >= 0; --k) {
      o[k] = alc[v];
      v = par[v];
    }
  }
  return HMC_OK;
}

int Ctx::table_to_host(Cands &c, std::vector<int32_t> &succ) {
  if (table_on_host) {
    c = ht;
    succ = ht_succ;
    return HMC_OK;
  }
  const int P = this->P, A = pan.amax;
  std::vector<int32_t> st(P), ln(P);
  std::vector<double> fr(P), pre(P), tp(P);
  std::vector<uint32_t> su((size_t)P * A);
  hipError_t e;
  if ((e = hipMemcpyAsync(st.data(), t_start.p, (size_t)P * 4, hipMemcpyDeviceToHost, this->st)) ||
      (e = hipMemcpyAsync(ln.data(), t_len.p, (size_t)P * 4, hipMemcpyDeviceToHost, this->st)) ||
      (e = hipMemcpyAsync(fr.data(), t_freq.p, (size_t)P * 8, hipMemcpyDeviceToHost, this->st)) ||
      (e = hipMemcpyAsync(pre.data(), t_prefix.p, (size_t)P * 8, hipMemcpyDeviceToHost, this->st)) ||
      (e = hipMemcpyAsync(tp.data(), t_tp.p, (size_t)P * 8, hipMemcpyDeviceToHost, this->st)) ||
      (e = hipMemcpyAsync(su.data(), t_succ.p, su.size() * 4, hipMemcpyDeviceToHost, this->st)) ||
      (e = this->sync_st()))
    return hipfail(e, "exact: table");
  std::vector<int64_t> off;
  std::vector<uint8_t> al;
  int rc = spell_table(ln, off, al);
  if (rc) return rc;
  c = Cands();
  for (int i = 0; i < P; ++i) c.push(st[i], ln[i], al.data() + off[i], 0, false, fr[i], pre[i], tp[i]);
  succ.resize((size_t)P * A);
  for (size_t i = 0; i < su.size(); ++i) succ[i] = su[i] == NONE ? -1 : (int32_t)su[i];
  return HMC_OK;
}

int Ctx::estimate_round(Cands &c, size_t b, size_t e) {
  const int L = pan.L, A = pan.amax, N = pan.N;
  const auto t_round = std::chrono::steady_clock::now();
  const double walk0 = ms_walk;
  const bool reused = xc_reuse;
  std::vector<int32_t> child, data, root(L, -1);
  int maxd = 0;
  auto new_node = [&]() {
    child.insert(child.end(), A, -1);
    data.push_back(-1);
    return (int32_t)data.size() - 1;
  };
  for (size_t k = b; k < e; ++k) {  // ForwardPatternTree::addPattern (PatternTree.cpp:188-212)
    const int s = c.start[k];
    if (root[s] < 0) root[s] = new_node();
    int32_t u = root[s];
    const uint8_t *al = c.alleles(k);
    for (int q = 0; q < c.len[k]; ++q) {
      if (al[q] >= A) return fail(HMC_EUNSUPPORTED, "exact M-step: pattern with a missing allele");
      int32_t v = child[(size_t)u * A + al[q]];
      if (v < 0) {
        v = new_node();
        child[(size_t)u * A + al[q]] = v;
      }
      u = v;
    }
    data[u] = (int32_t)(k - b);
    maxd = std::max(maxd, (int)c.len[k]);
  }
  const size_t nc = e - b;
  hipError_t er;
  if ((er = d_tr_child.ensure(std::max<size_t>(child.size(), 1))) || (er = d_tr_data.ensure(std::max<size_t>(data.size(), 1))) ||
      (er = d_tr_root.ensure(L)) || (er = d_xacc.ensure(2 * std::max<size_t>(nc, 1))) ||
      (!child.empty() && (er = hipMemcpyAsync(d_tr_child.p, child.data(), child.size() * 4, hipMemcpyHostToDevice, st))) ||
      (!data.empty() && (er = hipMemcpyAsync(d_tr_data.p, data.data(), data.size() * 4, hipMemcpyHostToDevice, st))) ||
      (er = hipMemcpyAsync(d_tr_root.p, root.data(), (size_t)L * 4, hipMemcpyHostToDevice, st)) ||
      (er = hipMemsetAsync(d_xacc.p, 0, 2 * nc * 8, st)))
    return hipfail(er, "exact: trie");
  tr_maxd = maxd;
  // the individuals of the shard, heaviest first, through the split machinery
  const int n = nloc();
  if ((er = d_xstatus.ensure(n)) || (er = d_xre.ensure(n)) || (er = d_xfmax.ensure(n))) return hipfail(er, "exact");
  std::vector<int32_t> order(n);
  for (int q = 0; q < n; ++q) order[q] = q;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return h_cost[x] > h_cost[y]; });
  xacc_nc = nc;
  int rc;
  if (xc_reuse) {
    if ((rc = exact_group(nullptr, xc_k))) return rc;
  } else {
    const int passes0 = n_struct_passes;
    while (true) {
      xc_groups = 0;
      rc = estep_split(order, true);
      if (rc != ESTEP_RESTART) break;
      if ((er = hipMemsetAsync(d_xacc.p, 0, 2 * nc * 8, st))) return hipfail(er, "exact");
    }
    if (rc) return rc;
    // one structure pass and one walk group: the stores hold every individual
    xc_reuse = n_struct_passes == passes0 + 1 && xc_groups == 1;
  }
  std::vector<unsigned long long> acc(2 * nc);
  if ((er = hipMemcpyAsync(acc.data(), d_xacc.p, acc.size() * 8, hipMemcpyDeviceToHost, st)) ||
      (er = sync_st()))
    return hipfail(er, "exact");
  if (multi()) {  // integer sums over ranks, exactly: 32-bit halves through the double collective
    std::vector<double> h(4 * nc);
    for (size_t i = 0; i < 2 * nc; ++i) {
      h[2 * i] = (double)(acc[i] & 0xFFFFFFFFull);
      h[2 * i + 1] = (double)(acc[i] >> 32);
    }
    if ((rc = allreduce_host(h.data(), h.size()))) return rc;
    for (size_t i = 0; i < 2 * nc; ++i) acc[i] = ((unsigned long long)h[2 * i + 1] << 32) + (unsigned long long)h[2 * i];
  }
  for (size_t k = 0; k < nc; ++k) {  // HaploBuilder.cpp:317-331
    double freq = std::min((double)acc[k] / EXACT_FIXED_SCALE, (double)N);
    const double pre = std::min((double)acc[nc + k] / EXACT_FIXED_SCALE, (double)N);
    freq = std::min(freq, pre);
    c.freq[b + k] = freq / N;
    c.prefix[b + k] = pre / N;
    const double t = pre > 0 ? freq / pre : freq / N;
    c.tp[b + k] = t < 1.0 ? t : 1.0;  // HaploPattern::setTransitionProb (HaploPattern.h:47)
  }
  ++exact_rounds;
  exact_candidates += nc;
  if (debug_mem)
    fprintf(stderr, "[hmc] exact round %d: %zu candidates, trie depth %d, walk %.1f ms, round %.1f ms%s\n", exact_rounds,
            nc, maxd, ms_walk - walk0,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_round).count(),
            reused ? " (E-step data reused)" : "");
  return HMC_OK;
}

int Ctx::exact_group(const int32_t *ids, int k, const std::function<int(std::vector<int32_t> &)> &rerun) {
  const int L = pan.L;
  int dev_cu = 256;
  hipDeviceGetAttribute(&dev_cu, hipDeviceAttributeMultiprocessorCount, device);
  hipError_t e;
  ExactArgs x;
  x.L = L;
  x.head_len = head_len;
  x.width = pan.amax;
  x.order = d_order2.p;
  x.n_order = k;
  x.rec = d_rec.p;
  x.rec_off = d_rec_off.p;
  x.status = d_xstatus.p;
  x.gprob = d_total.p;
  x.x = d_trace.p;
  x.x_base = d_tbase.p;
  x.x_off = d_loc_off.p;
  x.tr_child = d_tr_child.p;
  x.tr_data = d_tr_data.p;
  x.tr_root = d_tr_root.p;
  x.max_depth = tr_maxd;
  x.head_al = d_head_al.p;
  x.acc_freq = d_xacc.p;
  x.acc_prefix = d_xacc.p + xacc_nc;
  x.forward_only = (xp_mode == XP_DRAW && dr_forward_only) || xp_mode == XP_LIK || xp_mode == XP_MAP || xp_mode == XP_RANK;
  // extended range: the posterior calls when asked for, the likelihoods always, the exact M-step never
  x.extended = xp_mode == XP_LIK || (xp_mode != XP_OFF && xp_extended);
  if (x.extended) {
    if ((e = d_xtot.ensure(nloc())) || (e = d_xtot_exp.ensure(nloc()))) return hipfail(e, "exact_fb");
    x.xtot = d_xtot.p;
    x.xtot_exp = d_xtot_exp.p;
  }
  if (xc_reuse) {  // a later round over the same group: records and fwd/bwd sums are still in place
    x.fmax = xc_fmax;
    return exact_walk_group(x, k, dev_cu);
  }
  if (xp_mode) hipEventRecord(ev[0], st);
  if ((e = launch_exact_fb(x, std::max(1, std::min(k, dev_cu * 8)), st))) return hipfail(e, "exact_fb");
  if (xp_mode) hipEventRecord(ev[1], st);
  const int n = nloc();
  std::vector<int32_t> xs(n), fm(n);
  if ((e = hipMemcpyAsync(xs.data(), d_xstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)) ||
      (e = hipMemcpyAsync(fm.data(), d_xfmax.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)) ||
      (e = sync_st()))
    return hipfail(e, "exact_fb");
  auto fb_timed = [&]() {  // (posteriors only; the stream is drained at both call sites)
    float ms = 0;
    if (xp_mode && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) xp_ms_fb += ms;
  };
  fb_timed();
  std::vector<int32_t> redo;
  for (int q = 0; q < k; ++q)
    if (xs[ids[q]] == EST_NEEDS_EXACT) redo.push_back(ids[q]);
  if (!redo.empty()) {  // their records again, pruned, then their fwd/bwd sums
    if (!rerun) return fail(HMC_EHIP, "exact M-step: a forward likelihood underflows (individual %d)", i0 + redo[0]);
    exact_pruned += (int)redo.size();
    int rc;
    if ((rc = rerun(redo))) return rc;
    const int nr = (int)redo.size();
    if ((e = d_redo.ensure(nr))) return hipfail(e, "exact underflow re-run");
    if ((rc = upload_order(d_redo, redo.data(), nr))) return rc;
    ExactArgs x2 = x;
    x2.order = d_redo.p;
    x2.n_order = nr;
    if (xp_mode) hipEventRecord(ev[0], st);
    if ((e = launch_exact_fb(x2, std::max(1, std::min(nr, dev_cu * 8)), st))) return hipfail(e, "exact_fb");
    if (xp_mode) hipEventRecord(ev[1], st);
    if ((e = hipMemcpyAsync(xs.data(), d_xstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(fm.data(), d_xfmax.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)) ||
        (e = sync_st()))
      return hipfail(e, "exact_fb");
    fb_timed();
    for (int r : redo)
      if (xs[r] == EST_NEEDS_EXACT) return fail(HMC_EHIP, "exact M-step: pruned records still underflow (individual %d)", i0 + r);
  }
  int fmax = 1;
  for (int q = 0; q < k; ++q) fmax = std::max(fmax, fm[ids[q]]);
  x.fmax = fmax;
  xc_fmax = fmax;
  xc_k = k;
  ++xc_groups;
  if (xp_mode == XP_GENOTYPE) return site_group(x, k, dev_cu);  // genotype posteriors: no trie, no walk
  if (xp_mode == XP_SWITCH) return switch_group(x, ids, fm, k, dev_cu);
  if (xp_mode == XP_PAIR) return pair_group(x, ids, fm, k, dev_cu);
  if (xp_mode == XP_DRAW) return draw_group(x, ids, k, dev_cu);
  if (xp_mode == XP_DOSE) return dosage_group(x, ids, fm, k, dev_cu);
  if (xp_mode == XP_MAP) return map_group(x, ids, k, dev_cu);
  if (xp_mode == XP_RANK) return ranked_group(x, ids, k, dev_cu);
  if (xp_mode == XP_LIK) {  // the scaled totals of the group's individuals: nothing runs after exact_fb
    std::vector<double> tot(n);
    std::vector<int32_t> ex(n);
    if ((e = hipMemcpyAsync(tot.data(), d_xtot.p, (size_t)n * 8, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(ex.data(), d_xtot_exp.p, (size_t)n * 4, hipMemcpyDeviceToHost, st)) || (e = sync_st()))
      return hipfail(e, "genotype likelihoods");
    for (int q = 0; q < k; ++q) {
      const int bi = ids[q];
      if (xs[bi] != EST_OK || !(tot[bi] > 0.0) || std::isinf(tot[bi])) continue;  // status 1, (0.0, 0)
      int fe = 0;
      lk.mantissa[bi] = std::frexp(tot[bi], &fe);  // P(genotype) = tot 2^-E_L
      lk.exponent[bi] = fe - ex[bi];
      lk.status[bi] = 0;
    }
    return HMC_OK;
  }
  return exact_walk_group(x, k, dev_cu);
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
  sw_spilled += spilled;
  if (spilled) {  // frontiers past the tier: 32 B per state and block in HBM, at most 1 GiB (the grid does not change the bits)
    grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)1 << 30) / ((size_t)32 * x.fmax)));
    if ((e = d_sw_scratch.ensure((size_t)grid * 4 * x.fmax))) return hipfail(e, "exact_switch_posteriors");
    s.scratch = d_sw_scratch.p;
    s.scratch_states = x.fmax;
  }
  hipEventRecord(ev[0], st);
  if ((e = launch_exact_switch_posteriors(x, s, grid, st))) return hipfail(e, "exact_switch_posteriors");
  hipEventRecord(ev[1], st);
  if ((e = sync_st())) return hipfail(e, "exact_switch_posteriors");
  float ms = 0;
  hipEventElapsedTime(&ms, ev[0], ev[1]);
  xp_ms_sites += ms;
  return HMC_OK;
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
  if (!have_estep) return fail(HMC_EARG, "switch posteriors need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "switch posteriors: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "switch posteriors with more than 44 alleles per locus");
  const int n = nloc();
  SwitchList own;
  if (!pre) switch_list(own);
  const SwitchList &sl = pre ? *pre : own;
  const size_t ns = sl.locus_a.size();
  n_switch_last = ns;
  sw_ms_struct = sw_ms_fb = sw_ms_sweep = 0;
  sw_groups = sw_pruned = sw_spilled = 0;
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
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  const int rc = xp_pass(XP_SWITCH, "switch posteriors");
  sw_ms_struct = xp_ms_struct;
  sw_ms_fb = xp_ms_fb;
  sw_ms_sweep = xp_ms_sites;
  sw_groups = xp_groups;
  sw_pruned = xp_pruned;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  if (rc) return rc;
  if ((status && (er = hipMemcpyAsync(status, d_site_status.p, ns * 4, hipMemcpyDeviceToHost, st))) ||
      (post && (er = hipMemcpyAsync(post, d_site_post.p, ns * 2 * 8, hipMemcpyDeviceToHost, st))) || (er = sync_st()))
    return hipfail(er, "switch posteriors");
  return HMC_OK;
}

int Ctx::pair_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  const int NS = pr_ns_run;
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
  pr_spilled += spilled;
  if (spilled) {  // frontiers past the tier: 32 NS B per state and block in HBM, at most 1 GiB (the grid does not change the bits)
    grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)1 << 30) / ((size_t)32 * NS * x.fmax)));
    if ((e = d_pr_scratch.ensure((size_t)grid * 4 * NS * x.fmax))) return hipfail(e, "exact_pair_posteriors");
    s.scratch = d_pr_scratch.p;
    s.scratch_states = x.fmax;
  }
  hipEventRecord(ev[0], st);
  if ((e = launch_exact_pair_posteriors(x, s, NS, grid, st))) return hipfail(e, "exact_pair_posteriors");
  hipEventRecord(ev[1], st);
  if ((e = sync_st())) return hipfail(e, "exact_pair_posteriors");
  float ms = 0;
  hipEventElapsedTime(&ms, ev[0], ev[1]);
  xp_ms_sites += ms;
  return HMC_OK;
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
  if (!have_estep) return fail(HMC_EARG, "pair posteriors need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "pair posteriors: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "pair posteriors with more than 44 alleles per locus");
  if (nq < 0 || (nq > 0 && (!indiv || !locus_a || !locus_b))) return fail(HMC_EARG, "pair posteriors: no queries given");
  pr_ms_struct = pr_ms_fb = pr_ms_sweep = 0;
  pr_groups = pr_pruned = pr_spilled = pr_ns = pr_rounds = 0;
  if (nq == 0) return HMC_OK;
  const int n = nloc();
  PairPlan pl;
  int rc;
  // NS: as asked, else the smallest instantiated that holds every individual's anchors in one round (8 at most)
  int NS = pr_slots;
  if (NS == 0) {
    if ((rc = pair_plan(nq, indiv, locus_a, locus_b, PAIR_SLOTS_MAX, pl))) return rc;
    NS = pl.need <= 1 ? 1 : pl.need <= 2 ? 2 : pl.need <= 4 ? 4 : 8;
  }
  if (NS != PAIR_SLOTS_MAX || pr_slots) {
    if ((rc = pair_plan(nq, indiv, locus_a, locus_b, NS, pl))) return rc;
  }
  pr_ns = pr_ns_run = NS;
  pr_rounds = pl.rounds;
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
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  rc = xp_pass(XP_PAIR, "pair posteriors");
  pr_ms_struct = xp_ms_struct;
  pr_ms_fb = xp_ms_fb;
  pr_ms_sweep = xp_ms_sites;
  pr_groups = xp_groups;
  pr_pruned = xp_pruned;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  if (rc) return rc;
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
  std::vector<int32_t> sel;  // the group's individuals that the caller asked for
  for (int q = 0; q < k; ++q)
    if (dr.row_off[ids[q] + 1] > dr.row_off[ids[q]]) sel.push_back(ids[q]);
  if (sel.empty()) return HMC_OK;
  const size_t per = (size_t)2 * L * D;   // haplotype entries of one individual
  // device output of one individual: prob, the draw-minor bytes and the symbols
  const size_t dev_bytes = (size_t)D * 8 + (dr.hap ? per * 5 : 0);
  const size_t cap = std::max<size_t>(1, DRAW_OUT_BYTES / dev_bytes);
  const int ndc = (D + DRAW_BLOCK - 1) / DRAW_BLOCK;
  const int nchunks = (std::max(x.fmax, 1) + WAVE - 1) / WAVE;
  const int lds_chunks = dr_lds_chunks < 0 ? DRAW_LDS_CHUNKS : std::min(dr_lds_chunks, DRAW_LDS_CHUNKS);
  hipError_t e;
  std::vector<int32_t> symtab((size_t)L * A, -1);  // the panel's symbol table, [locus][allele index]
  for (int l = 0; l < L; ++l)
    for (size_t j = 0; j < pan.sym[l].size(); ++j) symtab[(size_t)l * A + j] = pan.sym[l][j].first;
  if (dr.hap &&
      ((e = d_dr_sym.ensure(symtab.size())) ||
       (e = hipMemcpyAsync(d_dr_sym.p, symtab.data(), symtab.size() * 4, hipMemcpyHostToDevice, st)) || (e = sync_st())))
    return hipfail(e, "exact_posterior_draws");
  std::vector<int32_t> h_st;
  std::vector<double> h_prob;
  for (size_t pos = 0; pos < sel.size(); pos += cap) {
    const int nb = (int)std::min(cap, sel.size() - pos);
    const int grid = (int)std::max<long long>(1, std::min<long long>((long long)nb * ndc, (long long)dev_cu * 8));
    ExactArgs xb = x;
    DrawArgs s;
    if ((e = d_dr_order.ensure(nb)) || (e = d_dr_status.ensure(nb)) || (e = d_dr_prob.ensure((size_t)nb * D)) ||
        (dr.hap && (e = d_dr_al.ensure((size_t)nb * per))) || (dr.hap && (e = d_dr_hap.ensure((size_t)nb * per))) ||
        (nchunks > lds_chunks && (e = d_dr_csum.ensure((size_t)grid * nchunks))) ||
        (e = hipMemsetAsync(d_dr_status.p, 0, (size_t)nb * 4, st)))  // the kernel writes the non-zero ones
      return hipfail(e, "exact_posterior_draws");
    int rc;
    if ((rc = upload_order(d_dr_order, sel.data() + pos, nb))) return rc;
    xb.order = d_dr_order.p;
    xb.n_order = nb;
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
    hipEventRecord(ev[0], st);
    if ((e = launch_exact_posterior_draws(xb, s, grid, st))) return hipfail(e, "exact_posterior_draws");
    if (dr.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, D, A, st)))
      return hipfail(e, "draws_to_symbols");
    hipEventRecord(ev[1], st);
    h_st.resize(nb);
    h_prob.resize((size_t)nb * D);
    if ((e = hipMemcpyAsync(h_st.data(), d_dr_status.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * D * 8, hipMemcpyDeviceToHost, st)) ||
        (e = sync_st()))
      return hipfail(e, "exact_posterior_draws");
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    xp_ms_sites += ms;
    if (dr.hap) {  // each individual's symbols straight into the first of the caller's rows that ask for it
      for (int u = 0; u < nb; ++u)
        if (h_st[u] == 0 && (e = hipMemcpyAsync(dr.hap + (size_t)dr.rows[dr.row_off[sel[pos + u]]] * per, d_dr_hap.p + (size_t)u * per,
                                                per * 4, hipMemcpyDeviceToHost, st)))
          return hipfail(e, "exact_posterior_draws");
      if ((e = sync_st())) return hipfail(e, "exact_posterior_draws");
    }
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      dr.status[bi] = h_st[u];
      if (h_st[u] != 0) continue;  // (the caller's rows get the input genotype)
      int32_t *first = dr.hap ? dr.hap + (size_t)dr.rows[dr.row_off[bi]] * per : nullptr;
      for (int64_t w = dr.row_off[bi]; w < dr.row_off[bi + 1]; ++w) {
        const int64_t row = dr.rows[w];
        if (dr.prob) std::copy(h_prob.begin() + (size_t)u * D, h_prob.begin() + (size_t)(u + 1) * D, dr.prob + row * D);
        if (dr.hap && w > dr.row_off[bi]) std::copy(first, first + per, dr.hap + (size_t)row * per);  // a repeated individual
      }
    }
  }
  return HMC_OK;
}

int Ctx::map_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) {
  const int L = pan.L, A = pan.amax;
  std::vector<int32_t> sel;  // the group's individuals that the caller asked for
  for (int q = 0; q < k; ++q)
    if (mp.row_off[ids[q] + 1] > mp.row_off[ids[q]]) sel.push_back(ids[q]);
  if (sel.empty()) return HMC_OK;
  const size_t per = (size_t)2 * L;  // haplotype entries of one individual
  const size_t cap = std::max<size_t>(1, DRAW_OUT_BYTES / (8 + (mp.hap ? per * 5 : 0)));
  hipError_t e;
  std::vector<int32_t> symtab((size_t)L * A, -1);  // the panel's symbol table, [locus][allele index]
  for (int l = 0; l < L; ++l)
    for (size_t j = 0; j < pan.sym[l].size(); ++j) symtab[(size_t)l * A + j] = pan.sym[l][j].first;
  if (mp.hap &&
      ((e = d_dr_sym.ensure(symtab.size())) ||
       (e = hipMemcpyAsync(d_dr_sym.p, symtab.data(), symtab.size() * 4, hipMemcpyHostToDevice, st)) || (e = sync_st())))
    return hipfail(e, "exact_map_phase");
  std::vector<int32_t> h_st, h_hap;
  std::vector<double> h_prob;
  for (size_t pos = 0; pos < sel.size(); pos += cap) {
    const int nb = (int)std::min(cap, sel.size() - pos);
    const int grid = std::max(1, std::min(nb, dev_cu * 8));
    ExactArgs xb = x;
    MapArgs s;
    if ((e = d_dr_order.ensure(nb)) || (e = d_dr_status.ensure(nb)) || (e = d_dr_prob.ensure(nb)) ||
        (mp.hap && (e = d_dr_al.ensure((size_t)nb * per))) || (mp.hap && (e = d_dr_hap.ensure((size_t)nb * per))) ||
        (e = hipMemsetAsync(d_dr_status.p, 0, (size_t)nb * 4, st)) ||  // the kernel writes the non-zero ones
        (mp.hap && (e = hipMemsetAsync(d_dr_al.p, 0xFF, (size_t)nb * per, st))))
      return hipfail(e, "exact_map_phase");
    int rc;
    if ((rc = upload_order(d_dr_order, sel.data() + pos, nb))) return rc;
    xb.order = d_dr_order.p;
    xb.n_order = nb;
    s.al = mp.hap ? d_dr_al.p : nullptr;
    s.prob = d_dr_prob.p;
    s.status = d_dr_status.p;
    hipEventRecord(ev[0], st);
    if ((e = launch_exact_map_phase(xb, s, grid, st))) return hipfail(e, "exact_map_phase");
    if (mp.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, 1, A, st)))
      return hipfail(e, "draws_to_symbols");
    hipEventRecord(ev[1], st);
    h_st.resize(nb);
    h_prob.resize(nb);
    h_hap.resize(mp.hap ? (size_t)nb * per : 0);
    if ((e = hipMemcpyAsync(h_st.data(), d_dr_status.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st)) ||
        (mp.hap && (e = hipMemcpyAsync(h_hap.data(), d_dr_hap.p, (size_t)nb * per * 4, hipMemcpyDeviceToHost, st))) ||
        (e = sync_st()))
      return hipfail(e, "exact_map_phase");
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    xp_ms_sites += ms;
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      mp.status[bi] = h_st[u];
      if (h_st[u] != 0) continue;  // (the caller's rows get the input genotype)
      for (int64_t w = mp.row_off[bi]; w < mp.row_off[bi + 1]; ++w) {
        const int64_t row = mp.rows[w];
        if (mp.prob) mp.prob[row] = h_prob[u];
        if (mp.hap) std::copy(h_hap.begin() + (size_t)u * per, h_hap.begin() + (size_t)(u + 1) * per, mp.hap + (size_t)row * per);
      }
    }
  }
  return HMC_OK;
}

int Ctx::ranked_group(const ExactArgs &x, const int32_t *ids, int k, int dev_cu) {
  const int L = pan.L, A = pan.amax, K = rk.draws, KL = rank_width(K);
  std::vector<int32_t> sel;  // the group's individuals that the caller asked for
  for (int q = 0; q < k; ++q)
    if (rk.row_off[ids[q] + 1] > rk.row_off[ids[q]]) sel.push_back(ids[q]);
  if (sel.empty()) return HMC_OK;
  const size_t per = (size_t)2 * L * K;  // haplotype entries of one individual
  const size_t out_cap = std::max<size_t>(1, DRAW_OUT_BYTES / ((size_t)K * 8 + (rk.hap ? per * 5 : 0)));
  hipError_t e;
  int rc;
  std::vector<int32_t> symtab((size_t)L * A, -1);  // the panel's symbol table, [locus][allele index]
  for (int l = 0; l < L; ++l)
    for (size_t j = 0; j < pan.sym[l].size(); ++j) symtab[(size_t)l * A + j] = pan.sym[l][j].first;
  if (rk.hap &&
      ((e = d_dr_sym.ensure(symtab.size())) ||
       (e = hipMemcpyAsync(d_dr_sym.p, symtab.data(), symtab.size() * 4, hipMemcpyHostToDevice, st))))
    return hipfail(e, "exact_ranked_phasings");
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
  std::vector<int32_t> h_st, h_cnt, h_hap;
  std::vector<double> h_prob;
  std::vector<unsigned long long> sbase;
  for (size_t pos = 0; pos < sel.size();) {
    // a batch: individuals in order while their lists fit the budget (and the outputs theirs)
    uint64_t bytes = 0;
    int nb = 0;
    sbase.clear();
    while (pos + nb < sel.size() && (size_t)nb < out_cap && (nb == 0 || bytes + need[pos + nb] <= budget)) {
      if (need[pos + nb] > alone)
        return fail(HMC_ENOMEM, "ranked phasings: the lists of individual %d need %llu bytes at width %d (list store budget %llu)",
                    i0 + sel[pos + nb], (unsigned long long)need[pos + nb], KL, (unsigned long long)budget);
      sbase.push_back(bytes);
      bytes += need[pos + nb];
      ++nb;
    }
    const int grid = std::max(1, std::min(nb, dev_cu * 8));
    ExactArgs xb = x;
    RankArgs s;
    if ((e = d_dr_order.ensure(nb)) || (e = d_dr_status.ensure(nb)) || (e = d_rk_count.ensure(nb)) || (e = d_rk_base.ensure(nb)) ||
        (e = d_dr_prob.ensure((size_t)nb * K)) || (e = d_rk_store.ensure(std::max<size_t>(bytes, 8))) ||
        (rk.hap && (e = d_dr_al.ensure((size_t)nb * per))) || (rk.hap && (e = d_dr_hap.ensure((size_t)nb * per))) ||
        (e = hipMemsetAsync(d_dr_status.p, 0, (size_t)nb * 4, st)) ||  // the kernel writes the non-zero ones
        (e = hipMemsetAsync(d_rk_count.p, 0, (size_t)nb * 4, st)) ||
        (e = hipMemsetAsync(d_dr_prob.p, 0, (size_t)nb * K * 8, st)) ||  // rows past an individual's count: prob 0
        (rk.hap && (e = hipMemsetAsync(d_dr_al.p, 0xFF, (size_t)nb * per, st))) ||
        (e = hipMemcpyAsync(d_rk_base.p, sbase.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st)))
      return hipfail(e, "exact_ranked_phasings");
    if ((rc = upload_order(d_dr_order, sel.data() + pos, nb))) return rc;
    xb.order = d_dr_order.p;
    xb.n_order = nb;
    s.k = K;
    s.al = rk.hap ? d_dr_al.p : nullptr;
    s.prob = d_dr_prob.p;
    s.count = d_rk_count.p;
    s.status = d_dr_status.p;
    s.store = d_rk_store.p;
    s.store_base = d_rk_base.p;
    hipEventRecord(ev[0], st);
    if ((e = launch_exact_ranked_phasings(xb, s, KL, grid, st))) return hipfail(e, "exact_ranked_phasings");
    if (rk.hap && (e = launch_draws_to_symbols(d_dr_al.p, d_dr_sym.p, d_dr_hap.p, nb, L, K, A, st)))
      return hipfail(e, "draws_to_symbols");
    hipEventRecord(ev[1], st);
    h_st.resize(nb);
    h_cnt.resize(nb);
    h_prob.resize((size_t)nb * K);
    h_hap.resize(rk.hap ? (size_t)nb * per : 0);
    if ((e = hipMemcpyAsync(h_st.data(), d_dr_status.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_cnt.data(), d_rk_count.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_prob.data(), d_dr_prob.p, (size_t)nb * K * 8, hipMemcpyDeviceToHost, st)) ||
        (rk.hap && (e = hipMemcpyAsync(h_hap.data(), d_dr_hap.p, (size_t)nb * per * 4, hipMemcpyDeviceToHost, st))) ||
        (e = sync_st()))
      return hipfail(e, "exact_ranked_phasings");
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    xp_ms_sites += ms;
    ++rk_batches;
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      rk.status[bi] = h_st[u];
      if (h_st[u] != 0) continue;  // (the caller's rows get the input genotype)
      rk_count[bi] = h_cnt[u];
      for (int64_t w = rk.row_off[bi]; w < rk.row_off[bi + 1]; ++w) {
        const int64_t row = rk.rows[w];
        if (rk.prob) std::copy(h_prob.begin() + (size_t)u * K, h_prob.begin() + (size_t)(u + 1) * K, rk.prob + (size_t)row * K);
        if (rk.hap) std::copy(h_hap.begin() + (size_t)u * per, h_hap.begin() + (size_t)(u + 1) * per, rk.hap + (size_t)row * per);
      }
    }
    pos += (size_t)nb;
  }
  return HMC_OK;
}

int Ctx::dosage_group(const ExactArgs &x, const int32_t *ids, const std::vector<int32_t> &fm, int k, int dev_cu) {
  const int NS = ds_ns_run, P = ds.P;
  std::vector<int32_t> sel;  // the group's individuals that the caller asked for
  for (int q = 0; q < k; ++q)
    if (ds.row_off[ids[q] + 1] > ds.row_off[ids[q]]) sel.push_back(ids[q]);
  if (sel.empty()) return HMC_OK;
  const size_t cap = std::max<size_t>(1, DOSE_OUT_BYTES / ((size_t)P * 8));  // individuals per batch of output rows
  DoseArgs s;
  s.ev = d_ds_ev.p;
  s.n_events = ds.n_events;
  s.codes = d_ds_codes.p;
  s.n_patterns = P;
  s.maxlen = ds.maxlen;
  s.tier = ds_tier > 0 ? ds_tier : PAIR_TIER_DEFAULT;
  s.lds_states = std::max(1, std::min(s.tier, x.fmax));  // no more LDS than the group's largest record asks for
  hipError_t e;
  int spilled = 0;
  for (int bi : sel) spilled += fm[bi] > s.tier;
  ds_spilled += spilled;
  std::vector<int32_t> h_st;
  std::vector<double> h_out;
  for (size_t pos = 0; pos < sel.size(); pos += cap) {
    const int nb = (int)std::min(cap, sel.size() - pos);
    int grid = std::max(1, std::min(nb, dev_cu * 8));
    if (spilled) {  // frontiers past the tier: 32 NS B per state and block in HBM, at most 1 GiB (the grid does not change the bits)
      grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)1 << 30) / ((size_t)32 * NS * x.fmax)));
      if ((e = d_ds_scratch.ensure((size_t)grid * 4 * NS * x.fmax))) return hipfail(e, "exact_haplotype_dosages");
      s.scratch = d_ds_scratch.p;
      s.scratch_states = x.fmax;
    }
    if ((e = d_ds_order.ensure(nb)) || (e = d_ds_status.ensure(nb)) || (e = d_ds_out.ensure((size_t)nb * P)) ||
        (e = hipMemsetAsync(d_ds_status.p, 0, (size_t)nb * 4, st)) || (e = hipMemsetAsync(d_ds_out.p, 0, (size_t)nb * P * 8, st)))
      return hipfail(e, "exact_haplotype_dosages");
    int rc;
    if ((rc = upload_order(d_ds_order, sel.data() + pos, nb))) return rc;
    ExactArgs xb = x;
    xb.order = d_ds_order.p;
    xb.n_order = nb;
    s.dosage = d_ds_out.p;
    s.status = d_ds_status.p;
    hipEventRecord(ev[0], st);
    if ((e = launch_exact_haplotype_dosages(xb, s, NS, grid, st))) return hipfail(e, "exact_haplotype_dosages");
    hipEventRecord(ev[1], st);
    h_st.resize(nb);
    h_out.resize((size_t)nb * P);
    if ((e = hipMemcpyAsync(h_st.data(), d_ds_status.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_out.data(), d_ds_out.p, (size_t)nb * P * 8, hipMemcpyDeviceToHost, st)) || (e = sync_st()))
      return hipfail(e, "exact_haplotype_dosages");
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    xp_ms_sites += ms;
    for (int u = 0; u < nb; ++u) {
      const int bi = sel[pos + u];
      ds.status[bi] = h_st[u];
      if (h_st[u] != 0 || !ds.dosage) continue;  // (the caller's rows get zeros)
      for (int64_t w = ds.row_off[bi]; w < ds.row_off[bi + 1]; ++w)
        std::copy(h_out.begin() + (size_t)u * P, h_out.begin() + (size_t)(u + 1) * P, ds.dosage + (size_t)ds.rows[w] * P);
    }
  }
  return HMC_OK;
}

int Ctx::haplotype_dosages(int64_t n, const int32_t *indiv, int n_patterns, const int32_t *start, const int32_t *len, int maxlen,
                           const int32_t *alleles_a, const int32_t *alleles_b, double *dosage, int32_t *status) {
  if (!have_estep) return fail(HMC_EARG, "haplotype dosages need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "haplotype dosages: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "haplotype dosages with more than 44 alleles per locus");
  const int nl = nloc(), L = pan.L, P = n_patterns;
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "haplotype dosages: n = %lld is negative", (long long)n);
  if (P < 0 || (P > 0 && (!start || !len || !alleles_a))) return fail(HMC_EARG, "haplotype dosages: no patterns given");
  for (int64_t q = 0; indiv && q < n; ++q)
    if (indiv[q] < i0 || indiv[q] >= i1)
      return fail(HMC_EARG, "haplotype dosages: entry %lld: individual %d is outside this rank's shard [%d, %d)", (long long)q,
                  indiv[q], i0, i1);
  for (int p = 0; p < P; ++p)
    if (start[p] < 0 || len[p] < 1 || len[p] > maxlen || (long long)start[p] + len[p] > L)
      return fail(HMC_EARG, "haplotype dosages: pattern %d: window start %d, length %d is outside [0, %d) or longer than maxlen %d",
                  p, start[p], len[p], L, maxlen);
  ds_ms_struct = ds_ms_fb = ds_ms_sweep = 0;
  ds_groups = ds_pruned = ds_spilled = ds_ns = ds_rounds = 0;
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
  ds_ns = ds_ns_run = NS;
  ds_rounds = pl.rounds;
  auto local = [&](int64_t q) { return indiv ? indiv[q] - i0 : (int)q; };
  ds.P = P;
  ds.maxlen = maxlen;
  ds.n_events = (int)pl.ev.size();
  ds.dosage = dosage;
  ds.row_off.assign((size_t)nl + 1, 0);
  for (int64_t q = 0; q < n; ++q) ++ds.row_off[local(q) + 1];
  for (int i = 0; i < nl; ++i) ds.row_off[i + 1] += ds.row_off[i];
  ds.rows.assign((size_t)n, 0);
  {
    std::vector<int64_t> at(ds.row_off.begin(), ds.row_off.end() - 1);
    for (int64_t q = 0; q < n; ++q) ds.rows[at[local(q)]++] = q;
  }
  ds.status.assign(nl, 1);
  if (dosage) std::fill(dosage, dosage + (size_t)n * P, 0.0);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl)) || (er = d_ds_ev.ensure(pl.ev.size())) ||
      (er = d_ds_codes.ensure(codes.size())) ||
      (er = hipMemcpyAsync(d_ds_ev.p, pl.ev.data(), pl.ev.size() * sizeof(DoseEvent), hipMemcpyHostToDevice, st)) ||
      (er = hipMemcpyAsync(d_ds_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, st)) || (er = sync_st()))
    return hipfail(er, "haplotype dosages");
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  std::vector<char> asked(nl, 0);  // the passes run over the individuals asked for, not the whole shard
  for (int i = 0; i < nl; ++i) asked[i] = ds.row_off[i + 1] > ds.row_off[i];
  const int rc = xp_pass(XP_DOSE, "haplotype dosages", &asked);
  ds_ms_struct = xp_ms_struct;
  ds_ms_fb = xp_ms_fb;
  ds_ms_sweep = xp_ms_sites;
  ds_groups = xp_groups;
  ds_pruned = xp_pruned;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  ds.dosage = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int stt = ds.status[local(q)];
    if (status) status[q] = stt;
    // (a restarted pass may have left an earlier attempt's numbers in a row that ended unresolved)
    if (stt != 0 && dosage) std::fill(dosage + (size_t)q * P, dosage + (size_t)(q + 1) * P, 0.0);
  }
  return HMC_OK;
}

int Ctx::posterior_draws(int64_t n, const int32_t *indiv, int draws, uint64_t seed, int32_t *hap, double *prob, int32_t *status) {
  if (!have_estep) return fail(HMC_EARG, "posterior draws need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "posterior draws: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "posterior draws with more than 44 alleles per locus");
  if (draws < 1) return fail(HMC_EARG, "posterior draws: draws = %d is below 1", draws);
  const int nl = nloc(), L = pan.L;
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "posterior draws: n = %lld is negative", (long long)n);
  for (int64_t q = 0; indiv && q < n; ++q)
    if (indiv[q] < i0 || indiv[q] >= i1)
      return fail(HMC_EARG, "posterior draws: entry %lld: individual %d is outside this rank's shard [%d, %d)", (long long)q,
                  indiv[q], i0, i1);
  dr_ms_struct = dr_ms_fb = dr_ms_draw = 0;
  dr_groups = dr_pruned = 0;
  if (n == 0) return HMC_OK;
  auto local = [&](int64_t q) { return indiv ? indiv[q] - i0 : (int)q; };
  dr.draws = draws;
  dr.seed = seed;
  dr.hap = hap;
  dr.prob = prob;
  dr.row_off.assign((size_t)nl + 1, 0);
  for (int64_t q = 0; q < n; ++q) ++dr.row_off[local(q) + 1];
  for (int i = 0; i < nl; ++i) dr.row_off[i + 1] += dr.row_off[i];
  dr.rows.assign((size_t)n, 0);
  {
    std::vector<int64_t> at(dr.row_off.begin(), dr.row_off.end() - 1);
    for (int64_t q = 0; q < n; ++q) dr.rows[at[local(q)]++] = q;
  }
  dr.status.assign(nl, 1);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, "posterior draws");
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  std::vector<char> asked(nl, 0);  // the passes run over the individuals asked for, not the whole shard
  for (int i = 0; i < nl; ++i) asked[i] = dr.row_off[i + 1] > dr.row_off[i];
  const int rc = xp_pass(XP_DRAW, "posterior draws", &asked);
  dr_ms_struct = xp_ms_struct;
  dr_ms_fb = xp_ms_fb;
  dr_ms_draw = xp_ms_sites;
  dr_groups = xp_groups;
  dr_pruned = xp_pruned;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  dr.hap = nullptr;
  dr.prob = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = local(q), stt = dr.status[i];
    if (status) status[q] = stt;
    if (stt == 0) continue;
    // unresolved, or P(genotype) subnormal: the input genotype, as hmc_get_resolutions gives it, at probability 0
    if (prob) std::fill(prob + q * draws, prob + (q + 1) * draws, 0.0);
    if (hap)
      for (int d = 0; d < draws; ++d)
        for (int side = 0; side < 2; ++side)
          for (int l = 0; l < L; ++l)
            hap[(((size_t)q * draws + d) * 2 + side) * L + l] = pan.symbol(l, pan.idx[((size_t)(i0 + i) * 2 + side) * L + l]);
  }
  return HMC_OK;
}

int Ctx::map_phase(int64_t n, const int32_t *indiv, int32_t *hap, double *prob, int32_t *status) {
  if (!have_estep) return fail(HMC_EARG, "MAP phasing needs an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "MAP phasing: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "MAP phasing with more than 44 alleles per locus");
  const int nl = nloc(), L = pan.L;
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "MAP phasing: n = %lld is negative", (long long)n);
  for (int64_t q = 0; indiv && q < n; ++q)
    if (indiv[q] < i0 || indiv[q] >= i1)
      return fail(HMC_EARG, "MAP phasing: entry %lld: individual %d is outside this rank's shard [%d, %d)", (long long)q,
                  indiv[q], i0, i1);
  mp_ms_struct = mp_ms_fb = mp_ms_sweep = 0;
  mp_groups = mp_pruned = 0;
  if (n == 0) return HMC_OK;
  auto local = [&](int64_t q) { return indiv ? indiv[q] - i0 : (int)q; };
  mp.draws = 1;
  mp.hap = hap;
  mp.prob = prob;
  mp.row_off.assign((size_t)nl + 1, 0);
  for (int64_t q = 0; q < n; ++q) ++mp.row_off[local(q) + 1];
  for (int i = 0; i < nl; ++i) mp.row_off[i + 1] += mp.row_off[i];
  mp.rows.assign((size_t)n, 0);
  {
    std::vector<int64_t> at(mp.row_off.begin(), mp.row_off.end() - 1);
    for (int64_t q = 0; q < n; ++q) mp.rows[at[local(q)]++] = q;
  }
  mp.status.assign(nl, 1);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, "MAP phasing");
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  std::vector<char> asked(nl, 0);  // the passes run over the individuals asked for, not the whole shard
  for (int i = 0; i < nl; ++i) asked[i] = mp.row_off[i + 1] > mp.row_off[i];
  const int rc = xp_pass(XP_MAP, "MAP phasing", &asked);
  mp_ms_struct = xp_ms_struct;
  mp_ms_fb = xp_ms_fb;
  mp_ms_sweep = xp_ms_sites;
  mp_groups = xp_groups;
  mp_pruned = xp_pruned;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  mp.hap = nullptr;
  mp.prob = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = local(q), stt = mp.status[i];
    if (status) status[q] = stt;
    if (stt == 0) continue;
    // unresolved, or P(genotype) subnormal: the input genotype, as hmc_get_resolutions gives it, at probability 0
    if (prob) prob[q] = 0.0;
    if (hap)
      for (int side = 0; side < 2; ++side)
        for (int l = 0; l < L; ++l)
          hap[((size_t)q * 2 + side) * L + l] = pan.symbol(l, pan.idx[((size_t)(i0 + i) * 2 + side) * L + l]);
  }
  return HMC_OK;
}

int Ctx::ranked_phasings(int64_t n, const int32_t *indiv, int k, int32_t *hap, double *prob, int32_t *count, int32_t *status) {
  if (!have_estep) return fail(HMC_EARG, "ranked phasings need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "ranked phasings: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "ranked phasings with more than 44 alleles per locus");
  if (k < 1 || k > RANK_K_MAX) return fail(HMC_EARG, "ranked phasings: k = %d is outside [1, %d]", k, RANK_K_MAX);
  const int nl = nloc(), L = pan.L;
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "ranked phasings: n = %lld is negative", (long long)n);
  for (int64_t q = 0; indiv && q < n; ++q)
    if (indiv[q] < i0 || indiv[q] >= i1)
      return fail(HMC_EARG, "ranked phasings: entry %lld: individual %d is outside this rank's shard [%d, %d)", (long long)q,
                  indiv[q], i0, i1);
  rk_ms_struct = rk_ms_fb = rk_ms_sweep = 0;
  rk_groups = rk_pruned = rk_built = rk_batches = 0;
  if (n == 0) return HMC_OK;
  auto local = [&](int64_t q) { return indiv ? indiv[q] - i0 : (int)q; };
  rk.draws = k;
  rk.hap = hap;
  rk.prob = prob;
  rk.row_off.assign((size_t)nl + 1, 0);
  for (int64_t q = 0; q < n; ++q) ++rk.row_off[local(q) + 1];
  for (int i = 0; i < nl; ++i) rk.row_off[i + 1] += rk.row_off[i];
  rk.rows.assign((size_t)n, 0);
  {
    std::vector<int64_t> at(rk.row_off.begin(), rk.row_off.end() - 1);
    for (int64_t q = 0; q < n; ++q) rk.rows[at[local(q)]++] = q;
  }
  rk.status.assign(nl, 1);
  rk_count.assign(nl, 0);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, "ranked phasings");
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  std::vector<char> asked(nl, 0);  // the passes run over the individuals asked for, not the whole shard
  for (int i = 0; i < nl; ++i) asked[i] = rk.row_off[i + 1] > rk.row_off[i];
  const int rc = xp_pass(XP_RANK, "ranked phasings", &asked);
  rk_ms_struct = xp_ms_struct;
  rk_ms_fb = xp_ms_fb;
  rk_ms_sweep = xp_ms_sites;
  rk_groups = xp_groups;
  rk_pruned = xp_pruned;
  rk_built = rank_width(k);
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  rk.hap = nullptr;
  rk.prob = nullptr;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = local(q), stt = rk.status[i], cnt = stt == 0 ? rk_count[i] : 0;
    if (status) status[q] = stt;
    if (count) count[q] = cnt;
    // rows past the count (all of them for an unresolved individual or a subnormal P(genotype)): the input
    // genotype, as hmc_get_resolutions gives it, at probability 0
    for (int r = cnt; r < k; ++r) {
      if (prob) prob[(size_t)q * k + r] = 0.0;
      if (hap)
        for (int side = 0; side < 2; ++side)
          for (int l = 0; l < L; ++l)
            hap[(((size_t)q * k + r) * 2 + side) * L + l] = pan.symbol(l, pan.idx[((size_t)(i0 + i) * 2 + side) * L + l]);
    }
  }
  return HMC_OK;
}

int Ctx::genotype_likelihoods(int64_t n, const int32_t *indiv, double *mantissa, int32_t *exponent, int32_t *status) {
  if (!have_estep) return fail(HMC_EARG, "genotype likelihoods need an E-step first (hmc_resolve_all)");
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "genotype likelihoods: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44) return fail(HMC_EUNSUPPORTED, "genotype likelihoods with more than 44 alleles per locus");
  const int nl = nloc();
  if (!indiv) n = nl;
  if (n < 0) return fail(HMC_EARG, "genotype likelihoods: n = %lld is negative", (long long)n);
  for (int64_t q = 0; indiv && q < n; ++q)
    if (indiv[q] < i0 || indiv[q] >= i1)
      return fail(HMC_EARG, "genotype likelihoods: entry %lld: individual %d is outside this rank's shard [%d, %d)",
                  (long long)q, indiv[q], i0, i1);
  lk_ms_struct = lk_ms_fb = 0;
  lk_groups = 0;
  if (n == 0) return HMC_OK;
  auto local = [&](int64_t q) { return indiv ? indiv[q] - i0 : (int)q; };
  lk.mantissa.assign(nl, 0.0);
  lk.exponent.assign(nl, 0);
  lk.status.assign(nl, 1);
  hipError_t er;
  if ((er = d_xstatus.ensure(nl)) || (er = d_xre.ensure(nl)) || (er = d_xfmax.ensure(nl))) return hipfail(er, "genotype likelihoods");
  // the pass counts in the genotype posteriors' fields: theirs are put back
  const double g_struct = xp_ms_struct, g_fb = xp_ms_fb, g_sites = xp_ms_sites;
  const int g_groups = xp_groups, g_pruned = xp_pruned;
  std::vector<char> asked(nl, 0);  // the passes run over the individuals asked for, not the whole shard
  for (int64_t q = 0; q < n; ++q) asked[local(q)] = 1;
  const int rc = xp_pass(XP_LIK, "genotype likelihoods", &asked);
  lk_ms_struct = xp_ms_struct;
  lk_ms_fb = xp_ms_fb;
  lk_groups = xp_groups;
  xp_ms_struct = g_struct;
  xp_ms_fb = g_fb;
  xp_ms_sites = g_sites;
  xp_groups = g_groups;
  xp_pruned = g_pruned;
  if (rc) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const int i = local(q);
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
  hipError_t e;
  hipEventRecord(ev[0], st);
  if ((e = launch_exact_site_posteriors(x, s, std::max(1, std::min(k, dev_cu * 8)), st))) return hipfail(e, "exact_site_posteriors");
  hipEventRecord(ev[1], st);
  if ((e = sync_st())) return hipfail(e, "exact_site_posteriors");
  float ms = 0;
  hipEventElapsedTime(&ms, ev[0], ev[1]);
  xp_ms_sites += ms;
  return HMC_OK;
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
  int rc;
  while (true) {  // a capacity overflow restarts the pass; every site is written again
    xc_groups = 0;
    xp_ms_fb = xp_ms_sites = 0;
    if (mode == XP_SWITCH) sw_spilled = 0;
    if (mode == XP_PAIR) pr_spilled = 0;
    if (mode == XP_DOSE) ds_spilled = 0;
    rc = estep_split(order, true);
    if (rc != ESTEP_RESTART) break;
  }
  xp_mode = XP_OFF;
  xc_reuse = false;
  xp_ms_struct = ms_s1 + ms_fb;  // (ms_fb: the pruned structure re-runs of underflowing individuals)
  xp_groups = xc_groups;
  xp_pruned = exact_pruned;
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
  if (!have_estep) return fail(HMC_EARG, "genotype posteriors need an E-step first (hmc_resolve_all)");
  // P(genotype) of the last E-step is the divisor: the table must still be the one it ran on
  if (estep_gen != model_gen)
    return fail(HMC_EARG, "genotype posteriors: the model changed since the last E-step (hmc_resolve_all again)");
  if (pan.amax > 44)  // the records pack a locus's allele pairs (amax (amax + 1) / 2) in 10 bits
    return fail(HMC_EUNSUPPORTED, "genotype posteriors with more than 44 alleles per locus");
  const int n = nloc(), NP = pan.amax * (pan.amax + 1) / 2;
  SiteList own;
  if (!pre) site_list(own);
  const std::vector<unsigned long long> &off = pre ? pre->off : own.off;
  const std::vector<int32_t> &loc = pre ? pre->locus : own.locus;
  const size_t ns = loc.size();
  n_sites_last = ns;
  xp_ms_struct = xp_ms_fb = xp_ms_sites = 0;
  xp_groups = xp_pruned = 0;
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
  const int rc = xp_pass(XP_GENOTYPE, "posteriors");
  if (rc) return rc;
  if ((status && (er = hipMemcpyAsync(status, d_site_status.p, ns * 4, hipMemcpyDeviceToHost, st))) ||
      (post && (er = hipMemcpyAsync(post, d_site_post.p, ns * NP * 8, hipMemcpyDeviceToHost, st))) || (er = sync_st()))
    return hipfail(er, "posteriors");
  return HMC_OK;
}

int Ctx::exact_walk_group(ExactArgs &x, int k, int dev_cu) {
  if (exact_ipw == 2) return exact_walk_bfs(x, k, dev_cu);  // (variants)
  const int L = pan.L;
  hipError_t e;
  if (exact_walk_lds_bytes(tr_maxd, x.fmax, x.width) > EXACT_WALK_LDS_MAX)
    return fail(HMC_EUNSUPPORTED, "exact M-step: a frontier of %d states (trie depth %d) exceeds the walk's LDS bitmap",
                x.fmax, tr_maxd);
  // (variants) items per wavefront: 4 (16 lanes each) when their LDS fits, else 1
  const int ipw = exact_ipw == 4 && exact_walk_lds_bytes(tr_maxd, x.fmax, x.width) * 4 <= EXACT_WALK_LDS_MAX ? 4 : 1;
  {  // the largest list span of any item of the group (the per-wave scratch)
    unsigned span = 0;
    if ((e = d_xspan.ensure(1))) return hipfail(e, "exact_span");
    x.span_max = d_xspan.p;
    if ((e = hipMemsetAsync(d_xspan.p, 0, 4, st)) || (e = launch_exact_span(x, std::max(1, std::min(k, dev_cu * 8)), st)) ||
        (e = hipMemcpyAsync(&span, d_xspan.p, 4, hipMemcpyDeviceToHost, st)) || (e = sync_st()))
      return hipfail(e, "exact_span");
    x.span = std::max<long long>(span, 1);
  }
  x.scratch_stride = exact_walk_scratch_doubles(tr_maxd, x.span, x.width);
  const long long items = (long long)k * L;
  // 28 waves per CU, fewer when the per-item lists would pass SCRATCH_MAX
  const long long by_mem = std::max<long long>(1, (long long)(SCRATCH_MAX / (x.scratch_stride * 8 * ipw)));
  const int grid = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(items, (long long)dev_cu * 28), by_mem));
  // the walk's zero invariant (its lists; the child frequencies and touched
  // lists are left behind by each item and would land inside the lists of
  // a group whose depth or frontier differs): zeroed for every group
  const size_t need = x.scratch_stride * grid * ipw;
  if ((e = d_xscr.ensure(need)) || (e = hipMemsetAsync(d_xscr.p, 0, need * 8, st)))
    return hipfail(e, "exact scratch");
  x.scratch = d_xscr.p;
  // long walks (over 4 M items) in 16 slices, so that they report progress
  // (the lists return to zero between slices: every item clears its entries)
  const long long slice = items > (4ll << 20) ? std::max<long long>(grid, (items + 15) / 16) : items;
  for (long long i0 = 0; i0 < items; i0 += slice) {
    x.item0 = i0;
    x.item1 = std::min(items, i0 + slice);
    hipEventRecord(ev[0], st);
    if ((e = launch_exact_walk(x, grid, st, ipw))) return hipfail(e, "exact_walk");
    hipEventRecord(ev[1], st);
    if ((e = sync_st())) return hipfail(e, "exact_walk");
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[1]);
    ms_walk += ms;
    if (debug_mem)
      fprintf(stderr, "[hmc] exact walk: items %lld..%lld of %lld (%d individuals), %.1f ms; grid %d (%.1f waves per CU), "
              "fmax %d, depth %d, %.1f MB per wave\n", i0, x.item1, items, k, ms, grid, (double)grid / dev_cu, x.fmax, tr_maxd,
              x.scratch_stride * 8e-6);
  }
  return HMC_OK;
}

int Ctx::exact_walk_bfs(ExactArgs &x, int k, int dev_cu) {
  const int L = pan.L, fmax = std::max(x.fmax, 1);
  const long long items = (long long)k * L;
  hipError_t e;
  // lanes: 8 waves per CU; each owns [a side | b side][3][fmax] accumulators and a state bitmap
  const int grid = dev_cu * 2, nthr = grid * 256;
  const size_t lacc = 6 * (size_t)fmax, lbits = (size_t)fmax / 32 + 2;
  // unit and entry pools: a third of what is free (entries 28 B, units 32 B)
  size_t freeb = 0, totb = 0;
  hipMemGetInfo(&freeb, &totb);
  const double scratch_b = (double)nthr * (lacc * 8 + lbits * 4);
  const double pool_b = std::max(256e6, std::min(24e9, ((double)freeb - scratch_b) / 3.0));
  const unsigned long long ecap = (unsigned long long)(pool_b * 0.8 / 28.0), ucap = (unsigned long long)(pool_b * 0.2 / 32.0);
  const long long batch = std::max<long long>(1, std::min<long long>({items, (long long)(ecap / (2ull * (unsigned long long)fmax)),
                                                                        (long long)ucap / 2, 1ll << 30}));
  if ((e = d_xu_q.ensure(ucap)) || (e = d_xu_start.ensure(ucap)) || (e = d_xu_node.ensure(ucap)) || (e = d_xu_freq.ensure(ucap)) ||
      (e = d_xu_e0.ensure(ucap)) || (e = d_xu_ne.ensure(ucap)) || (e = d_xe_t.ensure(ecap)) || (e = d_xe_w.ensure(3 * ecap)) ||
      (e = d_xcur.ensure(2)) || (e = d_xndef.ensure(1)) || (e = d_xdef.ensure(std::max<size_t>((size_t)batch, ucap))) ||
      (e = d_xidx.ensure(std::max<size_t>((size_t)batch, ucap))) || (e = d_xlacc.ensure((size_t)nthr * lacc)) ||
      (e = d_xlbits.ensure((size_t)nthr * lbits)) || (e = hipMemsetAsync(d_xlacc.p, 0, (size_t)nthr * lacc * 8, st)) ||
      (e = hipMemsetAsync(d_xlbits.p, 0, (size_t)nthr * lbits * 4, st)))
    return hipfail(e, "exact walk pools");
  XWalkArgs w;
  w.u.q = d_xu_q.p;
  w.u.start = d_xu_start.p;
  w.u.node = d_xu_node.p;
  w.u.freq = d_xu_freq.p;
  w.u.e0 = d_xu_e0.p;
  w.u.ne = d_xu_ne.p;
  w.e_t = d_xe_t.p;
  w.e_w = d_xe_w.p;
  w.e_cap = ecap;
  w.u_cap = ucap;
  w.cursor = d_xcur.p;
  w.defer = d_xdef.p;
  w.n_defer = d_xndef.p;
  w.lacc = d_xlacc.p;
  w.lbits = d_xlbits.p;
  w.lacc_stride = lacc;
  w.lbits_stride = lbits;
  x.scratch = nullptr;
  hipEventRecord(ev[0], st);
  // One level: the units [in_base, in_base + n) (or the listed ones) at
  // `depth`, outputs from (u_top, e_top); then the next level over those
  // outputs, then — with the pools above free again — the deferred units (a
  // loop at the same depth: the recursion is as deep as the trie only).
  std::function<int(int, bool, unsigned long long, std::vector<int32_t> *, int, unsigned long long, unsigned long long)> level;
  level = [&](int depth, bool roots, unsigned long long in_base, std::vector<int32_t> *idx0, int n,
              unsigned long long u_top, unsigned long long e_top) -> int {
    std::vector<int32_t> idx_v;
    if (idx0) idx_v.swap(*idx0);
    bool listed = idx0 != nullptr;
    while (n > 0) {
      hipError_t e2;
      const unsigned long long cur0[2] = {u_top, e_top};
      const int zero = 0;
      if ((e2 = hipMemcpyAsync(d_xcur.p, cur0, 16, hipMemcpyHostToDevice, st)) ||
          (e2 = hipMemcpyAsync(d_xndef.p, &zero, 4, hipMemcpyHostToDevice, st)) ||
          (listed && (e2 = hipMemcpyAsync(d_xidx.p, idx_v.data(), idx_v.size() * 4, hipMemcpyHostToDevice, st))) ||
          (listed && (e2 = sync_st())))
        return hipfail(e2, "exact walk");
      XWalkArgs w2 = w;
      w2.in_base = in_base;
      w2.idx = listed ? d_xidx.p : nullptr;
      w2.n_in = n;
      w2.depth = depth;
      w2.roots = roots;
      if ((e2 = launch_exact_walk_units(x, w2, std::max(1, std::min(grid, (n + 255) / 256)), st)))
        return hipfail(e2, "exact_walk_units");
      unsigned long long cur[2];
      int nd = 0;
      if ((e2 = hipMemcpyAsync(cur, d_xcur.p, 16, hipMemcpyDeviceToHost, st)) ||
          (e2 = hipMemcpyAsync(&nd, d_xndef.p, 4, hipMemcpyDeviceToHost, st)) || (e2 = sync_st()))
        return hipfail(e2, "exact walk");
      ++xw_launches;
      xw_units += n;
      std::vector<int32_t> def((size_t)nd);
      if (nd && ((e2 = hipMemcpyAsync(def.data(), d_xdef.p, (size_t)nd * 4, hipMemcpyDeviceToHost, st)) ||
                 (e2 = sync_st())))
        return hipfail(e2, "exact walk");
      const unsigned long long u_end = std::min(cur[0], ucap), e_end = std::min(cur[1], ecap);
      if (nd == n && u_end == u_top)
        return fail(HMC_ENOMEM, "exact M-step: one trie node's children exceed the walk's pools (%llu units, %llu entries)",
                    ucap, ecap);
      int rc2;
      if (u_end > u_top && (rc2 = level(depth + 1, false, u_top, nullptr, (int)(u_end - u_top), u_end, e_end))) return rc2;
      xw_defers += nd;
      std::sort(def.begin(), def.end());  // (any order gives the same sums: fixed-point adds)
      idx_v.swap(def);
      listed = true;
      n = nd;
    }
    return HMC_OK;
  };
  for (long long b = 0; b < items; b += batch) {
    const int nb = (int)std::min<long long>(batch, items - b);
    int rc = level(0, true, (unsigned long long)b, nullptr, nb, 0, 0);
    if (rc) return rc;
  }
  hipEventRecord(ev[1], st);
  if ((e = sync_st())) return hipfail(e, "exact walk");
  float ms = 0;
  hipEventElapsedTime(&ms, ev[0], ev[1]);
  ms_walk += ms;
  if (debug_mem)
    fprintf(stderr, "[hmc] exact walk (breadth-first): %lld items, %d individuals, %.1f ms; %lld units in %lld launches, "
            "%lld deferred; pools %llu units / %llu entries\n", items, k, ms, xw_units, xw_launches, xw_defers, ucap, ecap);
  return HMC_OK;
}

void Ctx::host_successors(const Cands &c, std::vector<int32_t> &succ) {
  const int L = pan.L, A = pan.amax;
  const size_t P = c.size();
  std::vector<int32_t> child, data, root(L, -1);
  auto new_node = [&]() {
    child.insert(child.end(), A, -1);
    data.push_back(-1);
    return (int32_t)data.size() - 1;
  };
  for (size_t k = 0; k < P; ++k) {
    const int s = c.start[k];
    if (root[s] < 0) root[s] = new_node();
    int32_t u = root[s];
    const uint8_t *al = c.alleles(k);
    for (int q = 0; q < c.len[k]; ++q) {
      int32_t v = child[(size_t)u * A + al[q]];
      if (v < 0) {
        v = new_node();
        child[(size_t)u * A + al[q]] = v;
      }
      u = v;
    }
    data[u] = (int32_t)k;
  }
  succ.assign(P * A, -1);
  for (size_t k = 0; k < P; ++k) {
    const int s = c.start[k], ln = c.len[k], e = s + ln;
    if (e >= L) continue;
    const uint8_t *al = c.alleles(k);
    for (int j = 0; j < h_anum[e]; ++j) {
      int32_t res = -1;
      for (int s2 = s; s2 <= e && res < 0; ++s2) {  // longest first
        int32_t u = root[s2];
        for (int q = s2 - s; q < ln && u >= 0; ++q) u = child[(size_t)u * A + al[q]];
        if (u >= 0) u = child[(size_t)u * A + j];
        if (u >= 0) res = data[u];
      }
      succ[k * A + j] = res;
    }
  }
}

int Ctx::install_host_table(Cands &c, std::vector<int32_t> &succ) {
  const int P = (int)c.size(), A = pan.amax;
  if ((int64_t)P > INT32_MAX) return fail(HMC_EUNSUPPORTED, "too many patterns");
  int rc = alloc_table(std::max(P, 1));
  if (rc) return rc;
  std::vector<uint8_t> last(P);
  std::vector<int32_t> node(P, -1);
  std::vector<uint32_t> su((size_t)P * A);
  for (int i = 0; i < P; ++i) last[i] = c.alleles(i)[c.len[i] - 1];
  for (size_t i = 0; i < su.size(); ++i) su[i] = succ[i] < 0 ? NONE : (uint32_t)succ[i];
  hipError_t e;
  if (P && ((e = hipMemcpyAsync(t_start.p, c.start.data(), (size_t)P * 4, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_len.p, c.len.data(), (size_t)P * 4, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_node.p, node.data(), (size_t)P * 4, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_freq.p, c.freq.data(), (size_t)P * 8, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_prefix.p, c.prefix.data(), (size_t)P * 8, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_tp.p, c.tp.data(), (size_t)P * 8, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_last.p, last.data(), (size_t)P, hipMemcpyHostToDevice, st)) ||
            (e = hipMemcpyAsync(t_succ.p, su.data(), su.size() * 4, hipMemcpyHostToDevice, st)) ||
            (e = hipMemsetAsync(t_ppat.p, 0xFE, (size_t)P * 4, st)) ||  // alleles are kept on the host (ht)
            (e = sync_st())))
    return hipfail(e, "exact: install table");
  this->P = P;
  // head list: start 0, length head_len, id order (PatternManager.cpp:304-306)
  std::vector<std::pair<uint32_t, uint8_t>> heads;
  h_head_ids.clear();
  h_head_al.clear();
  std::vector<uint8_t> tab;
  if (head_len > 1) tab.assign((size_t)std::max(P, 1) * head_len, 0);
  for (int i = 0; i < P; ++i)
    if (c.start[i] == 0 && c.len[i] == head_len) {
      heads.push_back({(uint32_t)i, c.alleles(i)[head_len - 1]});
      if (head_len > 1) {
        h_head_ids.push_back((uint32_t)i);
        h_head_al.insert(h_head_al.end(), c.alleles(i), c.alleles(i) + head_len);
        std::copy(c.alleles(i), c.alleles(i) + head_len, tab.begin() + (size_t)i * head_len);
      }
    }
  if (head_len > 1 && ((e = d_head_al.ensure(tab.size())) ||
                       (e = hipMemcpyAsync(d_head_al.p, tab.data(), tab.size(), hipMemcpyHostToDevice, st)) ||
                       (e = sync_st())))
    return hipfail(e, "exact: heads");
  if ((rc = set_heads(heads))) return rc;
  ht = c;
  ht_succ = succ;
  table_on_host = true;
  have_model = true;
  new_table(false);
  return HMC_OK;
}

int Ctx::estimate_patterns(int *P_out, uint64_t *rm_out) {
  if (!have_estep) return fail(HMC_EARG, "exact M-step needs an E-step first");
  // after findPatternByNum the reference estimates at that search's last
  // threshold (m_min_freq, PatternManager.cpp:53-60, 364-408)
  const bool bynum = num_patterns > 0 && model != 1;
  if (bynum && !(bynum_theta_last > 0))
    return fail(HMC_EARG, "exact M-step after findPatternByNum needs the search's threshold (mine first)");
  if (pan.amax > 44)  // the records pack a locus's allele pairs (amax (amax + 1) / 2) in 10 bits
    return fail(HMC_EUNSUPPORTED, "exact M-step with more than 44 alleles per locus");
  hipEventRecord(ev[4], st);
  const int L = pan.L;
  int mxl = max_len <= 0 ? L : max_len;  // m_max_len / m_min_len of the last findPatternByFreq
  int mnl = std::max(min_len, 1);
  mxl = std::max(mxl, mnl);
  double mf = bynum ? bynum_theta_last : current_min_freq();
  if (model == 1) {  // findPatternBlock: m_min_freq = -1 (PatternManager.cpp:75-88)
    mnl = mxl = std::max(1, mc_order + 1);
    mf = -1.0;
  }
  exact_rounds = 0;
  exact_candidates = 0;
  ms_walk = 0;
  xw_units = xw_launches = xw_defers = 0;
  exact_pruned = 0;
  xc_reuse = false;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  auto t0 = clk::now();
  Cands cur;
  std::vector<int32_t> succ;
  int rc = table_to_host(cur, succ);
  if (rc) return rc;
  const double ms_to_host = ms_since(t0);
  t0 = clk::now();
  const int A = pan.amax;
  if (mf < 0) {  // estimateFrequency() (:347-362): re-estimate in place, ids and successors unchanged
    if ((rc = estimate_round(cur, 0, cur.size()))) return rc;
    if ((rc = install_host_table(cur, succ))) return rc;
  } else {
    Cands all;
    std::vector<size_t> seeds;
    for (size_t i = 0; i < cur.size(); ++i) {
      all.push(cur.start[i], cur.len[i], cur.alleles(i), 0, false, cur.freq[i], cur.prefix[i], cur.tp[i]);
      const int s = cur.start[i], e = s + cur.len[i];
      if (e < L && cur.len[i] < mxl)
        for (int j = 0; j < h_anum[e]; ++j) {
          const int32_t sj = succ[i * A + j];
          if (sj < 0 || cur.start[sj] != s) {  // the extension is not stored: a seed
            all.push(s, cur.len[i] + 1, cur.alleles(i), (uint8_t)j, true, cur.freq[i]);
            seeds.push_back(all.size() - 1);
          }
        }
    }
    size_t rb = 0, re = all.size();
    std::vector<uint8_t> buf;
    while (rb < re) {
      if ((rc = estimate_round(all, rb, re))) return rc;
      const size_t nb = all.size();
      for (int level = 0; level < 4; ++level) {  // extendPatterns (:412-438)
        std::vector<size_t> ns;
        for (size_t si : seeds) {
          const int s = all.start[si], ln = all.len[si], e = s + ln;
          if (e < L && ln < mxl && all.freq[si] >= mf) {
            buf.assign(all.alleles(si), all.alleles(si) + ln);
            const double f = all.freq[si];
            for (int j = 0; j < h_anum[e]; ++j) {
              all.push(s, ln + 1, buf.data(), (uint8_t)j, true, f);
              ns.push_back(all.size() - 1);
            }
          }
        }
        seeds.swap(ns);
      }
      rb = nb;
      re = all.size();
    }
    const double ms_rounds = ms_since(t0);
    t0 = clk::now();
    Cands kept;  // (:396-408)
    for (size_t i = 0; i < all.size(); ++i)
      if (all.freq[i] >= mf || all.len[i] <= mnl)
        kept.push(all.start[i], all.len[i], all.alleles(i), 0, false, all.freq[i], all.prefix[i], all.tp[i]);
    std::vector<int32_t> ksucc;
    host_successors(kept, ksucc);
    const double ms_succ = ms_since(t0);
    t0 = clk::now();
    if ((rc = install_host_table(kept, ksucc))) return rc;
    if (debug_mem)
      fprintf(stderr, "[hmc] exact M-step: table to host %.1f ms, rounds %.1f ms (walks %.1f), kept + successors %.1f ms, "
              "install %.1f ms\n", ms_to_host, ms_rounds, ms_walk, ms_succ, ms_since(t0));
  }
  xc_reuse = false;
  hipEventRecord(ev[5], st);
  hipError_t e;
  if ((e = sync_st())) return hipfail(e, "exact");
  // the walk's scratch (up to SCRATCH_MAX) and the tries go back to the E-step
  d_xscr.release();
  d_tr_child.release();
  d_tr_data.release();
  float ms = 0;
  hipEventElapsedTime(&ms, ev[4], ev[5]);
  ms_m = ms;
  if (P_out) *P_out = P;
  if (rm_out) *rm_out = 0;  // no candidate x item scans: the cost is in the trie walks
  return HMC_OK;
}
}  // namespace hmc
