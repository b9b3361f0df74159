// Host-only checks of the patch-sweep planner (csrc/sweep_plan.hpp): invariants over seeded random
// cases, one case worked out by hand, and every validation error by message.  Built and run by
// tests/test_sweep_plan.py under the address and undefined-behaviour sanitizers; exits non-zero
// with a message at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "sweep_plan.hpp"

using namespace tvr;

namespace {

std::string g_case;  // names the case in a failure message

#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) {                                                                               \
      std::fprintf(stderr, "%s:%d: %s: check failed: %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
      std::exit(1);                                                                              \
    }                                                                                            \
  } while (0)

template <class T>
bool same(const std::vector<T>& a, std::initializer_list<T> b) { return a == std::vector<T>(b); }
bool eq(const SeqDesc& a, const SeqDesc& b) {
  return a.row0 == b.row0 && a.n == b.n && a.p0 == b.p0 && a.cache_row == b.cache_row && a.q0 == b.q0 &&
         a.prefix_live == b.prefix_live;
}

// A trace and a sweep's arguments, owned; in() views them.
struct Case {
  int L = 4, H = 2, d_head = 16, entry_group = 8, n_vectors = 2;
  std::vector<int> seq_off, seq_len;
  std::vector<int32_t> tokens;
  bool fused = false, prefix_share = true, lin_wanted = false, have_vectors = true, aligned = true, sets = false;
  std::vector<tvr_site> sites;
  std::vector<int32_t> set_off;
  std::vector<tvr_head_patch> patches;

  void add_seq(std::initializer_list<int32_t> t) {
    seq_off.push_back((int)tokens.size());
    seq_len.push_back((int)t.size());
    tokens.insert(tokens.end(), t);
  }
  SweepPlanIn in() const {
    return SweepPlanIn{L, H, H * d_head, d_head, seq_off.data(), seq_len.data(), tokens.data(), (int)seq_len.size(),
                       (int)tokens.size(), fused, prefix_share, lin_wanted, entry_group, n_vectors, have_vectors,
                       aligned, 4.0, sites.data(), (int)sites.size(), sets ? set_off.data() : nullptr,
                       patches.data()};
  }
};

tvr_site site(int seq, int kind, int layer = 0, int head = 0, int vec = 0, int pos = 0, int src_seq = 0,
              int src_pos = 0) {
  return tvr_site{seq, kind, layer, head, pos, src_seq, src_pos, vec, -1};
}

// --- a) invariants ----------------------------------------------------------------------------------------------

Case random_case(std::mt19937& rng) {
  auto r = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  Case c;
  c.L = r(1, 6);
  c.H = r(0, 1) ? 4 : 2;
  c.entry_group = r(1, 4);
  c.n_vectors = r(1, 3);
  c.fused = r(0, 1);
  c.prefix_share = r(0, 1);
  c.lin_wanted = r(0, 1);
  c.sets = r(0, 1);
  const int n_seq = r(1, 6), n_sites = r(1, 40);
  for (int s = 0; s < n_seq; ++s) {
    c.seq_off.push_back((int)c.tokens.size());
    c.seq_len.push_back(r(1, 7));
    for (int t = 0; t < c.seq_len[s]; ++t) c.tokens.push_back(r(0, 2));
  }
  // mostly head replacements in half of the cases, so that whole layers linearise and prefixes are shared
  const bool mostly_heads = r(0, 1);
  static const int plain_kinds[] = {0, 1, 2, 3, 6};
  c.set_off.push_back(0);
  for (int i = 0; i < n_sites; ++i) {
    const int seq = r(0, n_seq - 1), T = c.seq_len[seq], src = r(0, n_seq - 1);
    const int kind = mostly_heads && r(0, 7) ? 1 : c.sets ? r(0, 6) : plain_kinds[r(0, 4)];
    tvr_site s = site(seq, kind, r(0, c.L - 1), r(0, c.H - 1), r(0, c.n_vectors - 1), r(0, T - 1), src,
                      r(0, c.seq_len[src] - 1));
    s.target = r(-1, 5);
    c.sites.push_back(s);
    if (kind == 4 || kind == 5) {
      std::set<std::pair<int, int>> used;
      for (int q = r(0, 4); q > 0; --q) {
        const int l = r(0, c.L - 1), h = r(0, c.H - 1);
        if (used.insert({l, h}).second) c.patches.push_back(tvr_head_patch{l, h, r(0, c.n_vectors - 1)});
      }
    }
    c.set_off.push_back((int32_t)c.patches.size());
  }
  return c;
}

void check_rows(const Case& c, const SweepPlanIn& in, const SweepPlan& p) {
  const int n = in.n_sites, L = c.L;
  CHECK(p.Rc == (c.fused ? in.n_tokens : 0) && p.nc == (c.fused ? in.n_seq : 0));
  for (auto* v : {&p.entry, &p.p0, &p.nrow, &p.row0, &p.leader, &p.order}) CHECK((int)v->size() == n);
  CHECK((int)p.cnt_le.size() == L + 1 && (int)p.rows_le.size() == L + 1);
  // each site's entry layer and rows by its kind's rule; the rows end at the last position
  int maxT = 0;
  bool single = true;
  for (int s = 0; s < p.nc; ++s) maxT = std::max(maxT, c.seq_len[s]);
  for (int i = 0; i < n; ++i) {
    const tvr_site& s = c.sites[i];
    const int T = c.seq_len[s.seq];
    int l_min = L;
    if (c.sets)
      for (int q = c.set_off[i]; q < c.set_off[i + 1]; ++q) l_min = std::min(l_min, (int)c.patches[q].layer);
    const int entry = s.kind == 0 ? L : s.kind == 1 || s.kind == 2 ? s.layer + 1 : s.kind == 3 || s.kind == 6 ? s.layer : l_min;
    const int p0 = s.kind == 1 || (s.kind == 4 && l_min < L) ? 0 : s.kind == 3 || s.kind == 6 ? s.pos : T - 1;
    CHECK(p.entry[i] == entry);
    CHECK(p.p0[i] + p.nrow[i] == T && p.nrow[i] >= 1);
    if (p.leader[i] < 0) CHECK(p.p0[i] == p0);
    maxT = std::max(maxT, T);
    single = single && T - p0 == 1;
  }
  CHECK(p.maxT == maxT && p.single_rows == single);
  // order: a stable sort by entry; rows: disjoint ranges covering [0, R), laid out in that order
  std::vector<char> seen(n, 0), row_used(p.R, 0);
  for (int k = 0, rows = 0; k < n; ++k) {
    const int i = p.order[k];
    CHECK(i >= 0 && i < n && !seen[i]);
    seen[i] = 1;
    if (k > 0) {
      const int j = p.order[k - 1];
      CHECK(p.entry[j] < p.entry[i] || (p.entry[j] == p.entry[i] && j < i));
    }
    CHECK(p.row0[i] == rows);
    for (int q = 0; q < p.nrow[i]; ++q) {
      CHECK(p.row0[i] + q < p.R && !row_used[p.row0[i] + q]);
      row_used[p.row0[i] + q] = 1;
    }
    rows += p.nrow[i];
    if (k == n - 1) CHECK(rows == p.R);
  }
  for (int l = 0; l <= L; ++l) {
    int cnt = 0, rows = 0;
    for (int i = 0; i < n; ++i)
      if (p.entry[i] <= l) { ++cnt; rows += p.nrow[i]; }
    CHECK(p.cnt_le[l] == cnt && p.rows_le[l] == rows);
  }
}

void check_followers(const Case& c, const SweepPlan& p) {
  std::map<std::tuple<int, int, int, int>, int> first;
  for (int i = 0; i < (int)c.sites.size(); ++i) {
    const tvr_site& s = c.sites[i];
    const int ld = p.leader[i], T = c.seq_len[s.seq];
    const int32_t* tk = c.tokens.data() + c.seq_off[s.seq];
    if (!c.prefix_share || s.kind != 1) {
      CHECK(ld == -1);
      continue;
    }
    const int head_of_key = first.emplace(std::make_tuple(s.layer, s.head, s.vec, (int)tk[0]), i).first->second;
    if (ld < 0) {  // the first site of its patch and first token, or too short to share a row
      CHECK(head_of_key == i || T == 1);
      continue;
    }
    const tvr_site& sl = c.sites[ld];
    CHECK(ld < i && ld == head_of_key && p.leader[ld] == -1);
    CHECK(sl.kind == 1 && sl.layer == s.layer && sl.head == s.head && sl.vec == s.vec);
    const int32_t* tl = c.tokens.data() + c.seq_off[sl.seq];
    const int P = p.p0[i], cap = std::min(T - 1, c.seq_len[sl.seq]);
    CHECK(1 <= P && P <= cap);
    for (int j = 0; j < P; ++j) CHECK(tk[j] == tl[j]);
    CHECK(P == cap || tk[P] != tl[P]);
  }
}

void check_tables(const Case& c, const SweepPlanIn& in, const SweepPlan& p) {
  const int n = in.n_sites, Rc = p.Rc, nc = p.nc;
  CHECK((int)p.seqs.size() == nc + n && (int)p.seqs_last.size() == nc + n && (int)p.ents.size() == n);
  CHECK((int)p.last.size() == n && (int)p.tg.size() == n && (int)p.last_sorted.size() == Rc + n);
  CHECK((int)p.clean_last.size() == nc);
  for (int s = 0; s < nc; ++s) {
    CHECK(eq(p.seqs[s], SeqDesc{c.seq_off[s], c.seq_len[s], 0, -1, 0, 0}) && eq(p.seqs_last[s], p.seqs[s]));
    CHECK(p.clean_last[s] == c.seq_off[s] + c.seq_len[s] - 1);
  }
  for (int r = 0; r < Rc; ++r) CHECK(p.last_sorted[r] == r);
  for (int k = 0; k < n; ++k) {
    const int i = p.order[k], ld = p.leader[i];
    const tvr_site& s = c.sites[i];
    const int srow = c.seq_off[s.seq];
    const SeqDesc want{Rc + p.row0[i], p.nrow[i], p.p0[i], ld >= 0 ? Rc + p.row0[ld] : srow, 0, ld >= 0 ? 1 : 0};
    CHECK(eq(p.seqs[nc + k], want));
    SeqDesc want_last = want;
    want_last.q0 = want.n - 1;
    CHECK(eq(p.seqs_last[nc + k], want_last));
    const EntryDesc& e = p.ents[k];
    CHECK(e.kind == (s.kind == 4 || s.kind == 5 ? 0 : s.kind) && e.row0 == want.row0 && e.n == want.n && e.p0 == want.p0);
    CHECK(e.src_row == srow && e.src2_row == (s.kind == 3 ? c.seq_off[s.src_seq] + s.src_pos : 0));
    CHECK(e.patch_pos == s.pos && e.head == s.head && e.vec == s.vec && e.pad == 0);
    CHECK(p.last[i] == Rc + p.row0[i] + p.nrow[i] - 1 && p.tg[i] == s.target);
    CHECK(p.last_sorted[Rc + k] == p.last[i]);
  }
}

void check_entry_groups(const Case& c, const SweepPlan& p) {
  const int L = c.L;
  CHECK((int)p.ent_other.size() == L + 1 && (int)p.eg_beg.size() == L + 1 && (int)p.eg_cnt.size() == L + 1);
  CHECK((int)p.entry_bytes.size() == L + 1);
  int groups = 0, indices = 0;
  for (int l = 0; l <= L; ++l) {
    const int k0 = l > 0 ? p.cnt_le[l - 1] : 0, k1 = p.cnt_le[l];
    std::map<int, int> n_head;  // REPLACE_HEAD entries of the layer per head
    bool other = false;
    for (int k = k0; k < k1; ++k) {
      if (p.ents[k].kind == 1) ++n_head[p.ents[k].head];
      else other = true;
    }
    CHECK((p.ent_other[l] != 0) == other);
    CHECK(p.eg_beg[l] == groups && p.eg_beg[l] + p.eg_cnt[l] <= (int)p.egroups.size());
    std::set<int> used;
    std::map<int, std::vector<int>> sizes;
    for (int g = p.eg_beg[l]; g < p.eg_beg[l] + p.eg_cnt[l]; ++g) {
      const EntryGroup& eg = p.egroups[g];
      CHECK(eg.first == indices && eg.count >= 1 && eg.count <= c.entry_group);
      CHECK(eg.first + eg.count <= (int)p.egidx.size());
      const int head = p.ents[p.egidx[eg.first]].head;
      for (int x = eg.first; x < eg.first + eg.count; ++x) {
        const int k = p.egidx[x];
        CHECK(k >= k0 && k < k1 && p.ents[k].kind == 1 && p.ents[k].head == head && used.insert(k).second);
      }
      sizes[head].push_back(eg.count);
      indices += eg.count;
    }
    groups += p.eg_cnt[l];
    CHECK(sizes.size() == n_head.size());
    for (const auto& hs : sizes) {
      int total = 0, lo = hs.second[0], hi = hs.second[0];
      for (int x : hs.second) { total += x; lo = std::min(lo, x); hi = std::max(hi, x); }
      CHECK(total == n_head[hs.first] && hi - lo <= 1);
      CHECK((int)hs.second.size() == (total + c.entry_group - 1) / c.entry_group);
    }
  }
  CHECK(groups == (int)p.egroups.size() && indices == (int)p.egidx.size());
}

void check_headsets(const Case& c, const SweepPlan& p) {
  const int L = c.L, n = (int)c.sites.size();
  CHECK((int)p.hs_beg.size() == L + 1 && (int)p.hs_max_rows.size() == L && (int)p.hs_bytes.size() == L);
  size_t item = 0, patch = 0;
  for (int l = 0; l < L; ++l) {
    CHECK(p.hs_beg[l] == (int)item);
    int max_rows = 0;
    for (int k = 0; k < n && c.sets; ++k) {  // the items in entry order, each item's heads in the caller's order
      const int i = p.order[k], first = (int)patch;
      for (int q = c.set_off[i]; q < c.set_off[i + 1]; ++q) {
        if (c.patches[q].layer != l) continue;
        CHECK(patch < p.hs_patches.size());
        CHECK(p.hs_patches[patch].head == c.patches[q].head && p.hs_patches[patch].vec == c.patches[q].vec);
        ++patch;
      }
      if ((int)patch == first) continue;
      CHECK(item < p.hs_items.size());
      const HeadsetItem& it = p.hs_items[item++];
      CHECK(it.row0 == p.Rc + p.row0[i] && it.n_rows == p.nrow[i] && it.first_patch == first);
      CHECK(it.n_patches == (int)patch - first);
      max_rows = std::max(max_rows, p.nrow[i]);
    }
    CHECK(p.hs_max_rows[l] == max_rows);
  }
  CHECK(p.hs_beg[L] == (int)item && item == p.hs_items.size() && patch == p.hs_patches.size());
}

void check_lin(const Case& c, const SweepPlan& p) {
  const int L = c.L;
  CHECK((int)p.use_lin.size() == L);
  for (auto* v : {&p.lin_vid_off, &p.lin_nv, &p.lin_mb_off, &p.lin_nmb, &p.lin_nrows}) CHECK((int)v->size() == L);
  int vids = 0, rows = 0, mbs = 0, max_nv = 0;
  for (int l = 0; l < L; ++l) {
    const int k0 = l > 0 ? p.cnt_le[l - 1] : 0, k1 = p.cnt_le[l];
    bool all_heads = k1 > k0;
    for (int k = k0; k < k1; ++k) all_heads = all_heads && c.sites[p.order[k]].kind == 1;
    CHECK((p.use_lin[l] != 0) == (c.lin_wanted && 1 <= l && l <= L - 2 && all_heads));
    if (!p.use_lin[l]) {
      CHECK(p.lin_nv[l] == 0 && p.lin_nmb[l] == 0 && p.lin_nrows[l] == 0);
      continue;
    }
    CHECK(p.lin_vid_off[l] == vids && p.lin_mb_off[l] == mbs);
    // every entering row once, with its clean row and its vector; the vectors distinct
    std::map<int, std::tuple<int, int, int>> want;  // activation row -> (clean row, vector, head)
    std::set<int> vecs;
    for (int k = k0; k < k1; ++k) {
      const int i = p.order[k];
      const tvr_site& s = c.sites[i];
      vecs.insert(s.vec);
      for (int q = 0; q < p.nrow[i]; ++q)
        want[p.Rc + p.row0[i] + q] = std::make_tuple(c.seq_off[s.seq] + p.p0[i] + q, s.vec, s.head);
    }
    CHECK(p.lin_nv[l] == (int)vecs.size() && p.lin_nrows[l] == (int)want.size());
    CHECK(vids + p.lin_nv[l] <= (int)p.lin_vids.size() && rows + p.lin_nrows[l] <= (int)p.lin_rows.size());
    CHECK(std::set<int>(p.lin_vids.begin() + vids, p.lin_vids.begin() + vids + p.lin_nv[l]) == vecs);
    CHECK(mbs + p.lin_nmb[l] <= (int)p.lin_mbs.size());
    int next = rows;  // the m-blocks tile the layer's rows: at most 64 rows of one head each
    for (int b = mbs; b < mbs + p.lin_nmb[l]; ++b) {
      const LinMB& mb = p.lin_mbs[b];
      CHECK(mb.row0 == next && mb.rows >= 1 && mb.rows <= 64 && mb.pad == 0);
      CHECK(mb.row0 + mb.rows <= rows + p.lin_nrows[l]);
      for (int r = mb.row0; r < mb.row0 + mb.rows; ++r) {
        const LinRow& lr = p.lin_rows[r];
        const auto it = want.find(lr.out_row);
        CHECK(it != want.end());  // an entering row, not listed before
        CHECK(lr.clean_row == std::get<0>(it->second) && lr.vrow >= 0 && lr.vrow < p.lin_nv[l] && lr.pad == 0);
        CHECK(p.lin_vids[vids + lr.vrow] == std::get<1>(it->second) && mb.head == std::get<2>(it->second));
        want.erase(it);
      }
      next += mb.rows;
    }
    CHECK(want.empty() && next == rows + p.lin_nrows[l]);
    vids += p.lin_nv[l];
    rows += p.lin_nrows[l];
    mbs += p.lin_nmb[l];
    max_nv = std::max(max_nv, p.lin_nv[l]);
  }
  CHECK(vids == (int)p.lin_vids.size() && rows == (int)p.lin_rows.size() && mbs == (int)p.lin_mbs.size());
  CHECK(p.lin_max_nv == max_nv);
}

SweepPlan checked_plan(const Case& c) {
  const SweepPlanIn in = c.in();
  SweepPlan p;
  std::string err;
  CHECK(plan_sweep(in, p, err) == TVR_OK && err.empty());
  check_rows(c, in, p);
  check_followers(c, p);
  check_tables(c, in, p);
  check_entry_groups(c, p);
  check_headsets(c, p);
  check_lin(c, p);
  return p;
}

void check_invariants(int n_cases) {
  std::mt19937 rng(20240607u);
  int followers = 0, lin_layers = 0, set_items = 0;
  for (int t = 0; t < n_cases; ++t) {
    g_case = "random case " + std::to_string(t);
    const Case c = random_case(rng);
    SweepPlan p = checked_plan(c);
    for (int ld : p.leader) followers += ld >= 0;
    for (char u : p.use_lin) lin_layers += u != 0;
    set_items += (int)p.hs_items.size();
    p.drop_lin();
    CHECK(p.lin_vids.empty() && p.lin_rows.empty() && p.lin_mbs.empty() && p.lin_max_nv == 0);
    for (char u : p.use_lin) CHECK(u == 0);
  }
  g_case = "random cases";  // the generator reaches what the checks are about
  std::printf("%d cases: %d followers, %d linearised layers, %d head-set items\n", n_cases, followers, lin_layers,
              set_items);
  CHECK(followers > 100 && lin_layers > 50 && set_items > 100);

  // more than 64 entering rows of one head (the random cases stay below): 30 sites x 7 rows of head 1 and
  // 5 x 7 of head 0, one layer, no shared prefix
  g_case = "many rows of one head";
  Case c;
  c.L = 3;
  c.fused = c.lin_wanted = true;
  c.prefix_share = false;
  c.add_seq({0, 1, 2, 0, 1, 2, 0});
  for (int i = 0; i < 35; ++i) c.sites.push_back(site(0, 1, 0, i % 7 == 0 ? 0 : 1, i % 2));
  const SweepPlan p = checked_plan(c);
  CHECK(p.lin_nmb[1] == 5 && p.lin_nrows[1] == 245 && p.lin_nv[1] == 2);
  const int want_rows[5] = {35, 64, 64, 64, 18}, want_head[5] = {0, 1, 1, 1, 1};
  for (int b = 0; b < 5; ++b) CHECK(p.lin_mbs[b].rows == want_rows[b] && p.lin_mbs[b].head == want_head[b]);
}

// --- b) one exact case ------------------------------------------------------------------------------------------

Case exact_case() {
  Case c;
  c.add_seq({7, 1, 2});
  c.add_seq({7, 1, 3});
  c.add_seq({7, 4});
  c.sites = {site(0, 1, 1, 0, 0), site(1, 1, 1, 0, 0), site(2, 1, 1, 0, 0),
             site(0, 2, 0, 0, 1), site(1, 0),          site(2, 6, 0, 0, 0, 0)};
  return c;
}

void check_exact() {
  g_case = "exact case";
  Case c = exact_case();
  SweepPlan p;
  std::string err;
  CHECK(plan_sweep(c.in(), p, err) == TVR_OK);
  CHECK(same(p.entry, {2, 2, 2, 1, 4, 0}) && same(p.leader, {-1, 0, 0, -1, -1, -1}));
  CHECK(same(p.p0, {0, 2, 1, 2, 2, 0}) && same(p.nrow, {3, 1, 1, 1, 1, 2}));
  CHECK(same(p.order, {5, 3, 0, 1, 2, 4}) && same(p.row0, {3, 6, 7, 2, 8, 0}));
  CHECK(p.R == 9 && p.Rc == 0 && p.nc == 0 && p.maxT == 3 && !p.single_rows);
  CHECK(same(p.cnt_le, {1, 2, 5, 5, 6}) && same(p.rows_le, {2, 3, 8, 8, 9}));
  CHECK(eq(p.seqs[3], SeqDesc{6, 1, 2, 3, 0, 1}) && eq(p.seqs[4], SeqDesc{7, 1, 1, 3, 0, 1}));
  CHECK(p.egroups.size() == 1 && p.egroups[0].first == 0 && p.egroups[0].count == 3);
  CHECK(same(p.eg_beg, {0, 0, 0, 1, 1}) && same(p.eg_cnt, {0, 0, 1, 0, 0}) && same(p.egidx, {2, 3, 4}));
  CHECK(same(p.ent_other, {(char)1, (char)1, (char)0, (char)0, (char)1}));
  CHECK(same(p.last, {5, 6, 7, 2, 8, 1}) && same(p.last_sorted, {1, 2, 5, 6, 7, 8}));
  for (char u : p.use_lin) CHECK(u == 0);
  CHECK(p.lin_mbs.empty() && p.hs_items.empty());

  g_case = "exact case, fused";
  c.fused = c.lin_wanted = true;
  CHECK(plan_sweep(c.in(), p, err) == TVR_OK);
  CHECK(p.Rc == 8 && p.nc == 3 && p.R == 9);
  CHECK(same(p.row0, {3, 6, 7, 2, 8, 0}) && same(p.last, {13, 14, 15, 10, 16, 9}));
  CHECK(same(p.last_sorted, {0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 13, 14, 15, 16}) && same(p.clean_last, {2, 5, 7}));
  CHECK(eq(p.seqs[0], SeqDesc{0, 3, 0, -1, 0, 0}) && eq(p.seqs[2], SeqDesc{6, 2, 0, -1, 0, 0}));
  CHECK(eq(p.seqs[3], SeqDesc{8, 2, 0, 6, 0, 0}) && eq(p.seqs[5], SeqDesc{11, 3, 0, 0, 0, 0}));
  CHECK(eq(p.seqs[6], SeqDesc{14, 1, 2, 11, 0, 1}) && eq(p.seqs[7], SeqDesc{15, 1, 1, 11, 0, 1}));
  CHECK(p.ents[2].row0 == 11 && p.ents[0].row0 == 8 && p.ents[5].row0 == 16);
  CHECK(same(p.use_lin, {(char)0, (char)0, (char)1, (char)0}));
  CHECK(same(p.lin_vids, {0}) && same(p.lin_nv, {0, 0, 1, 0}) && p.lin_max_nv == 1);
  CHECK(same(p.lin_nrows, {0, 0, 5, 0}) && same(p.lin_nmb, {0, 0, 1, 0}) && p.lin_rows.size() == 5);
  const int out_rows[5] = {11, 12, 13, 14, 15}, clean_rows[5] = {0, 1, 2, 5, 7};
  for (int r = 0; r < 5; ++r)
    CHECK(p.lin_rows[r].out_row == out_rows[r] && p.lin_rows[r].clean_row == clean_rows[r] && p.lin_rows[r].vrow == 0);
  CHECK(p.lin_mbs.size() == 1 && p.lin_mbs[0].row0 == 0 && p.lin_mbs[0].rows == 5 && p.lin_mbs[0].head == 0);
}

// --- c) every validation error, by message ---------------------------------------------------------------------

void expect_error(const char* name, const Case& c, const std::string& msg) {
  g_case = std::string("error case: ") + name;
  SweepPlan p;
  std::string err;
  CHECK(plan_sweep(c.in(), p, err) == TVR_ERR_INVALID);
  if (err != msg) std::fprintf(stderr, "got \"%s\", want \"%s\"\n", err.c_str(), msg.c_str());
  CHECK(err == msg);
}

// the exact case's trace with the given sites; sets: every site owns the patches listed for it
Case with_sites(std::vector<tvr_site> sites, bool sets = false, std::vector<std::vector<tvr_head_patch>> own = {}) {
  Case c = exact_case();
  c.sites = sites;
  c.sets = sets;
  c.set_off.assign(1, 0);
  own.resize(sites.size());
  for (const auto& o : own) {
    c.patches.insert(c.patches.end(), o.begin(), o.end());
    c.set_off.push_back((int32_t)c.patches.size());
  }
  return c;
}

void check_errors() {
  expect_error("seq", with_sites({site(3, 0)}), "site 0: seq out of range");
  expect_error("negative seq", with_sites({site(-1, 0)}), "site 0: seq out of range");
  expect_error("set kind in the plain sweep", with_sites({site(0, 4)}),
               "site 0: head-set kinds (4, 5) go through tvr_patch_sweep_sets");
  expect_error("a plain kind owning patches", with_sites({site(0, 1, 1, 0, 0)}, true, {{{1, 0, 0}}}),
               "site 0: only head-set kinds (4, 5) own patches");
  expect_error("patch layer", with_sites({site(0, 4)}, true, {{{4, 0, 0}}}), "site 0: patch layer/head out of range");
  expect_error("patch head", with_sites({site(0, 5)}, true, {{{0, 2, 0}}}), "site 0: patch layer/head out of range");
  expect_error("patch vector", with_sites({site(0, 4)}, true, {{{0, 0, 2}}}), "site 0: patch vector out of range");
  expect_error("duplicate (layer, head)", with_sites({site(0, 4)}, true, {{{1, 1, 0}, {0, 0, 0}, {1, 1, 1}}}),
               "site 0: the same (layer, head) twice in one set");
  expect_error("layer", with_sites({site(0, 1, 4, 0, 0)}), "site 0: layer/head out of range");
  expect_error("head", with_sites({site(0, 1, 0, -1, 0)}), "site 0: layer/head out of range");
  expect_error("layer of an added vector", with_sites({site(0, 2, -1, 0, 0)}), "site 0: layer out of range");
  expect_error("vector", with_sites({site(0, 1, 0, 0, 2)}), "site 0: vector out of range");
  expect_error("vector of an added vector", with_sites({site(0, 2, 0, 0, -1)}), "site 0: vector out of range");
  expect_error("vector of a resid vector", with_sites({site(0, 6, 0, 0, 2, 0)}), "site 0: vector out of range");
  Case c = with_sites({site(0, 1, 0, 0, 0)});
  c.have_vectors = false;
  expect_error("null vectors", c, "site 0: vector out of range");
  c = with_sites({site(0, 1, 0, 0, 0)}, true);
  c.aligned = false;
  expect_error("unaligned vectors in the set sweep", c, "site 0: REPLACE_HEAD_ALLPOS needs 16-byte aligned vectors");
  c.sets = false;  // the plain sweep does not check
  g_case = "unaligned vectors in the plain sweep";
  SweepPlan p;
  std::string err;
  CHECK(plan_sweep(c.in(), p, err) == TVR_OK);
  expect_error("resid pos", with_sites({site(2, 3, 0, 0, 0, 2, 0, 0)}), "site 0: resid patch out of range");
  expect_error("resid src_seq", with_sites({site(0, 3, 0, 0, 0, 0, 3, 0)}), "site 0: resid patch out of range");
  expect_error("resid src_pos", with_sites({site(0, 3, 0, 0, 0, 0, 2, 2)}), "site 0: resid patch out of range");
  expect_error("resid layer", with_sites({site(0, 3, 4, 0, 0, 0, 0, 0)}), "site 0: resid patch out of range");
  expect_error("resid vector pos", with_sites({site(2, 6, 0, 0, 0, 2)}), "site 0: resid patch out of range");
  expect_error("resid vector layer", with_sites({site(0, 6, -1, 0, 0, 0)}), "site 0: resid patch out of range");
  expect_error("unknown kind", with_sites({site(0, 7)}), "site 0: unknown kind");
  expect_error("negative kind", with_sites({site(0, -1)}), "site 0: unknown kind");
  // the first bad site, and within it the first failing condition
  expect_error("two bad sites", with_sites({site(0, 0), site(1, 2, 9, 0, 0), site(0, 0), site(5, 0)}),
               "site 1: layer out of range");
  expect_error("two bad fields", with_sites({site(0, 1, 9, 0, 9)}), "site 0: layer/head out of range");
  // fields a kind does not read may hold anything
  g_case = "unread fields";
  tvr_site s = site(0, 0, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN);
  c = with_sites({s});
  CHECK(plan_sweep(c.in(), p, err) == TVR_OK && p.entry[0] == 4 && p.nrow[0] == 1);
}

}  // namespace

int main() {
  check_exact();
  check_errors();
  check_invariants(400);
  std::puts("sweep_plan_check: ok");
  return 0;
}
