// knockout_plan_check.cpp — the planner (csrc/sweep_plan.hpp) with knockout tables, stand-alone on the host.
//
// Over a few hundred random sweeps that mix TVR_SITE_ATTN_KNOCKOUT_LASTPOS sites with every older kind:
//   * a knockout site's entry layer (lowest member layer; L without members or without keys), its one row
//     at p0 = T - 1, and its entry as a plain copy of its clean row;
//   * the per-layer item tables against a direct restatement: one item per site with members at the layer,
//     in entry order, its sequence index, its head mask, and the mask words of its blocked keys;
//   * empty member lists / key lists produce no items;
//   * the old kinds of a mixed plan are planned as in the plan without the kind-7 sites (and the head-set
//     tables hold no knockout member);
//   * every validation message.
// Built with -fsanitize=address,undefined by tests/test_knockout_plan.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "sweep_plan.hpp"

using namespace tvr;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::printf("knockout_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

struct Sweep {
  int L, H, d_head;
  std::vector<int> seq_off, seq_len;
  std::vector<int32_t> tokens;
  std::vector<tvr_site> sites;
  std::vector<int32_t> set_off{0}, key_off{0}, keys;
  std::vector<tvr_head_patch> patches;
  bool fused;
  int n_vectors = 8;

  SweepPlanIn in(bool with_keys = true) const {
    SweepPlanIn x{L, H, H * d_head, d_head, seq_off.data(), seq_len.data(), tokens.data(), (int)seq_len.size(),
                  (int)tokens.size(), fused, true, false, 16, n_vectors, true, true, 4.0, sites.data(),
                  (int)sites.size(), set_off.data(), patches.data()};
    if (with_keys) {
      x.key_off = key_off.data();
      x.keys = keys.data();
    }
    return x;
  }
  void close_site() {
    set_off.push_back((int32_t)patches.size());
    key_off.push_back((int32_t)keys.size());
  }
};

static Sweep random_sweep(std::mt19937& rng, bool only_old = false) {
  auto ri = [&](int a, int b) { return (int)(a + rng() % (unsigned)(b - a + 1)); };
  Sweep s;
  s.L = ri(1, 6);
  s.H = ri(1, 64);
  s.d_head = 16;
  s.fused = ri(0, 1);
  const int n_seq = ri(1, 5);
  for (int q = 0; q < n_seq; ++q) {
    const int T = ri(1, 70);
    s.seq_off.push_back((int)s.tokens.size());
    s.seq_len.push_back(T);
    for (int j = 0; j < T; ++j) s.tokens.push_back(j == 0 ? 0 : ri(1, 5));
  }
  const int n_sites = ri(1, 24);
  for (int i = 0; i < n_sites; ++i) {
    tvr_site t{};
    t.seq = ri(0, n_seq - 1);
    t.target = ri(0, 9);
    const int T = s.seq_len[t.seq];
    const int kind = only_old ? ri(0, 6) : (ri(0, 2) ? 7 : ri(0, 6));
    t.kind = kind;
    t.layer = ri(0, s.L - 1);
    t.head = ri(0, s.H - 1);
    t.vec = ri(0, s.n_vectors - 1);
    t.pos = ri(0, T - 1);
    t.src_seq = ri(0, n_seq - 1);
    t.src_pos = ri(0, s.seq_len[t.src_seq] - 1);
    if (kind == 4 || kind == 5 || kind == 7) {
      std::vector<char> used((size_t)s.L * s.H, 0);
      const int nm = ri(0, 3) ? ri(1, std::min(12, s.L * s.H)) : 0;
      for (int q = 0; q < nm; ++q) {
        const int l = ri(0, s.L - 1), h = ri(0, s.H - 1);
        if (used[(size_t)l * s.H + h]) continue;
        used[(size_t)l * s.H + h] = 1;
        s.patches.push_back(tvr_head_patch{l, h, kind == 7 ? -1 : ri(0, s.n_vectors - 1)});
      }
    }
    if (kind == 7 && T > 1 && ri(0, 3)) {
      const int keep = ri(0, T - 1);  // one key always remains
      for (int j = 0; j < T; ++j)
        if (j != keep && ri(0, 2) == 0) s.keys.push_back(j);
    }
    s.sites.push_back(t);
    s.close_site();
  }
  return s;
}

static void check_sweep(const Sweep& s) {
  const SweepPlanIn in = s.in();
  SweepPlan p;
  std::string err;
  CHECK(plan_sweep(in, p, err) == TVR_OK);
  const int n = (int)s.sites.size(), L = s.L;
  CHECK((int)p.ko_beg.size() == L + 1 && (int)p.ko_bytes.size() == L && (int)p.ko_max_keys.size() == L);
  // entry layers, rows, the entry record
  std::vector<int> pos_in_order(n);
  for (int k = 0; k < n; ++k) pos_in_order[p.order[k]] = k;
  for (int i = 0; i < n; ++i) {
    if (s.sites[i].kind != 7) continue;
    const int T = s.seq_len[s.sites[i].seq];
    int entry = L;
    for (int q = s.set_off[i]; q < s.set_off[i + 1]; ++q) entry = std::min(entry, (int)s.patches[q].layer);
    if (s.key_off[i + 1] == s.key_off[i]) entry = L;
    CHECK(p.entry[i] == entry && p.p0[i] == T - 1 && p.nrow[i] == 1 && p.leader[i] == -1);
    const EntryDesc& e = p.ents[pos_in_order[i]];
    CHECK(e.kind == TVR_SITE_NONE && e.n == 1 && e.p0 == T - 1 && e.row0 == p.Rc + p.row0[i]);
    CHECK(e.src_row == s.seq_off[s.sites[i].seq]);
    const SeqDesc& sd = p.seqs[p.nc + pos_in_order[i]];
    CHECK(sd.row0 == p.Rc + p.row0[i] && sd.n == 1 && sd.p0 == T - 1 && sd.prefix_live == 0);
    CHECK(sd.cache_row == s.seq_off[s.sites[i].seq]);
  }
  // single_rows: every site one row
  bool single = true;
  for (int i = 0; i < n; ++i) single = single && p.nrow[i] == 1;
  CHECK(p.single_rows == single);
  // the item tables, restated directly
  size_t at = 0;
  for (int l = 0; l < L; ++l) {
    CHECK(p.ko_beg[l] == (int)at);
    int max_keys = 0;
    for (int k = 0; k < n; ++k) {
      const int i = p.order[k];
      if (s.sites[i].kind != 7 || s.key_off[i + 1] == s.key_off[i]) continue;
      uint64_t heads = 0;
      for (int q = s.set_off[i]; q < s.set_off[i + 1]; ++q)
        if (s.patches[q].layer == l) heads |= 1ull << s.patches[q].head;
      if (!heads) continue;
      CHECK(at < p.ko_items.size());
      const KnockoutItem& it = p.ko_items[at++];
      const int T = s.seq_len[s.sites[i].seq];
      CHECK(it.seq == p.nc + k && (((uint64_t)it.heads_hi << 32) | it.heads_lo) == heads);
      CHECK(p.entry[i] <= l);
      CHECK(it.mask_off >= 0 && (size_t)it.mask_off + (T + 31) / 32 <= p.ko_masks.size());
      std::vector<char> blocked(T, 0);
      for (int q = s.key_off[i]; q < s.key_off[i + 1]; ++q) blocked[s.keys[q]] = 1;
      for (int j = 0; j < 32 * ((T + 31) / 32); ++j)
        CHECK(((p.ko_masks[it.mask_off + j / 32] >> (j % 32)) & 1u) == (j < T && blocked[j] ? 1u : 0u));
      max_keys = std::max(max_keys, T);
    }
    CHECK(p.ko_max_keys[l] == max_keys);
    CHECK((p.ko_bytes[l] > 0) == (p.ko_beg[l] < (int)at));
  }
  CHECK(at == p.ko_items.size() && p.ko_beg[L] == (int)at);
  // the head-set tables hold the head-set sites' members only
  size_t hs_patches = 0;
  for (int i = 0; i < n; ++i)
    if (s.sites[i].kind == 4 || s.sites[i].kind == 5) hs_patches += s.set_off[i + 1] - s.set_off[i];
  CHECK(p.hs_patches.size() == hs_patches);

  // the old kinds are planned as without the kind-7 sites (prefix sharing included): the same entry, rows and
  // leaders relative to each other, and the same tables of theirs
  Sweep o = s;
  o.sites.clear();
  o.patches.clear();
  o.keys.clear();
  o.set_off.assign(1, 0);
  o.key_off.assign(1, 0);
  std::vector<int> old_of;
  for (int i = 0; i < n; ++i) {
    if (s.sites[i].kind == 7) continue;
    old_of.push_back(i);
    o.sites.push_back(s.sites[i]);
    for (int q = s.set_off[i]; q < s.set_off[i + 1]; ++q) o.patches.push_back(s.patches[q]);
    o.close_site();
  }
  if (old_of.empty()) return;
  SweepPlan po, pn;
  CHECK(plan_sweep(o.in(), po, err) == TVR_OK);
  CHECK(plan_sweep(o.in(false), pn, err) == TVR_OK);  // and without knockout tables at all
  for (size_t x = 0; x < old_of.size(); ++x) {
    const int i = old_of[x];
    CHECK(po.entry[x] == p.entry[i] && po.p0[x] == p.p0[i] && po.nrow[x] == p.nrow[i]);
    CHECK((po.leader[x] < 0) == (p.leader[i] < 0) && (po.leader[x] < 0 || old_of[po.leader[x]] == p.leader[i]));
    CHECK(pn.entry[x] == po.entry[x] && pn.row0[x] == po.row0[x] && pn.leader[x] == po.leader[x]);
  }
  CHECK(po.ko_items.empty() && po.ko_masks.empty() && pn.ko_items.empty());
  CHECK(po.hs_items.size() == p.hs_items.size() && po.hs_patches.size() == p.hs_patches.size());
  for (size_t x = 0; x < po.hs_patches.size(); ++x)
    CHECK(po.hs_patches[x].head == p.hs_patches[x].head && po.hs_patches[x].vec == p.hs_patches[x].vec);
  CHECK(po.egroups.size() == p.egroups.size() && po.lin_rows.size() == p.lin_rows.size());
  CHECK(pn.R == po.R && pn.seqs.size() == po.seqs.size() && pn.hs_items.size() == po.hs_items.size());
}

static void expect_invalid(const Sweep& s, const char* what, bool with_keys = true) {
  SweepPlan p;
  std::string err;
  const int rc = plan_sweep(s.in(with_keys), p, err);
  if (rc != TVR_ERR_INVALID || err.find(what) == std::string::npos) {
    std::printf("knockout_plan_check: expected \"%s\", got %d \"%s\"\n", what, rc, err.c_str());
    std::exit(1);
  }
}

static void check_messages() {
  Sweep b;
  b.L = 3; b.H = 4; b.d_head = 16; b.fused = false;
  b.seq_off = {0, 5};
  b.seq_len = {5, 1};
  b.tokens = {0, 1, 2, 3, 4, 0};
  auto one = [&](int kind, int seq, std::vector<tvr_head_patch> mem, std::vector<int32_t> keys) {
    Sweep s = b;
    tvr_site t{};
    t.seq = seq;
    t.kind = kind;
    s.sites.push_back(t);
    s.patches = mem;
    s.keys = keys;
    s.close_site();
    return s;
  };
  const tvr_head_patch m10{1, 0, -1};
  {  // valid: vec is ignored
    SweepPlan p;
    std::string err;
    CHECK(plan_sweep(one(7, 0, {m10}, {0, 4}).in(), p, err) == TVR_OK);
    CHECK(p.entry[0] == 1 && p.ko_items.size() == 1 && p.ko_masks.size() == 1 && p.ko_masks[0] == 0x11u);
    CHECK(plan_sweep(one(7, 0, {m10}, {}).in(), p, err) == TVR_OK);  // no keys: TVR_SITE_NONE
    CHECK(p.entry[0] == 3 && p.ko_items.empty());
    CHECK(plan_sweep(one(7, 0, {}, {1}).in(), p, err) == TVR_OK);  // no members
    CHECK(p.entry[0] == 3 && p.ko_items.empty());
  }
  // without knockout tables kind 7 is refused as before them
  expect_invalid(one(7, 0, {m10}, {0}), "site 0: only head-set kinds (4, 5) own patches", false);
  expect_invalid(one(7, 0, {}, {}), "site 0: unknown kind", false);
  expect_invalid(one(7, 2, {m10}, {0}), "site 0: seq out of range");
  expect_invalid(one(7, 0, {{3, 0, -1}}, {0}), "member layer/head out of range");
  expect_invalid(one(7, 0, {{-1, 0, -1}}, {0}), "member layer/head out of range");
  expect_invalid(one(7, 0, {{0, 4, -1}}, {0}), "member layer/head out of range");
  expect_invalid(one(7, 0, {m10, {0, 1, -1}, m10}, {0}), "the same (layer, head) twice in one set");
  expect_invalid(one(7, 0, {m10}, {5}), "blocked key outside [0, seq_len)");
  expect_invalid(one(7, 0, {m10}, {-1}), "blocked key outside [0, seq_len)");
  expect_invalid(one(7, 0, {m10}, {2, 2}), "blocked keys must be strictly increasing");
  expect_invalid(one(7, 0, {m10}, {3, 1}), "blocked keys must be strictly increasing");
  expect_invalid(one(7, 0, {m10}, {0, 1, 2, 3, 4}), "every key is blocked");
  expect_invalid(one(7, 1, {m10}, {0}), "every key is blocked");
  expect_invalid(one(7, 1, {}, {0}), "every key is blocked");  // (without members too: the call is wrong)
  expect_invalid(one(0, 0, {}, {1}), "only the knockout kind (7) owns keys");
  expect_invalid(one(5, 0, {{1, 0, 0}}, {1}), "only the knockout kind (7) owns keys");
  expect_invalid(one(2, 0, {m10}, {}), "only head-set and knockout kinds (4, 5, 7) own patches");
  expect_invalid(one(2, 0, {m10}, {}), "only head-set kinds (4, 5) own patches", false);
  expect_invalid(one(5, 0, {{1, 0, 9}}, {}), "patch vector out of range");
  expect_invalid(one(8, 0, {}, {}), "site 0: unknown kind");
}

int main() {
  check_messages();
  std::mt19937 rng(7);
  int with_items = 0;
  for (int it = 0; it < 400; ++it) {
    const Sweep s = random_sweep(rng, it % 8 == 7);
    check_sweep(s);
    SweepPlan p;
    std::string err;
    plan_sweep(s.in(), p, err);
    with_items += !p.ko_items.empty();
  }
  CHECK(with_items > 200);
  std::printf("knockout_plan_check: ok (%d of 400 sweeps with items)\n", with_items);
  return 0;
}
