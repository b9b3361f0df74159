// sweep_plan.hpp — the host planner of tvr_patch_sweep / tvr_patch_sweep_sets.
//
// From the trace's host metadata and the caller's sites it validates the sites and lays out the sweep: each
// site's entry layer and computed rows, shared-prefix leaders and followers, the rows in entry order, and the
// descriptor tables the kernels read (sweep_desc.hpp).  No HIP call, no device memory, no environment: the
// engine (engine.hip sweep_impl) passes its switches in, carves the workspace from the plan and uploads the
// tables.  Plain C++17, so tests/sweep_plan_check.cpp runs it on a CPU under the sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "sweep_desc.hpp"
#include "tvr.h"

namespace tvr {

// Length of the token prefix a sequence of T tokens shares with its leader's, capped so that the sequence's
// last row stays its own (tvr_forward_clean's and the sweep's shared prefixes).
inline int shared_prefix_len(const int32_t* tk, int T, const int32_t* tl, int T_leader) {
  const int cap = std::min(T - 1, T_leader);
  int P = 0;
  while (P < cap && tk[P] == tl[P]) ++P;
  return P;
}

struct SweepPlanIn {
  int n_layers, n_heads, d_model, d_head;
  // the trace's host metadata
  const int* seq_off;
  const int* seq_len;
  const int32_t* tokens;
  int n_seq, n_tokens;
  bool fused;         // a deferred clean forward runs inside this sweep (its rows first)
  bool prefix_share;  // TVR_PREFIX_SHARE
  bool lin_wanted;    // the linearised entry applies (fused, a planar GEMM mode, L >= 3, TVR_LIN_ENTRY)
  int entry_group;    // ENTRY_GROUP (entry_mfma.hpp)
  int n_vectors;
  bool have_vectors, vectors_aligned16;
  double hs_slice_bytes;  // bytes of one d_head element of a head's z slice, all planes (profiling)
  const tvr_site* sites;
  int n_sites;
  const int32_t* set_off;  // nullptr: the plain sweep
  const tvr_head_patch* patches;
  // tvr_patch_sweep_knockout: a site of kind TVR_SITE_ATTN_KNOCKOUT_LASTPOS owns keys[key_off[i], key_off[i + 1]),
  // the blocked key positions of its last query; nullptr: no knockout tables (kind 7 is then unknown)
  const int32_t* key_off = nullptr;
  const int32_t* keys = nullptr;
};

struct SweepPlan {
  int Rc = 0, nc = 0;  // the fused clean rows / sequences, which precede the sites' (0: not fused)
  int R = 0;           // the sites' rows
  int maxT = 0;
  // every site computes one row (its last position: ADD_ATTN_OUT_LASTPOS, NONE, a SET_RESID_PRE_POS /
  // SET_RESID_PRE_VEC of the last position): the site sequences go to the single-query attention kernel
  bool single_rows = true;
  // per site (caller's index): entry layer, first computed position, rows, first row, shared-prefix leader or -1
  std::vector<int> entry, p0, nrow, row0, leader;
  std::vector<int> order;            // the sites by entry layer (stable)
  std::vector<int> cnt_le, rows_le;  // [L + 1]: sites / rows with entry <= l
  // sequence descriptors: the fused clean sequences first, then the sites in entry order; seqs_last: the last
  // layer computes every clean row (the trace keeps them) and each site's last row
  std::vector<SeqDesc> seqs, seqs_last;
  std::vector<EntryDesc> ents;  // entry order
  std::vector<int32_t> last, tg, last_sorted, clean_last;
  // entry layers' head-replacement sites grouped by head, at most entry_group per group, groups of one head
  // balanced (entry_mfma.hpp); ent_other: the layer has sites of other kinds (entry_kernel)
  std::vector<char> ent_other;
  std::vector<int32_t> egidx;
  std::vector<EntryGroup> egroups;
  std::vector<int> eg_beg, eg_cnt;
  std::vector<double> entry_bytes;  // entry layers 0..L (L: the final norm's input), profiling
  // Head-set tables (headset_patch.hpp): per layer, one item per site with heads there (entry order) and
  // the items' (head, vector) lists, each in the caller's order.
  std::vector<HeadsetItem> hs_items;
  std::vector<HeadsetPatch> hs_patches;
  std::vector<int> hs_beg, hs_max_rows;
  std::vector<double> hs_bytes;
  // Knockout tables (attention_knockout.hpp): per layer, one item per kind-7 site with members there (entry
  // order); ko_masks: each such site's blocked keys as ceil(T / 32) words, shared by its layers.
  std::vector<KnockoutItem> ko_items;
  std::vector<uint32_t> ko_masks;
  std::vector<int> ko_beg, ko_max_keys;
  std::vector<double> ko_bytes;
  // Linearised entry layers (lin_entry.hpp), per such layer: the distinct vectors (rows of G), the entering
  // rows grouped by head, m-blocks of <= 64 rows of one head.
  std::vector<char> use_lin;
  std::vector<int32_t> lin_vids;
  std::vector<LinRow> lin_rows;
  std::vector<LinMB> lin_mbs;
  std::vector<int> lin_vid_off, lin_nv, lin_mb_off, lin_nmb, lin_nrows;
  int lin_max_nv = 0;
  // the Wsc planes do not fit: every layer takes the full-GEMM entry (as TVR_LIN_ENTRY=0)
  void drop_lin() {
    std::fill(use_lin.begin(), use_lin.end(), 0);
    lin_vids.clear();
    lin_rows.clear();
    lin_mbs.clear();
    lin_max_nv = 0;
  }
};

namespace plan_detail {

inline bool is_headset(int kind) {
  return kind == TVR_SITE_REPLACE_HEADSET_ALLPOS || kind == TVR_SITE_REPLACE_HEADSET_LASTPOS;
}
inline bool is_knockout(const SweepPlanIn& in, int kind) {
  return in.key_off && kind == TVR_SITE_ATTN_KNOCKOUT_LASTPOS;
}
inline bool vec_ok(const SweepPlanIn& in, int vec) { return in.have_vectors && vec >= 0 && vec < in.n_vectors; }

// One site's entry layer, first position and rows; "" or what is wrong with it.
inline const char* classify_site(const SweepPlanIn& in, int i, int& entry, int& p0, int& nrow) {
  const tvr_site& s = in.sites[i];
  const int L = in.n_layers, T = in.seq_len[s.seq];
  const bool is_set = is_headset(s.kind);
  if (is_set && !in.set_off) return "head-set kinds (4, 5) go through tvr_patch_sweep_sets";
  const bool is_ko = is_knockout(in, s.kind);
  if (in.set_off && !is_set && !is_ko && in.set_off[i + 1] != in.set_off[i])
    return in.key_off ? "only head-set and knockout kinds (4, 5, 7) own patches" : "only head-set kinds (4, 5) own patches";
  if (in.key_off && !is_ko && in.key_off[i + 1] != in.key_off[i]) return "only the knockout kind (7) owns keys";
  const bool layer_ok = s.layer >= 0 && s.layer < L;
  p0 = T - 1; nrow = 1;  // (the last position only; the all-position cases adjust)
  switch (s.kind) {
    case TVR_SITE_REPLACE_HEADSET_ALLPOS:
    case TVR_SITE_REPLACE_HEADSET_LASTPOS: {
      // Head-set site: enters at its lowest patched layer as an unpatched copy of the clean rows (the
      // entry kernel's row copy) and runs every layer from there, patched by headset_patch_kernel at
      // each layer where it has heads.  An empty set is TVR_SITE_NONE.
      entry = L;
      std::vector<std::pair<int, int>> lh;
      for (int q = in.set_off[i]; q < in.set_off[i + 1]; ++q) {
        const tvr_head_patch& hp = in.patches[q];
        if (hp.layer < 0 || hp.layer >= L || hp.head < 0 || hp.head >= in.n_heads) return "patch layer/head out of range";
        if (!vec_ok(in, hp.vec)) return "patch vector out of range";
        entry = std::min(entry, (int)hp.layer);
        lh.emplace_back(hp.layer, hp.head);
      }
      std::sort(lh.begin(), lh.end());
      if (std::adjacent_find(lh.begin(), lh.end()) != lh.end()) return "the same (layer, head) twice in one set";
      if (s.kind == TVR_SITE_REPLACE_HEADSET_ALLPOS && entry < L) { p0 = 0; nrow = T; }
      return "";
    }
    case TVR_SITE_ATTN_KNOCKOUT_LASTPOS: {
      // Knockout site: planned as the last-position head-set kind — it enters at its lowest member layer as a
      // copy of its clean last row and runs every layer from there; attention_knockout_kernel recomputes the
      // members' z slices at each layer where it has some.  No members or no keys: TVR_SITE_NONE.
      if (!is_ko) return "unknown kind";
      entry = L;
      std::vector<std::pair<int, int>> lh;
      for (int q = in.set_off[i]; q < in.set_off[i + 1]; ++q) {
        const tvr_head_patch& hp = in.patches[q];
        if (hp.layer < 0 || hp.layer >= L || hp.head < 0 || hp.head >= in.n_heads) return "member layer/head out of range";
        entry = std::min(entry, (int)hp.layer);
        lh.emplace_back(hp.layer, hp.head);
      }
      std::sort(lh.begin(), lh.end());
      if (std::adjacent_find(lh.begin(), lh.end()) != lh.end()) return "the same (layer, head) twice in one set";
      const int k0 = in.key_off[i], k1 = in.key_off[i + 1];
      for (int q = k0; q < k1; ++q) {
        if (in.keys[q] < 0 || in.keys[q] >= T) return "blocked key outside [0, seq_len)";
        if (q > k0 && in.keys[q] <= in.keys[q - 1]) return "blocked keys must be strictly increasing";
      }
      if (k1 - k0 >= T) return "every key is blocked: one key of the last query must remain";
      if (k1 == k0) entry = L;
      return "";
    }
    case TVR_SITE_NONE:
      entry = L;
      return "";
    case TVR_SITE_REPLACE_HEAD_ALLPOS:
      if (!layer_ok || s.head < 0 || s.head >= in.n_heads) return "layer/head out of range";
      if (!vec_ok(in, s.vec)) return "vector out of range";
      if (in.set_off && !in.vectors_aligned16)  // tvr.h: the head-replacement entry kernels load 16 bytes
        return "REPLACE_HEAD_ALLPOS needs 16-byte aligned vectors";
      entry = s.layer + 1; p0 = 0; nrow = T;
      return "";
    case TVR_SITE_ADD_ATTN_OUT_LASTPOS:
      if (!layer_ok) return "layer out of range";
      if (!vec_ok(in, s.vec)) return "vector out of range";
      entry = s.layer + 1;
      return "";
    case TVR_SITE_SET_RESID_PRE_POS:
    case TVR_SITE_SET_RESID_PRE_VEC: {  // one planning rule; _VEC's row comes from `vectors`, _POS's from the trace
      const bool src_ok = s.kind == TVR_SITE_SET_RESID_PRE_VEC ||
                          (s.src_seq >= 0 && s.src_seq < in.n_seq && s.src_pos >= 0 && s.src_pos < in.seq_len[s.src_seq]);
      if (!layer_ok || s.pos < 0 || s.pos >= T || !src_ok) return "resid patch out of range";
      if (s.kind == TVR_SITE_SET_RESID_PRE_VEC && !vec_ok(in, s.vec)) return "vector out of range";
      entry = s.layer; p0 = s.pos; nrow = T - s.pos;
      return "";
    }
    default:
      return "unknown kind";
  }
}

inline int classify(const SweepPlanIn& in, SweepPlan& p, std::string& err) {
  const int n = in.n_sites;
  p.entry.resize(n); p.p0.resize(n); p.nrow.resize(n);
  for (int s = 0; s < p.nc; ++s) p.maxT = std::max(p.maxT, in.seq_len[s]);
  for (int i = 0; i < n; ++i) {
    const char* what = in.sites[i].seq < 0 || in.sites[i].seq >= in.n_seq
                           ? "seq out of range"
                           : classify_site(in, i, p.entry[i], p.p0[i], p.nrow[i]);
    if (*what) {
      err = "site " + std::to_string(i) + ": " + what;
      return TVR_ERR_INVALID;
    }
    p.maxT = std::max(p.maxT, in.seq_len[in.sites[i].seq]);
    p.single_rows = p.single_rows && p.nrow[i] == 1;
  }
  return TVR_OK;
}

// Shared prefixes (REPLACE_HEAD_ALLPOS): sites with the same (layer, head,
// vector) whose sequences start with the same tokens compute identical rows
// over that common prefix (position j attends to positions <= j only, and
// the patch is the same at every position).  The first such site (the
// leader) computes them; a follower starts at its common-prefix length P
// and reads positions < P's K/V from the leader's rows of this run
// (SeqDesc.prefix_live).  A CIE sweep's prompts all start with BOS, so
// (n_prompts - 1) / n_prompts of the position-0 rows — 1/T of the sweep's
// rows — are not recomputed.  The reference's batch-1 forwards compute that
// row identically for every prompt (scratch2.py:181-194).
inline void share_prefixes(const SweepPlanIn& in, SweepPlan& p) {
  p.leader.assign(in.n_sites, -1);
  if (!in.prefix_share) return;
  std::map<std::tuple<int, int, int, int>, int> first;
  for (int i = 0; i < in.n_sites; ++i) {
    const tvr_site& s = in.sites[i];
    if (s.kind != TVR_SITE_REPLACE_HEAD_ALLPOS) continue;
    const int32_t* tk = in.tokens + in.seq_off[s.seq];
    const auto ins = first.emplace(std::make_tuple(s.layer, s.head, s.vec, (int)tk[0]), i);
    if (ins.second) continue;
    const int ld = ins.first->second, T = in.seq_len[s.seq], lseq = in.sites[ld].seq;
    const int P = shared_prefix_len(tk, T, in.tokens + in.seq_off[lseq], in.seq_len[lseq]);
    if (P == 0) continue;
    p.leader[i] = ld;
    p.p0[i] = P;
    p.nrow[i] = T - P;
  }
}

// The rows in entry order and everything indexed by them: SeqDesc / EntryDesc, the last rows, the targets.
inline void layout_rows(const SweepPlanIn& in, SweepPlan& p) {
  const int n = in.n_sites, L = in.n_layers, Rc = p.Rc, nc = p.nc;
  p.order.resize(n);
  for (int i = 0; i < n; ++i) p.order[i] = i;
  std::stable_sort(p.order.begin(), p.order.end(), [&](int a, int b) { return p.entry[a] < p.entry[b]; });
  p.row0.resize(n);
  for (int k = 0; k < n; ++k) {
    p.row0[p.order[k]] = p.R;
    p.R += p.nrow[p.order[k]];
  }
  p.cnt_le.assign(L + 1, 0);
  p.rows_le.assign(L + 1, 0);
  for (int l = 0, k = 0, rows = 0; l <= L; ++l) {
    while (k < n && p.entry[p.order[k]] <= l) rows += p.nrow[p.order[k++]];
    p.cnt_le[l] = k;
    p.rows_le[l] = rows;
  }
  p.seqs.resize(nc + n);
  p.clean_last.resize(nc);
  for (int s = 0; s < nc; ++s) {
    p.seqs[s] = SeqDesc{in.seq_off[s], in.seq_len[s], 0, -1, 0, 0};
    p.clean_last[s] = in.seq_off[s] + in.seq_len[s] - 1;
  }
  p.ents.resize(n);
  for (int k = 0; k < n; ++k) {
    const int i = p.order[k];
    const tvr_site& s = in.sites[i];
    const int srow = in.seq_off[s.seq];
    p.seqs[nc + k] = p.leader[i] >= 0 ? SeqDesc{Rc + p.row0[i], p.nrow[i], p.p0[i], Rc + p.row0[p.leader[i]], 0, 1}
                                      : SeqDesc{Rc + p.row0[i], p.nrow[i], p.p0[i], srow, 0, 0};
    EntryDesc e{};
    // a head-set or knockout site enters as a plain copy of its clean rows (the entry kernel's TVR_SITE_NONE path)
    e.kind = is_headset(s.kind) || is_knockout(in, s.kind) ? (int32_t)TVR_SITE_NONE : s.kind;
    e.row0 = Rc + p.row0[i];
    e.n = p.nrow[i];
    e.p0 = p.p0[i];
    e.src_row = srow;
    e.src2_row = (s.kind == TVR_SITE_SET_RESID_PRE_POS) ? in.seq_off[s.src_seq] + s.src_pos : 0;
    e.patch_pos = s.pos;
    e.head = s.head;
    e.vec = s.vec;
    p.ents[k] = e;
  }
  p.last.resize(n);
  p.tg.resize(n);
  for (int i = 0; i < n; ++i) {
    p.last[i] = Rc + p.row0[i] + p.nrow[i] - 1;
    p.tg[i] = in.sites[i].target;
  }
  p.seqs_last = p.seqs;
  p.last_sorted.resize(Rc + n);
  for (int r = 0; r < Rc; ++r) p.last_sorted[r] = r;
  for (int k = 0; k < n; ++k) {
    p.seqs_last[nc + k].q0 = p.seqs_last[nc + k].n - 1;
    p.last_sorted[Rc + k] = p.last[p.order[k]];
  }
}

inline void group_entries(const SweepPlanIn& in, SweepPlan& p) {
  const int L = in.n_layers, d = in.d_model;
  p.ent_other.assign(L + 1, 0);
  p.eg_beg.assign(L + 1, 0);
  p.eg_cnt.assign(L + 1, 0);
  p.entry_bytes.assign(L + 1, 0.0);
  for (int l = 0; l <= L; ++l) {
    p.eg_beg[l] = (int)p.egroups.size();
    std::map<int, std::vector<int>> byhead;
    for (int k = l > 0 ? p.cnt_le[l - 1] : 0; k < p.cnt_le[l]; ++k) {
      const EntryDesc& e = p.ents[k];
      // algorithmic bytes of the layer's entry launch: the clean rows read and the patched rows written, the
      // vector, and for REPLACE_HEAD the head's z rows plus its W_O slice once per distinct head
      double b = (2.0 * e.n * d + d) * 4.0;
      if (e.kind == TVR_SITE_REPLACE_HEAD_ALLPOS) {
        b += (double)e.n * in.d_head * 4.0;
        if (!byhead.count(e.head)) b += (double)d * in.d_head * 4.0;
        byhead[e.head].push_back(k);
      } else {
        p.ent_other[l] = 1;
      }
      p.entry_bytes[l] += b;
    }
    for (const auto& hv : byhead) {  // ceil(n / entry_group) groups of balanced size (the launch ends with its
      const size_t n = hv.second.size(), ng = (n + in.entry_group - 1) / in.entry_group;  // largest group)
      for (size_t gi = 0; gi < ng; ++gi) {
        const size_t a = gi * n / ng, b = (gi + 1) * n / ng;
        p.egroups.push_back(EntryGroup{(int32_t)p.egidx.size(), (int32_t)(b - a)});
        p.egidx.insert(p.egidx.end(), hv.second.begin() + a, hv.second.begin() + b);
      }
    }
    p.eg_cnt[l] = (int)p.egroups.size() - p.eg_beg[l];
  }
}

inline void build_headsets(const SweepPlanIn& in, SweepPlan& p) {
  const int L = in.n_layers, n = in.n_sites, d = in.d_model;
  p.hs_beg.assign(L + 1, 0);
  p.hs_max_rows.assign(L, 0);
  p.hs_bytes.assign(L, 0.0);
  if (!in.set_off || in.set_off[n] <= in.set_off[0]) return;
  const double slice = in.d_head * in.hs_slice_bytes;
  std::vector<std::vector<std::pair<int, int>>> by_layer(L);  // (site, patch) in (entry order, list order)
  for (int k = 0; k < n; ++k) {
    if (!is_headset(in.sites[p.order[k]].kind)) continue;  // (a knockout site's members: build_knockouts)
    for (int q = in.set_off[p.order[k]]; q < in.set_off[p.order[k] + 1]; ++q)
      by_layer[in.patches[q].layer].emplace_back(p.order[k], q);
  }
  for (int l = 0; l < L; ++l) {
    p.hs_beg[l] = (int)p.hs_items.size();
    const auto& bl = by_layer[l];
    for (size_t x = 0; x < bl.size();) {
      const int i = bl[x].first, first = (int)p.hs_patches.size();
      for (; x < bl.size() && bl[x].first == i; ++x)
        p.hs_patches.push_back(HeadsetPatch{in.patches[bl[x].second].head, in.patches[bl[x].second].vec});
      const int np = (int)p.hs_patches.size() - first;
      p.hs_items.push_back(HeadsetItem{p.Rc + p.row0[i], p.nrow[i], first, np});
      p.hs_max_rows[l] = std::max(p.hs_max_rows[l], p.nrow[i]);
      // slices zeroed + residual rows read and written + vectors read
      p.hs_bytes[l] += (double)p.nrow[i] * (8.0 * d + slice * np) + 4.0 * d * np;
    }
  }
  p.hs_beg[L] = (int)p.hs_items.size();
}

// Per layer, one item per knockout site with members there, in entry order; a site's mask words once.
inline void build_knockouts(const SweepPlanIn& in, SweepPlan& p) {
  const int L = in.n_layers, n = in.n_sites;
  p.ko_beg.assign(L + 1, 0);
  p.ko_max_keys.assign(L, 0);
  p.ko_bytes.assign(L, 0.0);
  if (!in.key_off || !in.set_off) return;
  std::vector<std::vector<KnockoutItem>> by_layer(L);
  std::vector<std::vector<int>> keys_of(L);  // the items' sequence lengths
  for (int k = 0; k < n; ++k) {
    const int i = p.order[k];
    if (!is_knockout(in, in.sites[i].kind) || p.entry[i] >= L) continue;  // (no members or no keys: entry == L)
    const int T = in.seq_len[in.sites[i].seq], mask_off = (int)p.ko_masks.size();
    p.ko_masks.resize(mask_off + (T + 31) / 32, 0u);
    for (int q = in.key_off[i]; q < in.key_off[i + 1]; ++q)
      p.ko_masks[mask_off + in.keys[q] / 32] |= 1u << (in.keys[q] % 32);
    std::map<int, uint64_t> heads;  // layer -> head mask
    for (int q = in.set_off[i]; q < in.set_off[i + 1]; ++q) heads[in.patches[q].layer] |= 1ull << in.patches[q].head;
    for (const auto& lh : heads) {
      by_layer[lh.first].push_back(KnockoutItem{p.nc + k, mask_off, (uint32_t)lh.second, (uint32_t)(lh.second >> 32)});
      keys_of[lh.first].push_back(T);
    }
  }
  for (int l = 0; l < L; ++l) {
    p.ko_beg[l] = (int)p.ko_items.size();
    for (size_t x = 0; x < by_layer[l].size(); ++x) {
      const KnockoutItem& it = by_layer[l][x];
      const int T = keys_of[l][x], nh = __builtin_popcountll(((uint64_t)it.heads_hi << 32) | it.heads_lo);
      p.ko_items.push_back(it);
      p.ko_max_keys[l] = std::max(p.ko_max_keys[l], T);
      // per listed head the Q slice, the K and V slices of every key, the z slice written; the mask words
      p.ko_bytes[l] += (double)nh * in.d_head * (4.0 * (1 + 2 * T) + in.hs_slice_bytes) + 4.0 * ((T + 31) / 32);
    }
  }
  p.ko_beg[L] = (int)p.ko_items.size();
}

// Layer l in [1, L-2] of a fused sweep whose entering sites are all REPLACE_HEAD computes its entering rows'
// QKV + MLP-in outputs from the clean rows' (this sweep's rows [0, Rc)) and a K = d_head GEMM.
inline void build_lin(const SweepPlanIn& in, SweepPlan& p) {
  const int L = in.n_layers;
  p.use_lin.assign(L, 0);
  for (auto* v : {&p.lin_vid_off, &p.lin_nv, &p.lin_mb_off, &p.lin_nmb, &p.lin_nrows}) v->assign(L, 0);
  if (!in.lin_wanted) return;
  for (int l = 1; l <= L - 2; ++l) {
    const int k0 = p.cnt_le[l - 1], k1 = p.cnt_le[l];
    bool ok = k1 > k0;
    for (int k = k0; k < k1 && ok; ++k) ok = in.sites[p.order[k]].kind == TVR_SITE_REPLACE_HEAD_ALLPOS;
    if (!ok) continue;
    p.use_lin[l] = 1;
    std::map<int, int> vrow;
    p.lin_vid_off[l] = (int)p.lin_vids.size();
    for (int k = k0; k < k1; ++k) {
      const int vec = in.sites[p.order[k]].vec;
      if (vrow.emplace(vec, (int)vrow.size()).second) p.lin_vids.push_back(vec);
    }
    p.lin_nv[l] = (int)vrow.size();
    p.lin_max_nv = std::max(p.lin_max_nv, p.lin_nv[l]);
    p.lin_mb_off[l] = (int)p.lin_mbs.size();
    const int r_first = (int)p.lin_rows.size();
    for (int h = 0; h < in.n_heads; ++h) {
      const int g0 = (int)p.lin_rows.size();
      for (int k = k0; k < k1; ++k) {
        const int i = p.order[k];
        const tvr_site& s = in.sites[i];
        if (s.head != h) continue;
        for (int q = 0; q < p.nrow[i]; ++q)
          p.lin_rows.push_back(LinRow{p.Rc + p.row0[i] + q, in.seq_off[s.seq] + p.p0[i] + q, vrow[s.vec], 0});
      }
      for (int r = g0; r < (int)p.lin_rows.size(); r += 64)
        p.lin_mbs.push_back(LinMB{r, std::min(64, (int)p.lin_rows.size() - r), h, 0});
    }
    p.lin_nmb[l] = (int)p.lin_mbs.size() - p.lin_mb_off[l];
    p.lin_nrows[l] = (int)p.lin_rows.size() - r_first;
  }
}

}  // namespace plan_detail

// TVR_OK and the plan, or TVR_ERR_INVALID and what is wrong with the first bad site.
inline int plan_sweep(const SweepPlanIn& in, SweepPlan& p, std::string& err) {
  p = SweepPlan{};
  p.Rc = in.fused ? in.n_tokens : 0;
  p.nc = in.fused ? in.n_seq : 0;
  const int rc = plan_detail::classify(in, p, err);
  if (rc != TVR_OK) return rc;
  plan_detail::share_prefixes(in, p);
  plan_detail::layout_rows(in, p);
  plan_detail::group_entries(in, p);
  plan_detail::build_headsets(in, p);
  plan_detail::build_knockouts(in, p);
  plan_detail::build_lin(in, p);
  return TVR_OK;
}

}  // namespace tvr
