// sweep_desc.hpp — the descriptor tables the host planner (sweep_plan.hpp) builds and the kernels read.
// Host-only: plain structs of 32-bit fields, no HIP type, so the planner compiles and runs without a GPU.
#pragma once
#include <stdint.h>

namespace tvr {

// One sequence as seen by attention at a layer: its computed rows are the
// positions [p0, p0+n); positions [0, p0) come from the clean trace's K/V.
struct SeqDesc {
  int32_t row0;       // first computed row in the activation buffers
  int32_t n;          // number of computed rows
  int32_t p0;         // absolute position of row0
  int32_t cache_row;  // row of position 0 for the K/V prefix (positions < p0), -1: none
  int32_t q0;         // first computed row that is a query (n-1: last row only)
  int32_t prefix_live;  // 0: the prefix is in the clean trace (cache); 1: in this run's qkv rows
                        // (a shared-prefix follower reads its leader's rows: tvr_patch_sweep)
};

// How a patch site's residual is materialised at its entry layer e
// (resid_pre[e] rows [p0, p0+n)), from the clean trace.
struct EntryDesc {
  int32_t kind;       // tvr_site_kind
  int32_t row0;       // destination row (activation buffer)
  int32_t n;          // rows
  int32_t p0;         // first position
  int32_t src_row;    // trace row of position 0 of `seq`
  int32_t src2_row;   // SET_RESID_PRE_POS: trace row supplying the patched position
  int32_t patch_pos;  // SET_RESID_PRE_POS / _VEC: absolute patched position
  int32_t head;       // REPLACE_HEAD
  int32_t vec;        // vector row (SET_RESID_PRE_VEC: the row written at patch_pos)
  int32_t pad;
};

// One block of entry_replace_mfma_kernel (entry_mfma.hpp): entries gidx[first .. first + count), REPLACE_HEAD
// sites of one head entering at one layer.
struct EntryGroup {
  int32_t first, count;
};
static_assert(sizeof(EntryGroup) == 8, "EntryGroup is read as two 32-bit words");

// One block's rows (lin_entry.hpp): entering rows [row0, row0 + rows) of the layer's row list
// (rows <= 64), all of head `head`.
struct LinMB {
  int row0, rows, head, pad;
};
// One entering row: its activation row, its clean row (trace row of the same
// prompt position: y_c, z_h and the clean LN statistics) and its vector's row of G.
struct LinRow {
  int out_row, clean_row, vrow, pad;
};

// headset_patch.hpp: one (site, layer) record and the flat (head, vector) list its range points into.
struct HeadsetItem {
  int32_t row0;         // first row of the site in the activation buffers
  int32_t n_rows;       // the site's rows (all positions: T, last position: 1)
  int32_t first_patch;  // range of the flat patch list: the site's heads at this layer
  int32_t n_patches;
};
struct HeadsetPatch {
  int32_t head;
  int32_t vec;  // row of `vectors`
};

// attention_knockout.hpp: one (site, layer) record.  The last query of sequence `seq` (an index into the
// launch's SeqDesc table) is recomputed for the heads of the mask with the keys of the bitmask blocked:
// key j is bit j % 32 of word masks[mask_off + j / 32], ceil(T / 32) words.
struct KnockoutItem {
  int32_t seq;
  int32_t mask_off;
  uint32_t heads_lo, heads_hi;  // head h: bit h % 32 of heads_lo (h < 32) or heads_hi
};
static_assert(sizeof(KnockoutItem) == 16, "KnockoutItem is read as four 32-bit words");

}  // namespace tvr
