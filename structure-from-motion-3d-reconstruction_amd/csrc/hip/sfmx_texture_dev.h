// sfmx_texture_dev.h — the texture object of texture.hip as the stages that build on its last run see it
// (level.hip): the layout, the views as they were uploaded, the images and the per-face arrays on the device.
#pragma once
#include <vector>

#include "sfmx_internal.h"
#include "sfmx_raster_dev.h"

struct TxLayout {
  int S, C, cells, n_tex, fill_cell, W, H, fill;  // fill_cell: its index, or -1 without one
};

struct sfmx_texture {
  std::vector<sfmx_fusion_view> views;
  std::vector<long long> img_off;  // of a view's image in the image slab, -1 without one
  std::vector<RsSlot> slots;       // of the last run, as uploaded
  long long img_used = 0;
  int forced_batch = 0, last_batch = 0;
  DevBuf img, d_slots;
  DevBuf keys, pv, fl, big, rcounters;      // one batch's z-buffers
  DevBuf work;                              // masks, flags, ranks, the list, the scan's partials
  DevBuf res;                               // the words
  DevBuf in_v, in_f;                        // host inputs, staged
  DevBuf fview, farea, uvh, vfaces, atlas;  // the result
  bool done = false;
  int n = 0, m = 0, nviews = 0;
  int32_t counts[6] = {};
  TxLayout lay{};    // of the last successful run
  StageTimer t, tb;  // the whole run, k_tx_bake alone
};

// rank -> face of the last successful run: int32 [n_tex] behind the masks, the flags and the ranks in `work`
static inline const int* tx_face_list(const sfmx_texture* tx) {
  return reinterpret_cast<const int*>(tx->work.as<unsigned long long>() + (size_t)tx->n) + 2 * (size_t)tx->m;
}
