// index_lists.hip -- the scan layouts derived from the add-order storage: inverted lists, IVF-PQ tiles,
// IVF-Flat postings, the window-ordered tiles, the one precursor-ordered list of the window-exact index, the
// (id, window value) pairs of the scans' post-filter.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "index.hpp"

namespace asl {

// What the two builders of build_postings share: the position order (device), the per-cell counts (host) and the
// fill's zeroed cursors (device, [ncell]). A builder that fits sets inv_layout; the caller sets has_inv.
struct PostingsInput {
  const int32_t *order, *pos_blk;     // the add-order row and the block of every position
  const uint16_t *pos_loc;            // ... and its local index
  int64_t n;
  size_t nblk, ncell;                 // blocks (at least 1), blocks * d
  const std::vector<uint32_t> &h_cnt; // postings per (block, dimension)
  uint32_t *cursor;
};

// Layout 2 (flat_postings.hpp): whole lines of posting words behind a byte table; the lines must fit 32 bits.
static int build_fx_postings(asl_index *ix, const PostingsInput &in) {
  const size_t d = (size_t)ix->d, stride = (d + 127) & ~(size_t)127;
  std::vector<uint8_t> h_tab8(in.nblk * stride, 0);
  std::vector<uint16_t> h_c16(in.ncell);
  std::vector<uint32_t> h_line(in.ncell), h_base(in.nblk);
  uint64_t run = 0;     // 128-byte lines
  for (size_t b = 0; b < in.nblk; b++) {
    h_base[b] = (uint32_t)run;
    run += fx_place_block(in.h_cnt.data() + b * d, ix->d, (uint32_t)run, h_tab8.data() + b * stride,
                          h_c16.data() + b * d, h_line.data() + b * d);
  }
  if (run >= (1ull << 32)) return ASL_OK;
  const size_t bytes = (size_t)std::max<uint64_t>(run, 1) * 128 + 512;
  DevBuf<uint32_t> line_dev;
  ASL_TRY(line_dev.upload(h_line.data(), in.ncell));
  ASL_TRY(ix->blk_base.upload(h_base.data(), in.nblk));
  ASL_TRY(ix->inv_tab8.upload(h_tab8.data(), h_tab8.size()));
  ASL_TRY(ix->inv_cnt16.upload(h_c16.data(), in.ncell));
  ASL_TRY(ix->inv_data.reserve(bytes));
  HIP_TRY(hipMemsetAsync(ix->inv_data.p, 0, bytes, stream()));
  ASL_TRY(fx_fill(ix->vecs.p, ix->d, in.order, in.pos_blk, in.pos_loc, in.n, (int64_t)in.ncell, line_dev.p, in.cursor,
                  reinterpret_cast<uint32_t *>(ix->inv_data.p)));
  ASL_TRY(sync_stream());      // (line_dev and the host tables are freed on return)
  ix->tab_stride = (int)stride;
  ix->inv_layout = 2;
  return ASL_OK;
}

// Layout 1: float postings, segments placed block by block; starts and counts must fit 16 bits, the units 32.
static int build_float_postings(asl_index *ix, const PostingsInput &in) {
  const size_t d = (size_t)ix->d;
  std::vector<uint32_t> h_tab(in.ncell), h_base(in.nblk);
  uint64_t run = 0;     // 64-byte units
  bool ok = true;
  for (size_t b = 0; b < in.nblk && ok; b++) {
    h_base[b] = (uint32_t)run;
    run += inv_place_block(in.h_cnt.data() + b * d, ix->d, h_tab.data() + b * d, &ok);
    run += run & 1ull;      // every block starts on a 128-byte line
  }
  if (!ok || run >= (1ull << 32)) return ASL_OK;     // 32-bit unit offsets (256 GB of postings)
  // (+ 512: the scan reads a full wave-width from the start of an empty segment)
  const size_t bytes = (size_t)std::max<uint64_t>(run, 2) * 64 + 512;
  ASL_TRY(ix->blk_base.upload(h_base.data(), in.nblk));
  ASL_TRY(ix->inv_tab.upload(h_tab.data(), in.ncell));
  ASL_TRY(ix->inv_data.reserve(bytes));
  HIP_TRY(hipMemsetAsync(ix->inv_data.p, 0, bytes, stream()));
  ASL_TRY(inv_fill(ix->vecs.p, ix->d, in.order, in.pos_blk, in.pos_loc, in.n, (int64_t)in.nblk, ix->blk_base.p,
                   ix->inv_tab.p, in.cursor, ix->inv_data.p));
  ASL_TRY(sync_stream());      // (the host tables are freed on return)
  ix->inv_layout = 1;
  return ASL_OK;
}

// The per-dimension postings (flat_postings.hpp) of ix->vecs in a position order, for the IVF-Flat lists and the
// one list of the window-exact index (index.hpp says what the arguments are). Count, decide, build: fixed-point
// words when every non-zero is on the 2^-22 grid inside (0, 1) and a table row fits one load per lane (the
// window-exact index: only in fixed-point storage mode), else -- or when those do not fit -- float postings.
int build_postings(asl_index *ix, const int32_t *order_dev, int64_t n, const std::vector<int32_t> &blk_off,
                   const std::vector<int32_t> &pos_blk, const std::vector<uint16_t> &pos_loc) {
  DevBuf<int32_t> nnz, nnz_max;
  ASL_TRY(nnz.reserve((size_t)n));
  ASL_TRY(nnz_max.reserve(2));
  ASL_TRY(count_nnz(ix->vecs.p, ix->d, n, nnz.p, nnz_max.p));
  int32_t h_nm[2] = {0, 0};     // the most non-zeros of a vector; 1 when a non-zero is off the grid
  ASL_TRY(nnz_max.download(h_nm, 2));
  ASL_TRY(sync_stream());
  ix->nnz_max = h_nm[0];
  if (!(h_nm[0] > 0 && (size_t)h_nm[0] * 8 < (size_t)ix->d)) return ASL_OK;     // too dense: the postings do not pay
  const size_t nblk = (size_t)std::max<int32_t>(blk_off.back(), 1), ncell = nblk * (size_t)ix->d;
  ix->n_blocks = blk_off.back();
  DevBuf<int32_t> pos_blk_dev;
  DevBuf<uint16_t> pos_loc_dev;
  DevBuf<uint32_t> cnt_dev;
  ASL_TRY(pos_blk_dev.upload(pos_blk.data(), (size_t)n));
  ASL_TRY(pos_loc_dev.upload(pos_loc.data(), (size_t)n));
  ASL_TRY(cnt_dev.reserve(ncell));
  HIP_TRY(hipMemsetAsync(cnt_dev.p, 0, ncell * 4, stream()));
  ASL_TRY(inv_count(ix->vecs.p, ix->d, order_dev, pos_blk_dev.p, n, cnt_dev.p));
  std::vector<uint32_t> h_cnt(ncell);
  ASL_TRY(cnt_dev.download(h_cnt.data(), ncell));
  ASL_TRY(sync_stream());
  HIP_TRY(hipMemsetAsync(cnt_dev.p, 0, ncell * 4, stream()));      // the counts become the fill's cursors
  ix->inv_layout = 0;
  const PostingsInput in{order_dev, pos_blk_dev.p, pos_loc_dev.p, n, nblk, ncell, h_cnt, cnt_dev.p};
  const bool fixed_point = h_nm[1] == 0 && ix->d <= FX_MAX_D &&
                           (ix->kind != ASL_INDEX_WINFLAT || ix->flat_storage == ASL_FLAT_FX22);
  if (fixed_point) ASL_TRY(build_fx_postings(ix, in));
  if (!ix->inv_layout) ASL_TRY(build_float_postings(ix, in));
  if (!ix->inv_layout) return ASL_OK;      // neither fits its offsets: no postings
  ASL_TRY(ix->blk_offsets.upload(blk_off.data(), blk_off.size()));
  ASL_TRY(sync_stream());
  ix->has_inv = true;
  return ASL_OK;
}

// list-ordered copy of the PQ codes (the scan layout) from the add-order master
int build_lists(asl_index *ix) {
  if (!ix->lists_dirty) return ASL_OK;
  if (ix->kind == ASL_INDEX_WINFLAT) return winflat_layout(ix, false, nullptr, 0, 0);   // (no key: id order)
  ix->agreed_val = -1;
  ix->idpay_ready = false;
  ix->win_ready = false;
  ix->mm_ready = false;
  ix->win_serial = 0;
  ix->sel_ready = ix->wsel_ready = false;
  ix->has_selector = false;       // (one byte per vector of the lists as they were)
  const int64_t n = ix->n_store;
  std::vector<int32_t> h_vlist((size_t)n), h_order((size_t)n), h_ids;
  ix->h_list_offsets.assign((size_t)ix->nlist + 1, 0);
  if (n) {
    ASL_TRY(ix->vlist.download(h_vlist.data(), (size_t)n));
    ASL_TRY(sync_stream());
  }
  auto &off = ix->h_list_offsets;
  for (int64_t i = 0; i < n; i++) off[(size_t)h_vlist[(size_t)i] + 1]++;
  for (int l = 0; l < ix->nlist; l++) off[(size_t)l + 1] += off[(size_t)l];
  {
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; i++) h_order[(size_t)cur[(size_t)h_vlist[(size_t)i]]++] = (int32_t)i;
  }
  ASL_TRY(ix->list_offsets.upload(off.data(), off.size()));
  DevBuf<int32_t> order;
  ASL_TRY(order.upload(h_order.data(), (size_t)n));
  if (ix->kind == ASL_INDEX_IVFPQ) {
    ASL_TRY(ix->codes.reserve((size_t)std::max<int64_t>(n, 1) * ix->pq_m));
    ASL_TRY(gather_rows_u8(ix->codes_add.p, order.p, n, ix->pq_m, ix->codes.p));
  }
  if (ix->has_vids) {
    h_ids.resize((size_t)n);
    std::vector<int32_t> h_vids((size_t)n);
    if (n) {
      ASL_TRY(ix->vids.download(h_vids.data(), (size_t)n));
      ASL_TRY(sync_stream());
    }
    for (int64_t i = 0; i < n; i++) h_ids[(size_t)i] = h_vids[(size_t)h_order[(size_t)i]];
    ASL_TRY(ix->ids.upload(h_ids.data(), (size_t)n));
  } else {
    ASL_TRY(ix->ids.upload(h_order.data(), (size_t)n));
  }
  ix->has_tiles = false;
  if (tiled_index(ix)) {
    std::vector<int32_t> tile_off((size_t)ix->nlist + 1, 0), dst_slot((size_t)n);
    for (int l = 0; l < ix->nlist; l++)
      tile_off[(size_t)l + 1] = tile_off[(size_t)l] + (off[(size_t)l + 1] - off[(size_t)l] + 63) / 64;
    for (int l = 0; l < ix->nlist; l++)
      for (int32_t i = off[(size_t)l]; i < off[(size_t)l + 1]; i++)
        dst_slot[(size_t)i] = tile_off[(size_t)l] * 64 + (i - off[(size_t)l]);
    const int64_t ntiles = std::max<int64_t>(tile_off[(size_t)ix->nlist], 1);
    DevBuf<int32_t> slot_dev;
    ASL_TRY(slot_dev.upload(dst_slot.data(), (size_t)n));
    ASL_TRY(ix->tile_offsets.upload(tile_off.data(), tile_off.size()));
    ASL_TRY(ix->codes_tiled.reserve((size_t)ntiles * 2048));
    ASL_TRY(ix->ids_tiled.reserve((size_t)ntiles * 64));
    ix->n_tile_slots = ntiles * 64;
    ASL_TRY(tile_codes(ix->codes.p, ix->ids.p, slot_dev.p, n, ntiles, ix->codes_tiled.p, ix->ids_tiled.p));
    ASL_TRY(sync_stream());
    ix->has_tiles = true;
  }
  ix->has_inv = false;
  if (ix->kind == ASL_INDEX_IVFFLAT && n > 0 && ix->d <= 65535) {
    std::vector<int32_t> blk_off((size_t)ix->nlist + 1, 0), pos_blk((size_t)n);
    std::vector<uint16_t> pos_loc((size_t)n);
    for (int l = 0; l < ix->nlist; l++)
      blk_off[(size_t)l + 1] =
          blk_off[(size_t)l] + (off[(size_t)l + 1] - off[(size_t)l] + FI_BLK - 1) / FI_BLK;
    for (int l = 0; l < ix->nlist; l++)
      for (int32_t i = off[(size_t)l]; i < off[(size_t)l + 1]; i++) {
        const int32_t r = i - off[(size_t)l];
        pos_blk[(size_t)i] = blk_off[(size_t)l] + r / FI_BLK;
        pos_loc[(size_t)i] = (uint16_t)(r % FI_BLK);
      }
    ASL_TRY(build_postings(ix, order.p, n, blk_off, pos_blk, pos_loc));
  }
  ASL_TRY(sync_stream());
  ix->lists_dirty = false;
  return ASL_OK;
}

// The derived layout of the window-exact index (ASL_INDEX_WINFLAT): all vectors as ONE list, in id
// order (not keyed: what asl_index_search needs) or ordered by (key ascending, NaN last, id ascending) --
// the order window_install uses inside a list -- cut into blocks of FI_BLK consecutive positions with the
// postings of build_postings, plus the id and the key per position. key: [n_store], host or device.
int winflat_layout(asl_index *ix, bool keyed, const float *key, uint64_t serial, uint64_t gen) {
  const int64_t n = ix->n_store;
  ix->win_ready = false;
  ix->win_serial = ix->win_gen = 0;
  ix->has_inv = false;
  ix->inv_layout = 0;
  ix->n_blocks = 0;
  std::vector<int32_t> h_order((size_t)n);
  std::iota(h_order.begin(), h_order.end(), 0);
  if (keyed && n) {
    std::vector<float> h_key((size_t)n), h_wkey((size_t)n);
    HIP_TRY(hipMemcpy(h_key.data(), key, (size_t)n * 4, hipMemcpyDefault));
    std::sort(h_order.begin(), h_order.end(), [&](int32_t x, int32_t y) {
      const float kx = h_key[(size_t)x], ky = h_key[(size_t)y];
      const bool nx = std::isnan(kx), ny = std::isnan(ky);
      if (nx != ny) return ny;
      if (!nx && kx != ky) return kx < ky;
      return x < y;
    });
    for (int64_t i = 0; i < n; i++) h_wkey[(size_t)i] = h_key[(size_t)h_order[(size_t)i]];
    ASL_TRY(ix->wf_key.upload(h_wkey.data(), (size_t)n));
    ASL_TRY(sync_stream());
  }
  ASL_TRY(ix->ids.upload(h_order.data(), (size_t)n));
  if (n > 0 && ix->d <= 65535) {
    std::vector<int32_t> blk_off = {0, (int32_t)((n + FI_BLK - 1) / FI_BLK)}, pos_blk((size_t)n);
    std::vector<uint16_t> pos_loc((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      pos_blk[(size_t)i] = (int32_t)(i / FI_BLK);
      pos_loc[(size_t)i] = (uint16_t)(i % FI_BLK);
    }
    ASL_TRY(build_postings(ix, ix->ids.p, n, blk_off, pos_blk, pos_loc));
  }
  ASL_TRY(sync_stream());
  ix->lists_dirty = false;
  if (keyed) {
    ix->win_ready = true;
    ix->win_serial = serial;
    ix->win_gen = gen;
  }
  return ASL_OK;
}

// (id, window value) per storage slot for the post-filter of the scans' finish
__global__ void make_idpay_kernel(const int32_t *__restrict__ slot_ids, int64_t nslots,
                                  const float *__restrict__ payload, int64_t n, int2 *__restrict__ out) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i >= nslots) return;
  const int32_t id = slot_ids[i];
  const float v = (id >= 0 && id < n) ? payload[id] : __builtin_nanf("");
  out[i] = make_int2(id, __float_as_int(v));
}

// ix->idpay for the window column p.payload of library `serial`, rewritten on the CURRENT stream: its only readers are
// the scans index_search_device launches behind this call on that stream (the pipeline keeps every scan on its stream
// B, every other entry point drains it first), so the rewrite is ordered after every scan that read the old pairs. A
// host that changes asl_set_stream between two libraries on one index synchronises the old stream first (as before).
int post_filter_pairs(asl_index *ix, const IndexPostFilter &p, uint64_t serial, uint64_t gen,
                      const int32_t *slot_ids, int64_t nslots) {
  if (ix->idpay_ready && ix->pay_serial == serial && ix->pay_gen == gen && ix->pay_n == p.n) return ASL_OK;
  ASL_TRY(ix->idpay.reserve((size_t)std::max<int64_t>(nslots, 1)));
  if (nslots > 0) {
    hipLaunchKernelGGL(make_idpay_kernel, grid_2d(cdiv(nslots, 256)), dim3(256), 0, stream(), slot_ids, nslots,
                       p.payload, p.n, ix->idpay.p);
    ASL_CHECK_LAUNCH();
  }
  ix->pay_serial = serial;
  ix->pay_gen = gen;
  ix->pay_n = p.n;
  ix->idpay_ready = true;
  return ASL_OK;
}

// ix->sel_words / wsel_words for the selector of rq, rewritten on the CURRENT stream when they hold another
// selector's bits (post_filter_pairs says why that orders the rewrite behind every scan that read the old
// words). window: the words of the window-ordered copy (which is installed by then).
int selector_words(asl_index *ix, const IndexSearch &rq, bool window, const unsigned long long **words) {
  DevBuf<unsigned long long> &buf = window ? ix->wsel_words : ix->sel_words;
  bool &ready = window ? ix->wsel_ready : ix->sel_ready;
  uint64_t &serial = window ? ix->wsel_serial : ix->sel_serial, &gen = window ? ix->wsel_gen : ix->sel_gen;
  *words = nullptr;
  if (!(ready && serial == rq.serial && gen == rq.gen)) {
    ready = false;
    if (ix->kind == ASL_INDEX_IVFPQ) {
      const int64_t ntiles = ix->n_tile_slots / 64;
      ASL_TRY(buf.reserve((size_t)std::max<int64_t>(ntiles, 1)));
      ASL_TRY(tile_selector(window ? ix->wids_tiled.p : ix->ids_tiled.p, ntiles, rq.sel_keep, rq.sel_n, buf.p));
    } else {
      ASL_TRY(buf.reserve((size_t)std::max<int64_t>(ix->n_blocks, 1) * flat_selector_words_per_block()));
      ASL_TRY(flat_selector(postings_view(ix), rq.sel_keep, rq.sel_n, buf.p));
    }
    serial = rq.serial;
    gen = rq.gen;
    ready = true;
  }
  *words = buf.p;
  return ASL_OK;
}

// ---- window scan (asl_index_set_window_key / _search_window / _set_window_scan)
// nullptr when the index can hold the window-ordered layout, else why not
const char *window_unsupported(const asl_index *ix) {
  if (ix->kind != ASL_INDEX_IVFPQ) return "the window scan needs an IVF-PQ index (not IVF-Flat or Flat)";
  if (!tiled_index(ix)) return "the window scan needs the tiled IVF-PQ scan (m = 32, 8 bits, d <= 1020)";
  if (ix->shard_world > 1 || ix->has_vids) return "the window scan does not run on a sharded index";
  return nullptr;
}

// The window-ordered layout from key[id] (n == ntotal; host or device): every list's vectors sorted by
// (key ascending, NaN last, id ascending) and tiled by tile_codes_kernel into that slot order, plus the
// key per slot. (serial, gen) record where the key came from (asl_library serial and the generation of its
// selection; 0: the caller's).
int window_install(asl_index *ix, int64_t n, const float *key, uint64_t serial, uint64_t gen) {
  if (ix->kind == ASL_INDEX_WINFLAT) {      // the one-list layout in key order
    if (n != ix->ntotal) return fail(ASL_ERR_INVALID, "window key: %lld keys for %lld vectors", (long long)n,
                                     (long long)ix->ntotal);
    if (n > 0 && !key) return fail(ASL_ERR_INVALID, "window key: null key");
    return winflat_layout(ix, true, key, serial, gen);
  }
  if (const char *why = window_unsupported(ix)) return fail(ASL_ERR_STATE, "%s", why);
  if (!ix->trained) return fail(ASL_ERR_STATE, "window key: index is not trained");
  if (n != ix->ntotal) return fail(ASL_ERR_INVALID, "window key: %lld keys for %lld vectors", (long long)n,
                                   (long long)ix->ntotal);
  if (n > 0 && !key) return fail(ASL_ERR_INVALID, "window key: null key");
  ASL_TRY(build_lists(ix));
  if (!ix->has_tiles) return fail(ASL_ERR_STATE, "window key: the index has no tiled layout");
  ix->win_ready = false;
  ix->wsel_ready = false;         // (the words follow the slot order about to change)
  std::vector<float> h_key((size_t)n);
  std::vector<int32_t> h_ids((size_t)n);
  if (n) {
    HIP_TRY(hipMemcpy(h_key.data(), key, (size_t)n * 4, hipMemcpyDefault));
    ASL_TRY(ix->ids.download(h_ids.data(), (size_t)n));
    ASL_TRY(sync_stream());
  }
  const auto &off = ix->h_list_offsets;
  std::vector<int32_t> tile_off((size_t)ix->nlist + 1, 0), dst_slot((size_t)n), perm;
  for (int l = 0; l < ix->nlist; l++)
    tile_off[(size_t)l + 1] = tile_off[(size_t)l] + (off[(size_t)l + 1] - off[(size_t)l] + 63) / 64;
  const int64_t ntiles = std::max<int64_t>(tile_off[(size_t)ix->nlist], 1);
  std::vector<float> h_wkey((size_t)ntiles * 64, __builtin_nanf(""));
  auto kv = [&](int32_t i) { return h_key[(size_t)h_ids[(size_t)i]]; };
  for (int l = 0; l < ix->nlist; l++) {
    const int32_t b = off[(size_t)l], e = off[(size_t)l + 1];
    perm.resize((size_t)(e - b));
    std::iota(perm.begin(), perm.end(), b);
    std::sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) {
      const float kx = kv(x), ky = kv(y);
      const bool nx = std::isnan(kx), ny = std::isnan(ky);
      if (nx != ny) return ny;
      if (!nx && kx != ky) return kx < ky;
      return h_ids[(size_t)x] < h_ids[(size_t)y];
    });
    for (int32_t r = 0; r < e - b; r++) {
      const int64_t slot = (int64_t)tile_off[(size_t)l] * 64 + r;
      dst_slot[(size_t)perm[(size_t)r]] = (int32_t)slot;
      h_wkey[(size_t)slot] = kv(perm[(size_t)r]);
    }
  }
  DevBuf<int32_t> slot_dev;
  ASL_TRY(slot_dev.upload(dst_slot.data(), (size_t)n));
  ASL_TRY(ix->wcodes_tiled.reserve((size_t)ntiles * 2048));
  ASL_TRY(ix->wids_tiled.reserve((size_t)ntiles * 64));
  ASL_TRY(ix->wkey_tiled.upload(h_wkey.data(), h_wkey.size()));
  ASL_TRY(tile_codes(ix->codes.p, ix->ids.p, slot_dev.p, n, ntiles, ix->wcodes_tiled.p, ix->wids_tiled.p));
  ASL_TRY(sync_stream());
  ix->win_ready = true;
  ix->win_serial = serial;
  ix->win_gen = gen;
  return ASL_OK;
}

}  // namespace asl

using namespace asl;

extern "C" {

int asl_index_flat_layout(asl_index_t *ix) {
  clear_error();
  if (!ix || (ix->kind != ASL_INDEX_IVFFLAT && ix->kind != ASL_INDEX_WINFLAT))
    return fail(ASL_ERR_INVALID, "flat_layout: an IVF-Flat or window-exact index is required");
  if (ix->trained && ix->n_store > 0) {
    ASL_TRY(ensure_device());
    ASL_TRY(build_lists(ix));
  }
  return ix->has_inv ? ix->inv_layout : 0;
}

int asl_index_set_window_key(asl_index_t *ix, int64_t n, const float *key) {
  clear_error();
  ASL_TRY(ensure_device());
  if (!ix) return fail(ASL_ERR_INVALID, "set_window_key: null index");
  return window_install(ix, n, key, 0);
}

int asl_index_get_lists(const asl_index_t *cix, int32_t *list_offsets, int32_t *ids,
                        uint8_t *codes, float *vecs) {
  clear_error();
  asl_index *ix = const_cast<asl_index *>(cix);
  if (!ix || !ivf_kind(ix->kind)) return fail(ASL_ERR_STATE, "get_lists: IVF index required");
  ASL_TRY(build_lists(ix));
  const int64_t n = ix->n_store;
  if (list_offsets)
    HIP_TRY(hipMemcpyAsync(list_offsets, ix->list_offsets.p, ((size_t)ix->nlist + 1) * 4, hipMemcpyDefault, stream()));
  if (ids && n) HIP_TRY(hipMemcpyAsync(ids, ix->ids.p, (size_t)n * 4, hipMemcpyDefault, stream()));
  if (codes && n) {
    if (ix->kind != ASL_INDEX_IVFPQ) return fail(ASL_ERR_STATE, "get_lists: no PQ codes in this index");
    HIP_TRY(hipMemcpyAsync(codes, ix->codes.p, (size_t)n * ix->pq_m, hipMemcpyDefault, stream()));
  }
  if (vecs && n) {
    if (ix->kind != ASL_INDEX_IVFFLAT) return fail(ASL_ERR_STATE, "get_lists: no flat vectors in this index");
    // list order = stable sort of add order by list: reuse ids when unsharded
    std::vector<int32_t> h_vlist((size_t)n);
    ASL_TRY(ix->vlist.download(h_vlist.data(), (size_t)n));
    ASL_TRY(sync_stream());
    std::vector<int64_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return h_vlist[(size_t)a] < h_vlist[(size_t)b]; });
    DevBuf<int64_t> od;
    DevBuf<float> tmp;
    ASL_TRY(od.upload(order.data(), (size_t)n));
    ASL_TRY(tmp.reserve((size_t)n * ix->d));
    ASL_TRY(gather_rows_f32(ix->vecs.p, ix->d, od.p, n, ix->d, tmp.p, ix->d));
    HIP_TRY(hipMemcpyAsync(vecs, tmp.p, (size_t)n * ix->d * 4, hipMemcpyDefault, stream()));
    ASL_TRY(sync_stream());
  }
  return sync_stream();
}

}  // extern "C"
