// index_shard.hip -- list ownership of a sharded index (LPT over the expected scan load); asl_index_shard keeps a rank's lists.
#include <algorithm>
#include <numeric>

#include "index.hpp"

using namespace asl;

extern "C" {

// the shards' own k (exchange.hip "shard-side k_s < k"; profiles/r05_sim_rank.txt: k / 2 at 8 ranks takes
// 0.3 (IVF-PQ) / 0.9 ms (IVF-Flat) off the shard scan, 0.25 % / 0.04 % of a shard's rows are scanned a second time)
int32_t asl_shard_k(int32_t k, int32_t world) {
  if (k < 1 || world < 4) return k;
  const int raw = world >= 8 ? (k + 1) / 2 : (5 * k + 7) / 8;
  const int ks = std::min(k, (raw + 63) / 64 * 64);
  const int head = std::min(k, (2 * k + world - 1) / world);
  return ks > head ? ks : k;
}

static void lpt_owner(const std::vector<int64_t> &sizes, int world, std::vector<int32_t> &owner) {
  const int nlist = (int)sizes.size();
  std::vector<int> order((size_t)nlist);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sizes[(size_t)a] > sizes[(size_t)b]; });
  std::vector<int64_t> load((size_t)world, 0);
  owner.assign((size_t)nlist, 0);
  for (int l : order) {
    int best = 0;
    for (int r = 1; r < world; r++)
      if (load[(size_t)r] < load[(size_t)best]) best = r;
    owner[(size_t)l] = best;
    load[(size_t)best] += sizes[(size_t)l];
  }
}

static int list_sizes(asl_index *ix, std::vector<int32_t> &h_vlist, std::vector<int64_t> &sizes) {
  const int64_t n = ix->n_store;
  h_vlist.resize((size_t)n);
  if (n) {
    ASL_TRY(ix->vlist.download(h_vlist.data(), (size_t)n));
    ASL_TRY(sync_stream());
  }
  sizes.assign((size_t)ix->nlist, 0);
  for (int64_t i = 0; i < n; i++) sizes[(size_t)h_vlist[(size_t)i]]++;
  return ASL_OK;
}

int asl_lpt_owner(int32_t nlist, const int64_t *sizes, int32_t world, int32_t *owner_out) {
  clear_error();
  if (nlist < 0 || world <= 0 || (nlist && (!sizes || !owner_out)))
    return fail(ASL_ERR_INVALID, "lpt_owner: bad arguments");
  std::vector<int64_t> sz(sizes, sizes + nlist);
  std::vector<int32_t> owner;
  lpt_owner(sz, world, owner);
  if (nlist) memcpy(owner_out, owner.data(), owner.size() * 4);
  return ASL_OK;
}

// Ownership balances the EXPECTED SCAN LOAD, not the stored vectors: a list is probed
// roughly in proportion to its population (dense regions attract queries as well as library
// spectra), so its expected contribution to a query's scan is ~ size^2. Measured on the
// 2.1M-spectrum bench library, 8 shards: max/mean scanned vectors 1.094 with weights = size,
// 1.039 with size^2 (stored vectors then differ by +-5 %).
static void shard_owner(const std::vector<int64_t> &sizes, int world, std::vector<int32_t> &owner) {
  std::vector<int64_t> w(sizes.size());
  for (size_t i = 0; i < sizes.size(); i++) w[i] = sizes[i] * sizes[i];
  lpt_owner(w, world, owner);
}

int asl_index_shard_map(const asl_index_t *cix, int32_t world, int32_t *owner_out) {
  clear_error();
  asl_index *ix = const_cast<asl_index *>(cix);
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "shard_map: a window-exact index has one list and is not sharded");
  if (!ix || ix->kind == ASL_INDEX_FLAT || world <= 0 || !owner_out)
    return fail(ASL_ERR_INVALID, "shard_map: IVF index and world > 0 required");
  if (ix->shard_world > 1) return fail(ASL_ERR_STATE, "shard_map: call before sharding");
  std::vector<int32_t> h_vlist, owner;
  std::vector<int64_t> sizes;
  ASL_TRY(list_sizes(ix, h_vlist, sizes));
  shard_owner(sizes, world, owner);
  memcpy(owner_out, owner.data(), owner.size() * 4);
  return ASL_OK;
}

int asl_index_shard(asl_index_t *ix, int32_t rank, int32_t world) {
  clear_error();
  if (ix && ix->kind == ASL_INDEX_WINFLAT)
    return fail(ASL_ERR_STATE, "shard: a window-exact index has one list and is not sharded");
  if (!ix || ix->kind == ASL_INDEX_FLAT) return fail(ASL_ERR_INVALID, "shard: IVF index required");
  if (world <= 0 || rank < 0 || rank >= world) return fail(ASL_ERR_INVALID, "shard: bad rank/world");
  if (ix->shard_world > 1) return fail(ASL_ERR_STATE, "shard: already sharded");
  if (world == 1) return ASL_OK;
  std::vector<int32_t> h_vlist, owner;
  std::vector<int64_t> sizes;
  ASL_TRY(list_sizes(ix, h_vlist, sizes));
  shard_owner(sizes, world, owner);
  const int64_t n = ix->n_store;
  std::vector<int64_t> keep;
  std::vector<int32_t> keep32, new_vlist;
  for (int64_t i = 0; i < n; i++)
    if (owner[(size_t)h_vlist[(size_t)i]] == rank) {
      keep.push_back(i);
      keep32.push_back((int32_t)i);
      new_vlist.push_back(h_vlist[(size_t)i]);
    }
  const int64_t nk = (int64_t)keep.size();
  if (ix->kind == ASL_INDEX_IVFFLAT) {
    DevBuf<int64_t> kd;
    DevBuf<float> nv;
    ASL_TRY(kd.upload(keep.data(), (size_t)nk));
    ASL_TRY(nv.reserve((size_t)std::max<int64_t>(nk, 1) * ix->d));
    ASL_TRY(gather_rows_f32(ix->vecs.p, ix->d, kd.p, nk, ix->d, nv.p, ix->d));
    ASL_TRY(sync_stream());
    ix->vecs = std::move(nv);
  } else {
    DevBuf<int32_t> kd;
    DevBuf<uint8_t> nc;
    ASL_TRY(kd.upload(keep32.data(), (size_t)nk));
    ASL_TRY(nc.reserve((size_t)std::max<int64_t>(nk, 1) * ix->pq_m));
    ASL_TRY(gather_rows_u8(ix->codes_add.p, kd.p, nk, ix->pq_m, nc.p));
    ASL_TRY(sync_stream());
    ix->codes_add = std::move(nc);
  }
  ASL_TRY(ix->vlist.upload(new_vlist.data(), (size_t)nk));
  ASL_TRY(ix->vids.upload(keep32.data(), (size_t)nk));
  ASL_TRY(sync_stream());
  ix->has_vids = true;
  ix->n_store = nk;
  ix->shard_rank = rank;
  ix->shard_world = world;
  ix->lists_dirty = true;
  return ASL_OK;
}

}  // extern "C"
