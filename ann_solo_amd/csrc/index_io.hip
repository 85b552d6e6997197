// index_io.hip -- asl_index_save / asl_index_load.
#include <cstdio>
#include <cstring>

#include "index.hpp"

using namespace asl;

extern "C" {

// ---------------------------------------------------------------- persistence
// '<base>_<hash7>_<charge>.idxann' stays the file name (spectral_library.py:98-108);
// the payload is this library's own little-endian format, not FAISS'.
struct IdxHeader {
  char magic[8];
  int32_t version, d, nlist, kind, pq_m, pq_bits, niter, trained;
  int64_t ntotal, n_store;
  int32_t shard_rank, shard_world, has_vids, pad;
};
// IVF-PQ `pad`: bit 0 exact rows follow, bits 1.. refine_k (<= TK_MAX_K), and -- version 3 only -- this bit:
// by_residual is off (raw-vector codes). Builds before version 3 refuse such a file rather than mis-score it.
constexpr int32_t PAD_PQ_RAW = 1 << 30;

int asl_index_save(const asl_index_t *ix, const char *path) {
  clear_error();
  if (!ix || !path) return fail(ASL_ERR_INVALID, "save: null");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(ASL_ERR_IO, "save: cannot open %s", path);
  IdxHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, "ASLIDX01", 8);
  h.version = 2;      // 2: the storage field of an IVF-Flat header is authoritative (see asl_index_load)
  h.d = ix->d;
  h.nlist = ix->nlist;
  h.kind = ix->kind;
  h.pq_m = ix->pq_m;
  h.pq_bits = ix->pq_bits;
  h.niter = ix->niter;
  h.trained = ix->trained;
  h.ntotal = ix->ntotal;
  h.n_store = ix->n_store;
  h.shard_rank = ix->shard_rank;
  h.shard_world = ix->shard_world;
  h.has_vids = ix->has_vids;
  h.pad = ix->refine_rows ? (1 | (ix->refine_k << 1)) : 0;   // IVF-PQ: exact rows follow the payload
  if (ix->kind == ASL_INDEX_IVFFLAT || ix->kind == ASL_INDEX_WINFLAT) h.pad = ix->flat_storage;   // component storage mode
  if (ix->kind == ASL_INDEX_IVFPQ && !ix->by_residual) {          // (a by-residual index: byte for byte version 2)
    h.version = 3;
    h.pad |= PAD_PQ_RAW;
  }
  bool ok = fwrite(&h, sizeof h, 1, f) == 1;
  auto dump = [&](const void *dev, size_t bytes) {
    if (!ok || bytes == 0) return;
    std::vector<char> tmp(bytes);
    if (hipMemcpy(tmp.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      ok = false;
      return;
    }
    ok = fwrite(tmp.data(), 1, bytes, f) == bytes;
  };
  (void)hipStreamSynchronize(stream());
  if (ix->trained && ivf_kind(ix->kind)) dump(ix->centroids.p, (size_t)ix->nlist * ix->d * 4);
  if (ix->trained && ix->kind == ASL_INDEX_IVFPQ) dump(ix->codebooks.p, (size_t)ix->pq_m * ix->ksub * ix->dsub * 4);
  const size_t n = (size_t)ix->n_store;
  if (ivf_kind(ix->kind)) dump(ix->vlist.p, n * 4);
  if (ix->has_vids) dump(ix->vids.p, n * 4);
  if (ix->kind == ASL_INDEX_IVFPQ)
    dump(ix->codes_add.p, n * ix->pq_m);
  else
    dump(ix->vecs.p, n * ix->d * 4);
  if (ix->refine_rows) {
    const size_t rn = (size_t)ix->r_n, S = (size_t)refine_stride();
    dump(ix->r_cnt.p, rn);
    dump(ix->r_dim.p, rn * S * 2);
    dump(ix->r_val.p, rn * S * 4);
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) return fail(ASL_ERR_IO, "save: write to %s failed", path);
  return ASL_OK;
}

asl_index_t *asl_index_load(const char *path) {
  clear_error();
  if (!path) {
    fail(ASL_ERR_INVALID, "load: null path");
    return nullptr;
  }
  if (ensure_device() != ASL_OK) return nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fail(ASL_ERR_IO, "load: cannot open %s", path);
    return nullptr;
  }
  IdxHeader h;
  if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, "ASLIDX01", 8) != 0) {
    fclose(f);
    fail(ASL_ERR_IO, "load: %s is not an annsolo_mi index", path);
    return nullptr;
  }
  // never trust a file. Its shape passes the check asl_index_create makes, so that what loads can be searched ...
  if (index_shape_check("load", h.d, h.nlist, h.kind, h.pq_m, h.pq_bits) != ASL_OK) {
    fclose(f);
    return nullptr;
  }
  bool raw = false;      // IVF-PQ, version 3: codes of the raw vectors (by_residual off)
  {  // ... and every count below sizes a host vector or a device allocation
    const char *bad = nullptr;
    const bool ivf = h.kind == ASL_INDEX_IVFFLAT || h.kind == ASL_INDEX_IVFPQ;
    raw = h.kind != ASL_INDEX_IVFFLAT && h.kind != ASL_INDEX_WINFLAT && h.pad >= 0 && (h.pad & PAD_PQ_RAW);
    if (raw) h.pad &= ~PAD_PQ_RAW;      // (the refine bits below it are checked and read as ever)
    if (h.version < 1 || h.version > 3) bad = "unsupported version";
    else if (h.kind < ASL_INDEX_FLAT || h.kind > ASL_INDEX_WINFLAT) bad = "unknown index kind";
    else if (h.d <= 0 || h.d > (1 << 20)) bad = "bad dimension";
    else if (ivf && (h.nlist <= 0 || h.nlist > (1 << 24))) bad = "bad nlist";
    else if (h.n_store < 0 || h.ntotal < h.n_store || h.ntotal >= ((int64_t)1 << 31)) bad = "bad vector counts";
    else if (h.niter < 0 || (h.trained != 0 && h.trained != 1) || (h.has_vids != 0 && h.has_vids != 1)) bad = "bad flags";
    else if (h.shard_world < 1 || h.shard_rank < 0 || h.shard_rank >= h.shard_world) bad = "bad shard fields";
    else if (!h.trained && h.n_store > 0 && ivf) bad = "vectors in an untrained index";
    else if (h.kind == ASL_INDEX_WINFLAT && (h.has_vids || h.shard_world != 1 || h.n_store != h.ntotal || !h.trained))
      bad = "bad fields for a window-exact index";
    else if (h.kind == ASL_INDEX_IVFFLAT || h.kind == ASL_INDEX_WINFLAT ? (h.pad != ASL_FLAT_FX22 && h.pad != ASL_FLAT_F32)
                                         : (h.pad < 0 || ((h.pad & 1) && h.kind != ASL_INDEX_IVFPQ) || (h.pad >> 1) > TK_MAX_K))
      bad = "bad refine / storage fields";
    else if (raw && (h.kind != ASL_INDEX_IVFPQ || h.version < 3)) bad = "bad refine / storage fields";
    if (!bad) {  // the payload must be exactly what the header announces
      const uint64_t ksub = h.kind == ASL_INDEX_IVFPQ ? (1ull << h.pq_bits) : 0;
      uint64_t want = sizeof h;
      if (h.trained && ivf) want += (uint64_t)h.nlist * h.d * 4;
      if (h.trained && h.kind == ASL_INDEX_IVFPQ) want += (uint64_t)h.pq_m * ksub * (uint64_t)(h.d / h.pq_m) * 4;
      if (ivf) want += (uint64_t)h.n_store * 4;
      if (h.has_vids) want += (uint64_t)h.n_store * 4;
      want += h.kind == ASL_INDEX_IVFPQ ? (uint64_t)h.n_store * h.pq_m : (uint64_t)h.n_store * h.d * 4;
      if (h.kind == ASL_INDEX_IVFPQ && (h.pad & 1)) want += (uint64_t)h.ntotal * (1 + (uint64_t)refine_stride() * 6);
      const long here = ftell(f);
      if (fseek(f, 0, SEEK_END) != 0 || (uint64_t)ftell(f) != want) bad = "file size does not match the header";
      fseek(f, here, SEEK_SET);
    }
    if (bad) {
      fclose(f);
      fail(ASL_ERR_IO, "load: %s: %s", path, bad);
      return nullptr;
    }
  }
  asl_index *ix = new asl_index();
  ix->d = h.d;
  ix->nlist = h.kind == ASL_INDEX_WINFLAT ? 0 : h.nlist;      // (unread by that kind)
  ix->kind = h.kind;
  ix->pq_m = h.pq_m;
  ix->pq_bits = h.pq_bits;
  ix->niter = h.niter;
  ix->trained = h.trained;
  ix->ntotal = h.ntotal;
  ix->n_store = h.n_store;
  ix->shard_rank = h.shard_rank;
  ix->shard_world = h.shard_world;
  ix->has_vids = h.has_vids;
  if (ix->kind == ASL_INDEX_IVFPQ) {
    ix->ksub = 1 << ix->pq_bits;
    ix->dsub = ix->d / ix->pq_m;
    ix->by_residual = !raw;
  }
  bool ok = true;
  auto slurp = [&](auto &buf, size_t count) {
    using T = typename std::remove_reference<decltype(*buf.p)>::type;
    if (!ok || count == 0) return;
    std::vector<T> tmp(count);
    if (fread(tmp.data(), sizeof(T), count, f) != count) {
      ok = false;
      return;
    }
    if (buf.reserve(count) != ASL_OK ||
        hipMemcpy(buf.p, tmp.data(), count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      ok = false;
  };
  if (ix->trained && ivf_kind(ix->kind)) slurp(ix->centroids, (size_t)ix->nlist * ix->d);
  if (ix->trained && ix->kind == ASL_INDEX_IVFPQ) slurp(ix->codebooks, (size_t)ix->pq_m * ix->ksub * ix->dsub);
  const size_t n = (size_t)ix->n_store;
  if (ivf_kind(ix->kind)) slurp(ix->vlist, n);
  if (ix->has_vids) slurp(ix->vids, n);
  if (ix->kind == ASL_INDEX_IVFPQ)
    slurp(ix->codes_add, n * ix->pq_m);
  else
    slurp(ix->vecs, n * ix->d);
  if (ix->kind == ASL_INDEX_WINFLAT) ix->flat_storage = h.pad;
  if (ix->kind == ASL_INDEX_IVFFLAT) {
    ix->flat_storage = h.pad;
    // version 1: the field was 0 both for fixed-point files and for the unrounded float32 files
    // of the builds before the storage modes existed -- the components say which
    if (ok && h.version == 1 && h.pad == ASL_FLAT_FX22 && n > 0) {
      DevBuf<int32_t> nnz, nnz_max;
      int32_t h_nm[2] = {0, 0};
      ok = nnz.reserve(n) == ASL_OK && nnz_max.reserve(2) == ASL_OK &&
           count_nnz(ix->vecs.p, ix->d, (int64_t)n, nnz.p, nnz_max.p) == ASL_OK &&
           nnz_max.download(h_nm, 2) == ASL_OK && sync_stream() == ASL_OK;
      if (ok && h_nm[1] != 0) ix->flat_storage = ASL_FLAT_F32;
    }
  }
  if (ix->kind == ASL_INDEX_IVFPQ && (h.pad & 1)) {
    const size_t rn = (size_t)ix->ntotal, S = (size_t)refine_stride();
    ix->refine_rows = true;
    ix->refine_k = h.pad >> 1;
    ix->r_n = ix->ntotal;
    if (rn) {
      slurp(ix->r_cnt, rn);
      slurp(ix->r_dim, rn * S);
      slurp(ix->r_val, rn * S);
    }
  }
  fclose(f);
  if (ok && ix->n_store > 0 && (ivf_kind(ix->kind) || ix->has_vids)) {
    // list assignments / global ids index host and device arrays later: range-check them now
    std::vector<int32_t> tmp((size_t)ix->n_store);
    if (ivf_kind(ix->kind)) {
      ok = hipMemcpy(tmp.data(), ix->vlist.p, tmp.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
      for (size_t i = 0; ok && i < tmp.size(); i++) ok = tmp[i] >= 0 && tmp[i] < ix->nlist;
    }
    if (ok && ix->has_vids) {
      ok = hipMemcpy(tmp.data(), ix->vids.p, tmp.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
      for (size_t i = 0; ok && i < tmp.size(); i++) ok = tmp[i] >= 0 && (int64_t)tmp[i] < ix->ntotal;
    }
    if (!ok) {
      delete ix;
      fail(ASL_ERR_IO, "load: %s holds list or id entries out of range", path);
      return nullptr;
    }
  }
  if (!ok) {
    delete ix;
    fail(ASL_ERR_IO, "load: %s is truncated or unreadable", path);
    return nullptr;
  }
  ix->lists_dirty = true;
  return ix;
}

}  // extern "C"
