// library.hip -- the library handle of one charge partition (struct asl_library, library.hpp): the processed
// library spectra resident in HBM as columns, as one packed slot per row for the rescoring kernels and as a
// precursor-sorted view for the window search; its group column and its row selection.
#include <atomic>
#include <memory>

#include "library.hpp"

namespace asl {

// The effective columns of a library with a selection (asl_library_set_selection): the window column with
// NaN where the row is unselected (or was NaN: invalid), the validity flags with 0 there.
__global__ void selection_columns_kernel(const uint8_t *__restrict__ keep, const float *__restrict__ wcol,
                                         const uint8_t *__restrict__ valid, int64_t n,
                                         float *__restrict__ wcol_eff, uint8_t *__restrict__ valid_eff) {
  const int64_t i = block_linear() * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool on = keep[i] != 0;
  wcol_eff[i] = on ? wcol[i] : __builtin_nanf("");
  valid_eff[i] = (on && (!valid || valid[i])) ? 1 : 0;
}

}  // namespace asl

using namespace asl;

// one wave per spectrum: its row record and its peaks from the three arrays into its slot
__global__ void pack_records_kernel(const int32_t *__restrict__ offsets, const float *__restrict__ mz,
                                    const float *__restrict__ inten, const uint8_t *__restrict__ chg,
                                    const RowMeta *__restrict__ meta, int64_t n, uint32_t slot,
                                    uint8_t *__restrict__ rec) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int co = offsets[r], cn = offsets[r + 1] - co;
  uint8_t *s0 = rec + (size_t)r * slot;
  if (lane < 8) reinterpret_cast<uint32_t *>(s0)[lane] = reinterpret_cast<const uint32_t *>(meta + r)[lane];
  uint8_t *b = rec + (size_t)meta[r].rec4 * 4;      // = s0 + 32
  float *f = reinterpret_cast<float *>(b);
  for (int j = lane; j < cn; j += 64) {
    f[j] = mz[co + j];
    b[4 * (size_t)cn + j] = chg[co + j];
    f[rec_int0(cn) + j] = inten[co + j];
  }
}

// Host copies of the per-row arrays that the steps of asl_library_create share: one download per array.
struct HostRows {
  std::vector<int32_t> off, chg;
  std::vector<double> pmz;
  std::vector<float> pmz32;       // spec_info's float32 precursor column (the caller's, or pmz rounded)
  std::vector<uint8_t> valid;     // 1 where no flags were given
  explicit HostRows(size_t n) : off(n + 1), chg(n), pmz(n), pmz32(n), valid(n, 1) {}
};

// Step 1: the columns, from the staged peaks (device pointers), and their host copies.
static int library_columns(asl_library *L, const DevPeaks &src, const float *lib_pmz_f32, const uint8_t *valid,
                           HostRows &H) {
  const size_t n = (size_t)L->n, np = (size_t)src.n_peaks;
  ASL_TRY(L->offsets.upload(src.offsets, n + 1));
  ASL_TRY(L->mz.upload(src.mz, np));
  ASL_TRY(L->intensity.upload(src.intensity, np));
  if (src.charge) {
    ASL_TRY(L->charge.upload(src.charge, np));
  } else if (np) {
    ASL_TRY(L->charge.reserve(np));
    HIP_TRY(hipMemsetAsync(L->charge.p, 0, np, stream()));
  }
  ASL_TRY(L->pmz.upload(src.precursor_mz, n));
  ASL_TRY(L->pcharge.upload(src.precursor_charge, n));
  if (n) {
    ASL_TRY(L->offsets.download(H.off.data(), n + 1));
    ASL_TRY(L->pcharge.download(H.chg.data(), n));
    ASL_TRY(L->pmz.download(H.pmz.data(), n));
    ASL_TRY(sync_stream());
    if (lib_pmz_f32) {
      HIP_TRY(hipMemcpy(H.pmz32.data(), lib_pmz_f32, n * 4, hipMemcpyDefault));
    } else {
      for (size_t i = 0; i < n; i++) H.pmz32[i] = (float)H.pmz[i];
    }
    if (valid) HIP_TRY(hipMemcpy(H.valid.data(), valid, n, hipMemcpyDefault));
  }
  ASL_TRY(L->pmz32.upload(H.pmz32.data(), n));
  if (valid) {
    ASL_TRY(L->valid.upload(valid, n));
    L->has_valid = true;
  }
  return ASL_OK;
}

// Step 2: the row records and slots, and the window column: NaN for invalid spectra (never a candidate).
static int library_records(asl_library *L, const HostRows &H) {
  const size_t n = (size_t)L->n;
  if (!n) return ASL_OK;
  int max_cn = 0;
  for (size_t i = 0; i < n; i++) max_cn = std::max(max_cn, H.off[i + 1] - H.off[i]);
  // slot = row record + the largest packed peak record, rounded up to whole 128-byte lines
  const uint64_t slot = (sizeof(RowMeta) + asl::rec_bytes((uint64_t)max_cn) + 127) & ~127ull;
  if ((uint64_t)n * slot >= (1ull << 34))       // rec4 is 32 bits of 4-byte units
    return fail(ASL_ERR_CAPACITY, "library_create: more than 16 GiB of row slots (%llu rows x %llu bytes) in one partition",
                (unsigned long long)n, (unsigned long long)slot);
  std::vector<RowMeta> hm(n);
  std::vector<float> h_wcol(n);
  for (size_t i = 0; i < n; i++) {
    hm[i].off = H.off[i];
    hm[i].cn = H.off[i + 1] - H.off[i];
    hm[i].charge = H.chg[i];
    hm[i].pmz32 = H.valid[i] ? H.pmz32[i] : __builtin_nanf("");
    hm[i].pmz64 = H.pmz[i];
    hm[i].rec4 = (uint32_t)(((uint64_t)i * slot + sizeof(RowMeta)) >> 2);
    hm[i].pad = 0u;
    h_wcol[i] = hm[i].pmz32;
  }
  L->slot = (uint32_t)slot;
  ASL_TRY(L->wcol.upload(h_wcol.data(), n));
  DevBuf<RowMeta> meta_tmp;
  ASL_TRY(meta_tmp.upload(hm.data(), n));
  ASL_TRY(L->records.reserve(n * slot + 16));
  HIP_TRY(hipMemsetAsync(L->records.p, 0, n * slot + 16, stream()));
  hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)cdiv((int64_t)n, 4)), dim3(256), 0, stream(), L->offsets.p,
                     L->mz.p, L->intensity.p, L->charge.p, meta_tmp.p, (int64_t)n, L->slot, L->records.p);
  ASL_CHECK_LAUNCH();
  return sync_stream();     // (meta_tmp and the host arrays are read until here)
}

// Step 3: the precursor-sorted view (host side: one-time, O(n log n)).
static int library_sorted_view(asl_library *L, const HostRows &H) {
  const size_t n = (size_t)L->n;
  std::vector<int32_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return H.pmz32[(size_t)a] < H.pmz32[(size_t)b]; });
  std::vector<float> sp(n);
  for (size_t i = 0; i < n; i++) sp[i] = H.pmz32[(size_t)order[i]];
  ASL_TRY(L->sorted_pmz.upload(sp.data(), n));
  ASL_TRY(L->sorted_row.upload(order.data(), n));
  return sync_stream();
}

extern "C" {

asl_library_t *asl_library_create(const asl_peaks_t *p, const float *lib_pmz_f32,
                                  const uint8_t *valid) {
  clear_error();
  if (!p || p->n < 0) {
    fail(ASL_ERR_INVALID, "library_create: null peaks");
    return nullptr;
  }
  if (ensure_device() != ASL_OK) return nullptr;
  PeaksStage st;
  if (st.init(p) != ASL_OK) return nullptr;
  std::unique_ptr<asl_library> L(new asl_library());
  static std::atomic<uint64_t> next_serial{1};
  L->serial = next_serial.fetch_add(1);
  L->n = p->n;
  HostRows H((size_t)p->n);
  if (library_columns(L.get(), st.dev, lib_pmz_f32, valid, H) != ASL_OK || library_records(L.get(), H) != ASL_OK ||
      library_sorted_view(L.get(), H) != ASL_OK)
    return nullptr;         // (the failing step has set the error)
  L->dev = {.n = (int32_t)p->n, .n_peaks = st.dev.n_peaks, .offsets = L->offsets.p, .mz = L->mz.p,
            .intensity = L->intensity.p, .charge = L->charge.p, .precursor_mz = L->pmz.p,
            .precursor_charge = L->pcharge.p, .records = L->records.p};
  return L.release();
}

void asl_library_free(asl_library_t *L) { delete L; }
int64_t asl_library_size(const asl_library_t *L) { return L ? L->n : 0; }

int asl_library_set_groups(asl_library_t *L, int64_t n, const int32_t *group) {
  clear_error();
  if (!L) return fail(ASL_ERR_INVALID, "library_set_groups: null library");
  if (!group) {
    ASL_TRY(ensure_device());     // (batches in flight may still read the column)
    L->group.release();
    L->has_group = false;
    return ASL_OK;
  }
  if (n != L->n)
    return fail(ASL_ERR_INVALID, "library_set_groups: %lld group ids for a library of %lld rows", (long long)n,
                (long long)L->n);
  ASL_TRY(ensure_device());
  ASL_TRY(L->group.reserve((size_t)std::max<int64_t>(n, 1)));   // (an empty library keeps a column too)
  ASL_TRY(L->group.upload(group, (size_t)n));
  ASL_TRY(sync_stream());         // a host array is the caller's again on return
  L->has_group = true;
  return ASL_OK;
}

int asl_library_set_selection(asl_library_t *L, int64_t n, const uint8_t *keep) {
  clear_error();
  if (!L) return fail(ASL_ERR_INVALID, "library_set_selection: null library");
  if (n != 0 && keep && n != L->n)
    return fail(ASL_ERR_INVALID, "library_set_selection: %lld flags for a library of %lld rows", (long long)n,
                (long long)L->n);
  ASL_TRY(ensure_device());       // (waits for the batches in flight: they read the columns about to change)
  L->has_sel = false;
  ++L->sel_gen;                   // whatever an index derived from the columns so far is out of date
  if (n == 0 || !keep) return ASL_OK;
  ASL_TRY(L->keep.reserve((size_t)n));
  ASL_TRY(L->wcol_eff.reserve((size_t)n));
  ASL_TRY(L->valid_eff.reserve((size_t)n));
  HIP_TRY(hipMemcpyAsync(L->keep.p, keep, (size_t)n, hipMemcpyDefault, stream()));
  hipLaunchKernelGGL(selection_columns_kernel, grid_2d(cdiv(n, 256)), dim3(256), 0, stream(), L->keep.p, L->wcol.p,
                     L->has_valid ? L->valid.p : nullptr, n, L->wcol_eff.p, L->valid_eff.p);
  ASL_CHECK_LAUNCH();
  ASL_TRY(sync_stream());         // a host array is the caller's again on return
  L->has_sel = true;
  return ASL_OK;
}

}  // extern "C"
