// fit_args.hpp -- the host prologue the models of the FDR step share (l2svm.hip, forest.hip): host copies of small
// arguments that may live on either side, and the checks of the shape, the class weights and the labels. who: the
// entry point's name in the messages. Everything here has internal linkage.
#pragma once
#include <cmath>

#include "common.hpp"

namespace asl {
namespace {

template <class T>
int host_copy(std::vector<T> &h, const T *src, size_t n) {   // host copy of an array on either side
  h.resize(n);
  if (n) HIP_TRY(hipMemcpy(h.data(), src, n * sizeof(T), hipMemcpyDefault));
  return ASL_OK;
}
template <class T>
int host_copy_back(T *dst, const std::vector<T> &h) {
  if (!h.empty()) HIP_TRY(hipMemcpy(dst, h.data(), h.size() * sizeof(T), hipMemcpyDefault));
  return ASL_OK;
}

// n_below_2_31: the forest's row ids are 32-bit, and its message says so (the SVM's does not)
int check_shape(const char *who, int64_t n, int32_t d, int32_t P, bool n_below_2_31) {
  if (d < 1 || P < 1 || n < 0 || (n_below_2_31 && n >= (1ll << 31)))
    return fail(ASL_ERR_INVALID,
                n_below_2_31 ? "%s: needs d >= 1, P >= 1, 0 <= n < 2^31" : "%s: needs d >= 1, P >= 1, n >= 0", who);
  if (d > ASL_SVM_MAX_DIM) return fail(ASL_ERR_CAPACITY, "%s: d = %d, at most %d", who, d, ASL_SVM_MAX_DIM);
  if (P > ASL_SVM_MAX_PROBLEMS)
    return fail(ASL_ERR_CAPACITY, "%s: P = %d, at most %d", who, P, ASL_SVM_MAX_PROBLEMS);
  return ASL_OK;
}

int check_class_weights(const char *who, const std::vector<double> &cw) {
  for (double v : cw)
    if (!(v >= 0.0) || !std::isfinite(v))
      return fail(ASL_ERR_INVALID, "%s: class weights must be finite and >= 0", who);
  return ASL_OK;
}

// label: [P, n] on either side, read on the host before anything is launched
int check_labels(const char *who, const int8_t *label, int32_t P, int64_t n) {
  std::vector<int8_t> h_label;
  const int8_t *lp = label;
  const size_t cnt = (size_t)P * (size_t)n;
  if (cnt && is_device_ptr(label)) {
    ASL_TRY(host_copy(h_label, label, cnt));
    lp = h_label.data();
  }
  for (size_t i = 0; i < cnt; ++i)
    if (lp[i] < -1 || lp[i] > 1)
      return fail(ASL_ERR_INVALID, "%s: label[%lld, %lld] = %d, not in {-1, 0, +1}", who, (long long)(i / n),
                  (long long)(i % n), (int)lp[i]);
  return ASL_OK;
}

}  // namespace
}  // namespace asl
