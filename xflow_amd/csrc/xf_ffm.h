// xf_ffm.h — the host entry points of xf_ffm.hip (field-aware FM, binary and valued).  Their
// contracts are stated where they are defined.
#ifndef XF_FFM_H_
#define XF_FFM_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "xf_device.h"

namespace xf {

// a null value pointer: a binary minibatch.  d_xfg: the nonzeros' fields in CSR order, every one
// below F (checked when the minibatch was compiled); d_coo_pos: the occurrences' CSR positions in
// key-grouped order.  The v rows are F x k wide, coordinate (h, f) at h k + f.
size_t ffm_heavy_doubles(const xf_dev_batch *b, int dim);
int ffm_forward(const xf_dev_batch *b, int k, int F, const float *d_wu, const float *d_vu,
                const uint32_t *d_xfg, float *d_loss, float *d_pctr, const float *d_xval,
                hipStream_t s);
int ffm_grad_update(xf_table *tw, xf_table *tv, const xf_dev_batch *b, int F,
                    const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                    const float *d_vu, const uint32_t *d_xfg, const uint32_t *d_coo_pos,
                    const float *d_loss, float *d_gw, double *d_hpart, const float *d_xval,
                    hipStream_t s);
// the gradient alone (a worker of a sharded trainer: the keys' owners step): d_gw[U],
// d_gv[U x F k] (untouched coordinates 0) and d_mask[U] (bit h: field h of the key touched),
// every entry written; no table, state row or pulled w is read
int ffm_grad_emit(const xf_dev_batch *b, int k, int F, const float *d_vu, const uint32_t *d_xfg,
                  const uint32_t *d_coo_pos, const float *d_loss, float *d_gw, float *d_gv,
                  uint64_t *d_mask, double *d_hpart, const float *d_xval, hipStream_t s);

}  // namespace xf
#endif  // XF_FFM_H_
