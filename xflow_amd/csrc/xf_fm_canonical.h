// xf_fm_canonical.h — the host entry points of xf_fm_canonical.hip (canonical FM, binary and
// valued) and xf_valued.hip (valued LR).  Their contracts are stated where they are defined.
#ifndef XF_FM_CANONICAL_H_
#define XF_FM_CANONICAL_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "xf_device.h"

namespace xf {

// canonical FM (xf_fm_canonical.hip); a null value pointer: a binary minibatch
size_t fmc_heavy_doubles(const xf_dev_batch *b, int k);
int fmc_forward(const xf_dev_batch *b, int k, const float *d_wu, const float *d_vu, float *d_S,
                float *d_loss, float *d_pctr, const float *d_xval, hipStream_t s);
int fmc_grad_update(xf_table *tw, xf_table *tv, const xf_dev_batch *b, const uint32_t *d_rows_w,
                    const uint32_t *d_rows_v, const float *d_wu, const float *d_vu,
                    const float *d_S, const float *d_loss, float *d_gw, double *d_hpart,
                    const float *d_coo_val, hipStream_t s);
// the gradient alone (a worker of a sharded trainer: the keys' owners step): d_gw[U] and
// d_gv[U x k], every entry written; no table, state row or pulled w is read
int fmc_grad_emit(const xf_dev_batch *b, int k, const float *d_vu, const float *d_S,
                  const float *d_loss, float *d_gw, float *d_gv, double *d_hpart,
                  const float *d_coo_val, hipStream_t s);
// opt: XF_OPT_*, or kOptEmit (xf_device.h) with d_gv
void fmc_heavy_update(int opt, const TableDev &TW, const TableDev &TV, int k, const xf_dev_batch *b,
                      const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                      const float *d_vu, const float *d_S, const float *d_loss, float *d_gw,
                      float *d_gv, double *d_hpart, const float *d_coo_val, hipStream_t s);

// feature values, LR (xf_valued.hip)
int val_lr_forward(const xf_dev_batch *b, const float *d_xval, const float *d_wu, float *d_loss,
                   float *d_pctr, hipStream_t s);
int val_lr_grad_update(xf_table *tw, const xf_dev_batch *b, const float *d_coo_val,
                       const uint32_t *d_rows_w, const float *d_wu, const float *d_loss,
                       float *d_gw, double *d_hpart, hipStream_t s);
// the gradient alone: d_gw[U], every entry written; d_hpart as val_lr_grad_update's
int val_lr_grad_emit(const xf_dev_batch *b, const float *d_coo_val, const float *d_loss,
                     float *d_gw, double *d_hpart, hipStream_t s);

}  // namespace xf
#endif  // XF_FM_CANONICAL_H_
