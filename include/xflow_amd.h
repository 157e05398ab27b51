/*
 * xflow_amd.h — C ABI of libxflow_amd.so: the MI355X-native replacement for the
 * ps-lite push/pull parameter server + worker math of xswang/xflow.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.  Every
 * function returns 0 on success and a non-zero XF_E* code on failure; xf_last_error()
 * returns a thread-local description.  Handles are opaque and NOT thread-safe (one
 * driver thread per device/stream, like one ps-lite customer thread per server).
 *
 * What each group replaces in the reference (paths relative to /root/reference):
 *   xf_hash_bytes / xf_reader_*   src/io/io.h:53, src/io/load_data_from_disk.cc:103-210
 *   xf_table_*                    ps::KVWorker<float>::{Pull,Push,Wait} as used at
 *                                 src/model/lr/lr_worker.cc:170,175 and
 *                                 src/model/fm/fm_worker.cc:228-242, plus the server
 *                                 handlers src/optimizer/ftrl.h:38-152, sgd.h:30-109 and
 *                                 their wiring src/model/server.h:22-31
 *   xf_batch_*                    key build in LRWorker::update, lr_worker.cc:146-166
 *   xf_lr_* / xf_fm_*             calculate_loss / calculate_gradient / update,
 *                                 lr_worker.cc:100-177, fm_worker.cc:126-245
 *   xf_auc_logloss                Base::calculate_auc, src/base/base.h:84-110
 *   XFCreate / XFStartTrain       src/c_api/c_api.h:26-29 (signatures kept verbatim)
 */
#ifndef XFLOW_AMD_H_
#define XFLOW_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XF_OK 0
#define XF_EINVAL 1   /* bad argument */
#define XF_EHIP 2     /* HIP runtime error */
#define XF_EFULL 3    /* table capacity exhausted */
#define XF_EIO 4      /* file open / read error */
#define XF_EPARSE 5   /* malformed libsvm-style input */
#define XF_ENOGPU 6   /* no usable HIP device */

const char *xf_last_error(void);
int xf_version(void);
int xf_device_count(int *count);

/* ---------------------------------------------------------------- key hash / sharding */
/* libstdc++ std::hash<std::string> (io.h:53), bit-exact */
uint64_t xf_hash_bytes(const void *ptr, size_t len);
/* out[i] = hash of the decimal string of (start + i): synthetic fids "0","1",... */
int xf_hash_decimal_range(uint64_t start, size_t n, uint64_t *out);
/* out[i] = hash of the decimal string of ids[i] */
int xf_hash_decimal_ids(const uint64_t *ids, size_t n, uint64_t *out);
/* ps-lite default key-range owner: min(key / (UINT64_MAX / nshards), nshards-1) */
uint32_t xf_shard_of(uint64_t key, uint32_t nshards);

/* ---------------------------------------------------------------- text block reader   */
/* load_minibatch_hash_data_fread (load_data_from_disk.cc:103-210): block = what fits in
 * cap_bytes-1 bytes, cut at the last newline when the buffer fills; label = atof > 1e-7;
 * key = hash of the middle field of fgid:fid:val; val is read only by a reader with feature
 * values switched on (xf_reader_set_values, below). */
typedef struct xf_reader xf_reader;
int xf_reader_open(xf_reader **out, const char *path, size_t cap_bytes);
/* The same reader over a binarized block cache: when `cache_path` holds the
 * blocks of this exact file (size, mtime) at this block size, they are served from it and the
 * text is not touched (*from_cache = 1); otherwise the text is parsed as above and every block
 * is also written to the cache, which becomes valid once a pass has reached end of file. */
int xf_reader_open_cached(xf_reader **out, const char *path, size_t cap_bytes,
                          const char *cache_path, int *from_cache);
int xf_reader_close(xf_reader *r);
/* *yes = 1: the text is a memory mapping (a non-empty regular file) — what xf_reader_peek_text /
 * _copy_text / _skip_text (the GPU tokeniser's feed) work on; 0: an empty file, a pipe: only
 * xf_reader_next* serve it. */
int xf_reader_mapped(xf_reader *r, int *yes);
/* rows_out = 0 at end of file.  Arrays are owned by the reader, valid until next call. */
int xf_reader_next(xf_reader *r, size_t *rows_out, size_t *nnz_out,
                   const uint64_t **rowptr, const uint64_t **keys, const int32_t **fgid,
                   const int32_t **labels);

/* The same, into a block object the caller owns: the arrays stay valid until the block is
 * reused or destroyed, also while the reader already parses the next block on another thread. */
typedef struct xf_block xf_block;
int xf_block_create(xf_block **out);
int xf_block_destroy(xf_block *b);
int xf_reader_next_into(xf_reader *r, xf_block *blk, size_t *rows_out, size_t *nnz_out,
                        const uint64_t **rowptr, const uint64_t **keys, const int32_t **fgid,
                        const int32_t **labels);

/* ---- feature values (not in the reference: its parser stops at the second field) ----
 * xf_reader_set_values(r, 1), before the first block: every token's third field — the bytes after
 * the second colon up to the blank or the end of the line; further colons belong to it — is
 * converted too, value = (float)atof(field), an empty field is 0; an empty token, which duplicates
 * the row's previous key, duplicates its value.  A field of 48 bytes or more, or a value that is
 * not finite, is XF_EPARSE.  Labels, keys, block boundaries and row order do not change.  The
 * values run beside the keys (nnz floats): xf_reader_values for the reader-owned arrays of
 * xf_reader_next, xf_block_values for a block of xf_reader_next_into / xf_reader_parse_text.  The
 * block cache carries no values: a reader opened with xf_reader_open_cached refuses (XF_EINVAL).
 * (The GPU tokeniser carries them after xf_ingest_set_fields.) */
int xf_reader_set_values(xf_reader *r, int on);
int xf_reader_values(xf_reader *r, const float **vals);
int xf_block_values(xf_block *blk, const float **vals);

/* ---- the block as text, for a caller that tokenises it itself (xf_ingest_*) ----
 * xf_reader_peek_text: the next block's text by the block rule above (*len = 0 at the end of the
 * file; mapped files without a block cache); nothing moves until xf_reader_skip_text — any
 * xf_reader_next* call instead parses that block on the host and moves on.
 * xf_reader_copy_text: the peeked text copied to `dst` by `threads` host threads.
 * xf_reader_parse_text: a block's text in memory parsed on the host into `blk` (what
 * xf_reader_next_into yields for that block). */
int xf_reader_peek_text(xf_reader *r, const char **text, size_t *len);
int xf_reader_skip_text(xf_reader *r);
int xf_reader_copy_text(xf_reader *r, char *dst, size_t cap, size_t *len, int threads);
int xf_reader_parse_text(xf_reader *r, const char *text, size_t len, xf_block *blk,
                         size_t *rows_out, size_t *nnz_out, const uint64_t **rowptr,
                         const uint64_t **keys, const int32_t **fgid, const int32_t **labels);

/* ---------------------------------------------------------------- GPU tokeniser       */
/* load_minibatch_hash_data_fread's token loop (load_data_from_disk.cc:126-208) and
 * std::hash<std::string> of every fid (io.h:53) as byte-parallel kernels, for blocks of the
 * common shape — lines "('0'|'1') '\t' field0:fid:rest (' ' field0:fid:rest)* '\n'" with single
 * blanks and no control bytes: label = the digit, one key per token = _Hash_bytes(fid), bit for
 * bit the host parser's arrays.  Any other block (other labels, empty tokens — which the
 * reference duplicates —, CR LF, NUL, a token without two colons, ...) comes back with *ok = 0 and
 * is the host parser's (xf_reader_parse_text).  Not in the reference: its io path is host code;
 * this feeds xf_sharded_compile_dev / xf_lr_update_dev without the keys ever being host arrays. */
typedef struct xf_ingest xf_ingest;
int xf_ingest_create(xf_ingest **out, size_t max_text_bytes);
int xf_ingest_destroy(xf_ingest *g);
/* the pinned staging buffer the next block's text goes to (xf_reader_copy_text) */
int xf_ingest_staging(xf_ingest *g, char **buf, size_t *cap);
/* the staged text on its way to the device, asynchronously on `stream` (a staging thread's own:
 * the copy of the next block runs while the GPU works on this one); the next
 * xf_ingest_block(g, NULL, len, ...) waits for that copy instead of making one */
int xf_ingest_upload(xf_ingest *g, size_t len, void *stream);
/* text == NULL: `len` bytes are in the staging buffer already.  Uploads, tokenises, waits for
 * the counts.  d_keys [nnz] u64, d_rowptr [rows + 1] u32, d_labels [rows] i32: device arrays
 * owned by `g`, valid until its next call. */
int xf_ingest_block(xf_ingest *g, const char *text, size_t len, void *stream,
                    const uint64_t **d_keys, const uint32_t **d_rowptr, const int32_t **d_labels,
                    uint32_t *rows, uint32_t *nnz, int *ok);
/* The tokeniser also reads field0 as the token's fgid (want_fgid) and / or the third field as its
 * feature value (want_vals), for the blocks that follow; the arrays are allocated on first use.
 * The common shape narrows to what the host parser converts without atof: field0 of 1 .. 9
 * decimal digits; a third field — up to the blank or the end of the line, one CR before the
 * newline dropped — that is empty (+0) or ['-'] digits ['.' digits] with 1 .. 15 digits in all,
 * value = (float)(+-(double)digits / 10^fraction digits), bit for bit xf_reader_set_values'.
 * Every other token (exponents, '+', nan, inf, a further colon, ...) hands its block back.
 * xf_ingest_fields: d_fgid [nnz] i32, d_vals [nnz] f32 of the last accepted block, beside d_keys,
 * valid until the next xf_ingest_block; NULL for an array that was not asked for. */
int xf_ingest_set_fields(xf_ingest *g, int want_fgid, int want_vals);
int xf_ingest_fields(xf_ingest *g, const int32_t **d_fgid, const float **d_vals);

/* device memory -> host, blocking (the tokeniser's arrays in tests and small tools) */
int xf_copy_to_host(void *dst, const void *d_src, size_t bytes);

typedef struct xf_table xf_table;

/* ---------------------------------------------------------------- compiled minibatch  */
/* Host-side key build (lr_worker.cc:146-166): sorted unique keys (== unique_keys, the
 * Pull/Push key list) + the two views of all_keys the kernels walk:
 *   CSR:  rowptr[R+1], uidx[NNZ]   (index of each nnz's key in ukeys, row-major order)
 *   COO grouped by key: segptr[U+1], coo_row[NNZ]  (row ids of each key's occurrences)
 *   heavy[H]: indices u whose segment is longer than XF_HEAVY_SEG (wave-per-key path) */
#define XF_HEAVY_SEG 64
#define XF_TILE_NNZ 2048
#define XF_TILE_KEYS 2048
/* gradient tiles are much smaller than forward tiles: a gradient workgroup goes through
 * load -> barrier -> sum -> store once per tile and waits on memory in between, so what counts
 * is how many independent tiles a CU has in flight (FM k = 16, 1e7 occurrences: 482 us with
 * 2048-occurrence tiles, 402 / 340 / 324 us with 1024 / 512 / 256). */
#ifndef XF_GRAD_TILE_NNZ /* (overridable at build time: experiments) */
#define XF_GRAD_TILE_NNZ 256
#endif
#define XF_GRAD_TILE_KEYS XF_GRAD_TILE_NNZ
#define XF_HEAVY_KMAX 64
typedef struct xf_batch xf_batch; /* host arrays + (after upload) device mirror */
int xf_batch_compile(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                     const int32_t *labels, size_t row_begin, size_t row_end);
/* The same key build on the GPU (rocPRIM radix sort + flag/scan/scatter kernels): the
 * compiled batch is born on the device, identical array for array to xf_batch_compile's.
 * _dev takes raw device arrays (d_rowptr row-relative, d_rowptr[0] == 0); _gpu takes the
 * reader's host arrays and a row slice like xf_batch_compile and uploads the raw slice. */
int xf_batch_compile_dev(xf_batch **out, const uint64_t *d_keys, const uint32_t *d_rowptr,
                         const int32_t *d_labels, uint32_t R, uint32_t NNZ, void *stream);
int xf_batch_compile_gpu(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                         const int32_t *labels, size_t row_begin, size_t row_end, void *stream);
/* The generic build of a minibatch WITH FEATURE VALUES (vals[] / d_vals[] beside keys[]): the
 * arrays above plus xval[NNZ] in CSR order (beside uidx) and coo_val[NNZ] in key-grouped order
 * (beside coo_row), on the device, where the _dev / _gpu builds make them (coo_val[j] =
 * xval[position of sorted entry j], the line that writes coo_row); the host build gives the
 * same arrays.  xf_dev_batch is that of a binary minibatch: the two value arrays come from
 * xf_batch_values_dev (after xf_batch_upload for a host-built batch; NULLs for a binary
 * minibatch), their host views from xf_batch_values_host.  xf_lr_step / xf_lr_predict and, with
 * XF_FM_CANONICAL, xf_fm_step / xf_fm_predict compute with x = val on such a minibatch:
 *   wx_r = sum_j w[u_j] x_j, S[r,f] = sum_j v[u_j,f] x_j, y2 = 0.5 (sum_f S^2 - sum_f sum_j (v x)^2),
 *   gw[u] = (sum_occ loss x) / R, gv[u,f] = (sum_occ loss x (S[r,f] - v[u,f] x)) / R
 * (exact fp64 sums of fp32 products; all values 1: the binary path's results bit for bit).
 * XF_FM_REFERENCE, XF_PARITY_REFERENCE_ORDER and xf_workspace_capture refuse it (XF_EINVAL). */
int xf_batch_compile_valued(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                            const float *vals, const int32_t *labels, size_t row_begin,
                            size_t row_end);
int xf_batch_compile_valued_dev(xf_batch **out, const uint64_t *d_keys, const float *d_vals,
                                const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                                uint32_t NNZ, void *stream);
int xf_batch_compile_valued_gpu(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                                const float *vals, const int32_t *labels, size_t row_begin,
                                size_t row_end, void *stream);
int xf_batch_values_dev(const xf_batch *b, const float **xval, const float **coo_val);
int xf_batch_values_host(const xf_batch *b, const float **xval, const float **coo_val);
/* The generic build of a minibatch WITH ITS FIELDS (fgid[] / d_fgid[] beside keys[], the first
 * field of fgid:fid:val; vals / d_vals may be NULL: a binary minibatch): the arrays above plus
 * xfg[NNZ] in CSR order (beside uidx) and coo_pos[NNZ] in key-grouped order (beside coo_row): the
 * CSR position of every occurrence — its field is xfg[coo_pos[j]], and "self" in its row is that
 * position.  Both live in an allocation of their own (xf_dev_batch is unchanged) and come from
 * xf_batch_fields_dev / _host (fields = 0 and NULLs for a minibatch compiled without fields).
 * fields must be in 1 .. 64; a nonzero whose fgid lies outside [0, fields) is XF_EINVAL (the
 * message names the fgid and fields), before anything is built.  What XF_FM_FIELD_AWARE steps. */
int xf_batch_compile_fielded(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                             const int32_t *fgid, const float *vals, const int32_t *labels,
                             size_t row_begin, size_t row_end, int fields);
int xf_batch_compile_fielded_dev(xf_batch **out, const uint64_t *d_keys, const int32_t *d_fgid,
                                 const float *d_vals, const uint32_t *d_rowptr,
                                 const int32_t *d_labels, uint32_t R, uint32_t NNZ, int fields,
                                 void *stream);
int xf_batch_compile_fielded_gpu(xf_batch **out, const uint64_t *rowptr, const uint64_t *keys,
                                 const int32_t *fgid, const float *vals, const int32_t *labels,
                                 size_t row_begin, size_t row_end, int fields, void *stream);
int xf_batch_fields_dev(const xf_batch *b, int *fields, const uint32_t **xfg,
                        const uint32_t **coo_pos);
int xf_batch_fields_host(const xf_batch *b, int *fields, const uint32_t **xfg,
                         const uint32_t **coo_pos);
/* The FM key build (fm_worker.cc:205-225) against the tables themselves: when every key of the
 * minibatch sits in the v table's settled tier (xf_table_defrag) and the w table numbers its rows
 * the same way, the key list comes with its state rows, the key-grouped occurrence lists and
 * the forward's per-nonzero record index from the range-partitioned build (no sort of (key,
 * position) pairs); otherwise this IS xf_batch_compile_dev.  *keyed (optional): 1 when the
 * fast build ran.  Such a minibatch is for xf_fm_step / xf_fm_predict on these two tables
 * (k in {4, 8, 16, 32, 64}, no capture, no parity mode); after a defrag its rows are looked up
 * again and its record index translated at its next use.  xf_batch_compile_fm: the host-array
 * front end (the reader's block arrays and a row slice, like xf_batch_compile_gpu). */
int xf_batch_compile_fm_dev(xf_batch **out, xf_table *w, xf_table *v, const uint64_t *d_keys,
                            const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                            uint32_t NNZ, void *stream, int *keyed);
int xf_batch_compile_fm(xf_batch **out, xf_table *w, xf_table *v, const uint64_t *rowptr,
                        const uint64_t *keys, const int32_t *labels, size_t row_begin,
                        size_t row_end, void *stream, int *keyed);
/* The key build for a table on THIS GPU, without the sort (LR): every raw key is resolved
 * straight to its state row in `t` (insert on first touch, ftrl.h:56; the table grows when
 * needed) and the nonzeros are grouped into cells (row window x 4096-row chunk of the state)
 * by a stable radix pass — no unique-key list, the state row is the key's identity.  The
 * result feeds xf_lr_step / xf_lr_predict on `t` only.  retain_keys != 0 is for minibatches that
 * are kept and replayed (epochs >= 2): the raw arrays stay on the device so that the batch
 * survives a renumbering of the rows (xf_table_defrag), and the cells get the key-sorted copy
 * the forward reads fastest; 0 is for a minibatch that is stepped once and freed. */
int xf_batch_compile_local_dev(xf_batch **out, xf_table *t, const uint64_t *d_keys,
                               const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                               uint32_t NNZ, int retain_keys, void *stream);
int xf_batch_compile_local(xf_batch **out, xf_table *t, const uint64_t *rowptr,
                           const uint64_t *keys, const int32_t *labels, size_t row_begin,
                           size_t row_end, int retain_keys, void *stream);
/* The same for a minibatch with feature values (LR; d_vals / vals: one fp32 per nonzero, beside
 * the keys): the sort-based local build — a probe of `t` per raw key (insert on first touch, the
 * table grows when needed), then one stable radix pass that carries every nonzero's value along
 * with its cell entry.  No key list, no uidx, no coo_val: xf_batch_host / xf_batch_values_* have
 * nothing to show.  xf_lr_step / xf_lr_predict on `t` then run the valued cell kernels:
 *   wx_r = sum_j w[row_j] x_j,   gw = (sum_occ loss_r x_occ) / R, stepped in place
 * — the function of the generic valued minibatch (xf_batch_compile_valued*), bit for bit where
 * its fp64 sums are exact; xf_workspace_fetch yields the loss only.  retain_keys != 0 also keeps
 * the raw values (the rebuild after xf_table_defrag).  XF_PARITY_REFERENCE_ORDER,
 * xf_workspace_capture and xf_fm_step / xf_fm_predict refuse it (XF_EINVAL). */
int xf_batch_compile_local_valued_dev(xf_batch **out, xf_table *t, const uint64_t *d_keys,
                                      const float *d_vals, const uint32_t *d_rowptr,
                                      const int32_t *d_labels, uint32_t R, uint32_t NNZ,
                                      int retain_keys, void *stream);
int xf_batch_compile_local_valued(xf_batch **out, xf_table *t, const uint64_t *rowptr,
                                  const uint64_t *keys, const float *vals, const int32_t *labels,
                                  size_t row_begin, size_t row_end, int retain_keys,
                                  void *stream);
/* shape of a batch's cells once a step / predict has built them: out[0..8) = rows per window,
 * windows, chunks, forward workgroups per window, gradient work items, 0 (reserved), chunks
 * cut into several work items, size of the index space */
int xf_batch_cells_info(const xf_batch *b, uint32_t *out);
/* the forward's own row windows over the key-sorted copy of a kept minibatch (DESIGN.md 3,
 * "forward windows"): out[0..6) = rows per forward window, forward windows, forward workgroups
 * per window, 1 when they differ from xf_batch_cells_info's (else they are those), 1 when the
 * copy has been built, 1 when the batch's last forward ran on them (a chain of segments and a
 * resumed forward do not) */
int xf_batch_fwd_info(const xf_batch *b, uint32_t *out);
/* the rule that picks the forward windows, by itself (no GPU): out[0..4) = forward windows, rows
 * per forward window, forward workgroups per window, the gradient's windows, of a minibatch of R
 * rows and NNZ nonzeros over M index positions under xf_tune("fwd_windows") = tune; flags: 1 a
 * kept minibatch (it has a key-sorted copy), 2 row-id cells, 4 valued cells */
int xf_fwd_windows_rule(uint32_t R, uint64_t NNZ, uint64_t M, int flags, int tune, uint32_t *out);
/* copy a device-built batch's arrays into its host views (xf_batch_host etc. do it on demand) */
int xf_batch_download(xf_batch *b);
int xf_batch_free(xf_batch *b);
int xf_batch_dims(const xf_batch *b, uint32_t *R, uint32_t *NNZ, uint32_t *U, uint32_t *H);
/* host views (owned by the batch) */
int xf_batch_host(const xf_batch *b, const uint64_t **ukeys, const uint32_t **rowptr,
                  const uint32_t **uidx, const uint32_t **segptr,
                  const uint32_t **coo_row, const int32_t **labels,
                  const uint32_t **heavy);
/* panel view (host arrays); *P == 0 when the batch is too small to need panels */
int xf_batch_panels(const xf_batch *b, uint32_t *P, const uint32_t **pptr,
                    const uint32_t **pidx);
int xf_batch_fwd_tiles(const xf_batch *b, uint32_t *ntiles, const uint32_t **tile_ptr,
                       const uint32_t **panel_first, uint32_t *grid);
/* chunk offsets of the heavy keys (host array, H+1 entries) */
int xf_batch_heavy_chunks(const xf_batch *b, uint32_t *H, const uint32_t **chunk_ptr);
/* gradient tiles (host array, ntiles+1 key indices) */
int xf_batch_tiles(const xf_batch *b, uint32_t *ntiles, const uint32_t **tile_ptr);
/* tuning knobs (process-wide): "panel_slice_bytes" (default 1.5 MiB: w_u bytes per panel),
 * "min_panel_nnz" (default 4e6: smaller batches keep the plain CSR forward),
 * "parse_threads" (default 64: threads of the block text parser),
 * "batch_pool_blobs" (default 8: device allocations of freed minibatches kept for reuse by
 * the next compile/upload; 0 returns every one to the driver).
 * Named switches between code paths that are all product code and normally chosen by the shape
 * (tests pin one to run each against the oracle; 0 = by shape): "key_build" (1 the sort-based
 * build, 2 the two-level partition, 3 an empty table's keys through the arrival index too), "old_weight" (1 read, 2 derive from (n, z)), "lr_gradient"
 * (1 the general kernel, 2 / 3 the dense kernel with byte-masked / whole-line stores),
 * "owner_pass" (1 the general loop, 2 / 3 the merged phases, 4 a phase per worker),
 * "valued_lr" (a valued LR minibatch of a one-rank trainer: 1 the generic build + the tile
 * kernels, 2 the local build + the valued cell kernels), "fwd_windows" (the row windows of a
 * kept minibatch's key-sorted copy: 1 the gradient's, 2 .. 32 that many) —
 * xflow_amd/csrc/xf_common.h.  An unknown name, or a value a switch does not take, is XF_EINVAL
 * (a library built with -DXF_EXPERIMENTS also has the experiments' numeric "exp_knob"). */
int xf_tune(const char *name, double value);
/* Size the calling thread's scratch arena of the device-side builders ahead of its first build
 * (a minibatch of NNZ nonzeros needs about 40 B x NNZ + 64 MiB when it meets new keys): a run's
 * first minibatches otherwise grow it build by build.  No-op when it is that large already. */
int xf_scratch_reserve(size_t bytes);
/* Set a device allocation of `bytes` aside in the pool of freed minibatches ("batch_pool_blobs")
 * for the first compile that asks for that much or less (and at least an eighth of it): a run's
 * first minibatch otherwise waits for the driver to map its cells (4-8 B x NNZ; 0.25 ms for
 * 40 MB, measured in its first xf_lr_update_dev).  No-op when such an allocation is waiting
 * already, or without pooling. */
int xf_batch_pool_reserve(size_t bytes);
/* copy to the current device (async on stream); idempotent */
int xf_batch_upload(xf_batch *b, void *stream);

/* device view of a compiled batch: raw device pointers (e.g. torch tensors) */
typedef struct {
  uint32_t R, NNZ, U, H;
  const uint32_t *rowptr;  /* R+1  */
  const uint32_t *uidx;    /* NNZ  */
  const uint64_t *ukeys;   /* U    */
  const uint32_t *segptr;  /* U+1  */
  const uint32_t *coo_row; /* NNZ  */
  const int32_t *labels;   /* R    */
  const uint32_t *heavy;   /* H (may be NULL when H == 0) */
  /* LR forward, panel-major view of the CSR (P == 0: absent, the plain CSR is used).
   * Panel p holds the nonzeros whose uidx lies in [U*p/P, U*(p+1)/P): row r's part is
   * pidx[pptr[p*(R+1)+r] .. pptr[p*(R+1)+r+1]).  Blocks working on panel p gather from
   * one L2-sized slice of w_u; p % 8 selects the XCD. */
  uint32_t P, fwd_ntiles;
  const uint32_t *pptr;    /* P*(R+1) */
  const uint32_t *pidx;    /* NNZ     */
  double *fwd_scratch;     /* P*R partial sums (device scratch owned by the batch) */
  /* forward tiles over the (panel,row) cells s = p*(R+1)+r: tile t = cells
   * [fwd_tile_ptr[t], fwd_tile_ptr[t+1]) of ONE panel, <= XF_TILE_NNZ nonzeros;
   * fwd_panel_first[p] = first tile of panel p.  Workgroup b takes the (b/8)-th tile of the
   * panels p with p % 8 == b % 8 (observed placement: XCD b % 8); fwd_grid = 8 x the longest
   * such list. */
  const uint32_t *fwd_tile_ptr;    /* fwd_ntiles+1 */
  const uint32_t *fwd_panel_first; /* P+1 */
  uint32_t fwd_grid, pad3_;
  /* gradient tiles: tile t covers keys [tile_ptr[t], tile_ptr[t+1]) whose occurrences
   * (<= XF_GRAD_TILE_NNZ of them, <= XF_GRAD_TILE_KEYS keys) are staged through LDS by one
   * workgroup; a heavy key (> XF_HEAVY_SEG occurrences) is a tile of its own, skipped by
   * the tile kernel and handled by the wave-per-key path. */
  uint32_t ntiles, n_heavy_chunks;
  const uint32_t *tile_ptr; /* ntiles+1 */
  /* heavy keys are reduced in chunks of XF_TILE_NNZ occurrences spread over the whole chip
   * (a power-law head key can own millions of occurrences): heavy key h owns chunks
   * [heavy_chunk_ptr[h], heavy_chunk_ptr[h+1]); heavy_scratch holds
   * n_heavy_chunks * (1 + XF_HEAVY_KMAX) partial sums. */
  const uint32_t *heavy_chunk_ptr; /* H+1 (NULL when H == 0) */
  double *heavy_scratch;
} xf_dev_batch;
int xf_batch_dev_view(const xf_batch *b, xf_dev_batch *view);

/* ---------------------------------------------------------------- sharded table       */
enum { XF_OPT_FTRL = 0, XF_OPT_SGD = 1 };
enum {
  XF_INIT_ZERO = 0,    /* ftrl.h:27-36, sgd.h:22-27 */
  XF_INIT_CONST = 1,   /* sgd.h:67-72 (0.001) */
  XF_INIT_HASHNORM = 2 /* deterministic N(0,1)*1e-2 stand-in for ftrl.h:114-120 */
};
typedef struct {
  int32_t opt_kind;     /* XF_OPT_* */
  int32_t dim;          /* 1 for w, k for v */
  int32_t init_kind;    /* XF_INIT_* */
  float init_const;
  uint64_t seed;        /* HASHNORM seed */
  float alpha, beta, lambda1, lambda2; /* ftrl.h:17-20 : 0.05, 1, 5e-5, 10 */
  float lr;                            /* sgd.h:16     : 0.001 */
  uint64_t capacity;    /* slots on THIS shard (keys stored <= capacity) */
  uint32_t shard, nshards; /* key range owned: ps-lite uniform range rule */
} xf_table_config;
void xf_table_config_default(xf_table_config *cfg); /* reference defaults, FTRL, dim 1 */

int xf_table_create(xf_table **out, const xf_table_config *cfg); /* on current device */
int xf_table_destroy(xf_table *t);
int xf_table_size(xf_table *t, uint64_t *nkeys); /* synchronises */
int xf_table_capacity(xf_table *t, uint64_t *slots);
/* keys of the settled tier (sorted, key r owns state row r): what the last xf_table_defrag —
 * or the first-touch build of an empty table's first minibatch — left there; 0 before */
int xf_table_settled(xf_table *t, uint64_t *nkeys);
/* allocate now what xf_table_defrag would allocate (its second state buffer, both allocations of
 * the settled tier at the size the table's rows allow): for a caller whose clock is about to
 * start — a defrag then calls the driver's allocator no more.  Optional. */
int xf_table_prepare_defrag(xf_table *t);
/* grow to new_capacity slots (rehash on device); earlier slot arrays become invalid */
int xf_table_reserve(xf_table *t, uint64_t new_capacity);
/* renumber the state rows in key order (locality of the Pull gather and the Push pass once
 * the key set has settled); row numbers change — call it between steps.  The table keeps a
 * second state buffer of the same size from its first call on (the two swap roles: no
 * allocation, no clearing per call). */
int xf_table_defrag(xf_table *t);
/* which way the table's last xf_table_defrag call put the arrival index's keys in order
 * (read-only, for tests and profiles): XF_DEFRAG_NONE when it found nothing to move (or before
 * the first call); XF_DEFRAG_SORTFREE the index read front to back, block by block; the radix
 * sort of every key because xf_tune("key_build", 1) asked for it or the table is beyond 2^38
 * positions (_ASKED), because a block's last cluster ran on for more than 32768 positions
 * (_EXTENT), because the blocks' counts did not add up to the keys the index holds (_COUNT), or
 * because a cluster held more than 1024 keys (_CLUSTER) */
enum {
  XF_DEFRAG_NONE = 0,
  XF_DEFRAG_SORTFREE = 1,
  XF_DEFRAG_RADIX_ASKED = 2,
  XF_DEFRAG_RADIX_EXTENT = 3,
  XF_DEFRAG_RADIX_COUNT = 4,
  XF_DEFRAG_RADIX_CLUSTER = 5
};
int xf_table_defrag_path(xf_table *t, int *path);
/* Table eviction — the one call that lowers a table's key count.  FTRL tables of dim 1 only (LR's
 * w table); XF_EINVAL with a message for an SGD table, dim != 1, a negative or NaN n_below.
 * A row is dropped iff  w == 0.0f (either sign of zero)  and  n < n_below,  compared in fp32.
 * n is the row's accumulated sum of SQUARED gradients, in the units the step uses: the gradient
 * of a key is the minibatch MEAN of (pctr - label) over the rows that hold it (times the value,
 * with feature values), so one occurrence in a minibatch of R rows adds at most 1 / R^2 to n —
 * 4e-10 at R = 50000 — and a key seen in every row of T minibatches has n <= T.  n_below = +inf
 * drops every zero-weight row; 0 does nothing (*rows_seen = 0); a NaN n is kept; the reserved
 * key 2^64-1 is judged like any other.  FTRL holds w at exactly 0 while |z| <= lambda1, so the
 * dropped rows added +0 to every prediction: predictions right after the call equal those before
 * it bit for bit.  A dropped key that comes back is a first touch: (w, n, z) = (0, 0, 0).
 * The call settles the table first (xf_table_defrag), then marks and compacts on the GPU (two
 * kernels and a scan, xf_evict.hip).  *rows_seen: the keys judged; *rows_dropped: those that
 * went (either may be NULL).  Nothing dropped: row numbers and epoch as the defrag left them.
 * Otherwise row numbers change like a defrag's — call it between steps.  Everything dropped: the
 * table is as after xf_table_create (same capacity and hyper-parameters).  No row's value is
 * written, so xf_table_w_derived stays what it was. */
int xf_table_evict(xf_table *t, float n_below, uint64_t *rows_seen, uint64_t *rows_dropped);
/* {rows of one workgroup of the eviction kernels, lanes of a wavefront}: the edges for tests */
void xf_evict_shape(uint32_t out[2]);
int xf_table_set_hyper(xf_table *t, float alpha, float beta, float l1, float l2, float lr);

/* ps-lite-shaped host API: keys sorted & unique (the KVWorker contract), host pointers,
 * blocking (== Push/Pull followed by Wait).  Pull inserts missing keys (ftrl.h:56). */
int xf_table_pull(xf_table *t, const uint64_t *keys, size_t n, float *vals /* n*dim */);
int xf_table_push(xf_table *t, const uint64_t *keys, size_t n, const float *grads);

/* device-pointer API, asynchronous on `stream` (a hipStream_t; NULL = default stream).
 * resolve: key -> slot with insert-on-miss (+ first-touch init); keys of other shards
 * are an error.  gather: vals[i*dim+j] = w[slot[i]*dim+j].  update: one optimizer step
 * per (slot, j) — slots must be unique within one call. */
int xf_table_resolve_dev(xf_table *t, const uint64_t *d_keys, size_t n, uint32_t *d_slots,
                         void *stream);
int xf_table_gather_dev(xf_table *t, const uint32_t *d_slots, size_t n, float *d_vals,
                        void *stream);
/* resolve + gather in one pass (dim-1 tables, keys unique within the call) */
int xf_table_pull_dev(xf_table *t, const uint64_t *d_keys, size_t n, uint32_t *d_slots,
                      float *d_vals, void *stream);
/* The owner side of a step with N source ranks, in ONE pass over the shard instead of one per
 * source: d_keys_sorted = the concatenated per-source key lists in (stable) ascending key
 * order, d_order[i] = position of sorted entry i in the per-source layout.  Rows / weights
 * are written, gradients read, in the per-source layout.  A key that several sources sent gets
 * their optimizer steps one after the other in source order, as N separate
 * xf_table_update_dev passes in rank order would apply them. */
int xf_table_pull_ordered_dev(xf_table *t, const uint64_t *d_keys_sorted,
                              const uint32_t *d_order, size_t n, uint32_t *d_slots,
                              float *d_vals /* may be null: resolve only */, void *stream);
int xf_table_update_merged_dev(xf_table *t, const uint64_t *d_keys_sorted,
                               const uint32_t *d_order, size_t n, const uint32_t *d_slots,
                               const float *d_grads, void *stream);
int xf_table_update_dev(xf_table *t, const uint32_t *d_slots, size_t n,
                        const float *d_grads, void *stream);
/* raises XF_EFULL / XF_EINVAL recorded by earlier async calls; synchronises the stream */
int xf_table_check(xf_table *t, void *stream);

/* state dump sorted by key (parity hook / checkpoint).  n_/z_ may be NULL. */
int xf_table_export(xf_table *t, uint64_t *keys, float *w, float *n_, float *z_,
                    size_t cap_entries, size_t *n_out);
int xf_table_import(xf_table *t, const uint64_t *keys, size_t n, const float *w,
                    const float *n_, const float *z_);
/* *yes = 1: the LR gradient + Push kernels derive a key's old weight from the (n, z) they load
 * anyway instead of reading it — the w an FTRL step leaves is a function of the n and z it
 * leaves (ftrl.h:66-73), so the stored w is that function's value, bit for bit, as long as every
 * row was written by steps under the table's present hyper-parameters (or never: 0, 0, 0).
 * An FTRL table of dim 1 starts that way; it stops (for good: the kernels read w again) when
 * xf_table_import brings a row whose w is not the w of its (n, z) — checked row by row on the
 * GPU, a model file saved under the same hyper-parameters passes — or xf_table_set_hyper
 * changes alpha / beta / lambda1 / lambda2 with keys in the table.  Same table bits either way. */
int xf_table_w_derived(xf_table *t, int *yes);
/* *out = 1: the table has found its alpha an exact divisor — the double product with 1 / alpha,
 * rounded to float, is x / alpha for every finite x — and its FTRL steps divide without the
 * guard of the subnormal range (the verdict rides in the sign of the device's inv_alpha). */
int xf_table_div_exact(xf_table *t, int *out);
/* out[i] = the step's x[i] / d (the product with 1.0 / (double)d, with its guard of the subnormal
 * range or, exact != 0, without it), computed on the GPU; host arrays of n floats.  For tests. */
int xf_div_by_const_probe(const float *x, size_t n, float d, int exact, float *out);
/* The scalar layer under every forward and step (xf_device.h), the functions as the kernels call
 * them, computed on the GPU.  For tests (tests/test_gpu_scalar.py): each is compared with the
 * host on all 2^32 floats.
 *   XF_SCALAR_SIGMOID   sigmoid_ref(a)            XF_SCALAR_SQRT      sqrtf(a)
 *   XF_SCALAR_DIV       a / b in fp32             XF_SCALAR_DIV_ROWS  div_by_rows(a, param)
 * xf_scalar_probe: out[i] = op(a[i], b[i]); host arrays of n floats, b is read by XF_SCALAR_DIV
 * alone (NULL otherwise), param (the row count R >= 1) by XF_SCALAR_DIV_ROWS alone.
 * xf_scalar_sweep: every op but XF_SCALAR_DIV over whole blocks of inputs.  Block i is the 65536
 * floats with the bit patterns (i << 16) .. (i << 16) + 65535; digests[j] (host, nblocks of them)
 * is the wrapping sum over block first_block + j of
 *   mix64((uint64_t)bits(a) << 32 | canon(bits(op(a))))
 * with splitmix64's finaliser for mix64 and canon = every NaN to 0x7fc00000 (the sign and payload
 * of a NaN are the one thing two IEEE machines may disagree on).  first_block + nblocks <= 65536. */
enum { XF_SCALAR_SIGMOID = 0, XF_SCALAR_SQRT = 1, XF_SCALAR_DIV = 2, XF_SCALAR_DIV_ROWS = 3 };
int xf_scalar_probe(int op, const float *a, const float *b, uint32_t param, size_t n, float *out);
int xf_scalar_sweep(int op, uint32_t param, uint32_t first_block, uint32_t nblocks,
                    uint64_t *digests);

/* ---------------------------------------------------------------- model kernels       */
/* All pointers are device pointers; asynchronous on `stream`. */
/* LR forward (lr_worker.cc:121-143): loss[r] = sigmoid(sum w_u[uidx]) - label */
int xf_lr_forward_dev(const xf_dev_batch *b, const float *d_wu, float *d_loss,
                      float *d_pctr /* may be NULL */, void *stream);
/* LR gradient (lr_worker.cc:100-119): g[u] = (sum_{occurrences} loss[row]) / R */
int xf_lr_grad_dev(const xf_dev_batch *b, const float *d_loss, float *d_g, void *stream);
/* LR gradient fused with the Push for a table on the same GPU (single shard): g is still
 * written (parity hook); slots as returned by resolve/pull for b->ukeys; d_wu = the weights
 * that Pull returned, if nothing has touched those rows since (saves re-reading w), or NULL */
int xf_lr_grad_update_dev(xf_table *t, const xf_dev_batch *b, const uint32_t *d_slots,
                          const float *d_wu, const float *d_loss, float *d_g, void *stream);
/* FM forward, reference form (fm_worker.cc:159-202); v_u is U x k row-major */
int xf_fm_forward_dev(const xf_dev_batch *b, int k, const float *d_wu, const float *d_vu,
                      float *d_loss, float *d_pctr, float *d_vsum, void *stream);
/* FM gradient (fm_worker.cc:126-157): gw U, gv U x k */
int xf_fm_grad_dev(const xf_dev_batch *b, int k, const float *d_vu, const float *d_vsum,
                   const float *d_loss, float *d_gw, float *d_gv, void *stream);

/* FM gradient fused with the two Pushes (fm_worker.cc:241-242), both tables on this GPU */
int xf_fm_grad_update_dev(xf_table *w, xf_table *v, const xf_dev_batch *b,
                          const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                          const float *d_vu, const float *d_vsum, const float *d_loss,
                          float *d_gw, float *d_gv, void *stream);

/* ---------------------------------------------------------------- fused steps         */
typedef struct xf_workspace xf_workspace; /* per-stream scratch: slots, w_u, g, loss... */
int xf_workspace_create(xf_workspace **out);
int xf_workspace_destroy(xf_workspace *ws);
/* One LRWorker::update (lr_worker.cc:167-176) on a single-shard table, device-resident:
 * pull(resolve+gather) -> loss -> gradient -> push(update).  Asynchronous. */
int xf_lr_step(xf_table *w, xf_batch *b, xf_workspace *ws, void *stream);
/* The whole LRWorker::update (lr_worker.cc:145-177) on a fresh minibatch: xf_batch_compile_local_dev
 * + xf_lr_step in one call — same kernels, same results; the key build's one host wait (work
 * items of the gradient pass, keys the table does not hold yet) is taken while the forward
 * already runs.  *out (optional): the minibatch, for replays (xf_batch_free); with out == NULL
 * the call waits for the step and frees it. */
int xf_lr_update_dev(xf_batch **out, xf_table *w, const uint64_t *d_keys, const uint32_t *d_rowptr,
                     const int32_t *d_labels, uint32_t R, uint32_t NNZ, int retain_keys,
                     xf_workspace *ws, void *stream);
/* One FMWorker::update (fm_worker.cc:226-242).  For k in {4, 8, 16, 32, 64} the forward's
 * per-key records (sum_k v, sum_k v^2, w) are kept in an array next to v's state rows and are
 * rewritten by the step's gradient + Push kernel; a minibatch that is stepped again starts with
 * the forward.  Other writers of w or v (xf_table_push / _update* / _import, a defrag, a step
 * with capture or a parity mode on) are noticed through the tables' write counters: the
 * minibatch's records are rebuilt on its next step.  Per-key intermediates (xf_workspace_fetch
 * of w_u / g) exist only with xf_workspace_capture.  Environment: XF_FM_TABLE_RECORDS=0 turns
 * the records off (the step then gathers the factor rows before every forward). */
int xf_fm_step(xf_table *w, xf_table *v, xf_batch *b, xf_workspace *ws, void *stream);
/* forward only (calculate_pctr, lr_worker.cc:25-71 / fm_worker.cc:25-95): pulls (and so
 * inserts) the batch's keys, writes R probabilities to host `pctr_out`.  Blocking. */
int xf_lr_predict(xf_table *w, xf_batch *b, xf_workspace *ws, float *pctr_out);
int xf_fm_predict(xf_table *w, xf_table *v, xf_batch *b, xf_workspace *ws,
                  float *pctr_out);
/* parity hook of the LR / FM step: when enabled, the step also stores the pulled weights and the
 * gradients per unique key of the minibatch for xf_workspace_fetch (the production step never
 * forms them: the forward reads the table in place, the gradient is consumed where it is
 * summed).  Needs a minibatch with a key list (xf_batch_compile*). */
int xf_workspace_capture(xf_workspace *ws, int enable);
/* Parity mode of the forward (xf_lr_step / xf_fm_step / xf_*_predict with this workspace):
 *   XF_PARITY_EXACT_SUMS       (default) row sums accumulated in fp64 and rounded once
 *   XF_PARITY_REFERENCE_ORDER  fp32 running sums in the reference's own order (ascending fid,
 *                              lr_worker.cc:127-138; FM: k-outer pooled sums, fm_worker.cc:
 *                              166-192): the loss equals the reference arithmetic's bit for
 *                              bit.  One thread per example: a checking mode, ~100x slower.
 *                              Needs a minibatch with a key list (xf_batch_compile*). */
#define XF_PARITY_EXACT_SUMS 0
#define XF_PARITY_REFERENCE_ORDER 1
int xf_workspace_parity(xf_workspace *ws, int mode);
/* FM form of xf_fm_step / xf_fm_predict with this workspace:
 *   XF_FM_REFERENCE  (default) the reference's second-order term as written (fm_worker.cc:
 *                    178-196): sums pooled over all k factors, v_y = (sum a_u)^2 - sum b_u
 *   XF_FM_CANONICAL  Rendle's FM: per-factor sums S[r,f] = sum_j v[u_j,f],
 *                    y2 = 0.5 (sum_f S^2 - sum_f sum_j v^2) = sum_{i<j} <v_i, v_j>;
 *                    gw = (sum_occ loss) / R, gv[u,f] = (sum_occ loss (S[r,f] - v[u,f])) / R.
 *                    Exact fp64 sums of fp32 terms, as XF_PARITY_EXACT_SUMS.  Needs a minibatch
 *                    with a key list (xf_batch_compile / _gpu / _dev, not the keyed build of
 *                    xf_batch_compile_fm*); refused together with XF_PARITY_REFERENCE_ORDER.
 *   XF_FM_FIELD_AWARE  the field-aware FM (Juan et al.): a key keeps one k-vector per field, the
 *                    v table is F k wide (F = xf_workspace_fm_fields, set first; coordinate
 *                    (h, f) at h k + f) and a pair interacts through the vectors each holds for
 *                    the other's field.  Nonzero j: key u_j, field g_j, x_j (1 without values),
 *                    a_j[h,f] = v[u_j,h,f] x_j:
 *                      y2 = sum_{i<j} sum_f a_i[g_j,f] a_j[g_i,f]   (pairs of POSITIONS)
 *                      gw = (sum_occ loss x) / R
 *                      gv[u,h,f] = (sum_{occ i of u} sum_{j != i, g_j = h} loss x_i a_j[g_i,f]) / R
 *                    Exact fp64 sums of fp32 products.  Only TOUCHED coordinates of v are stepped
 *                    ((u, h): some occurrence of u has another nonzero of field h in its row);
 *                    the others keep w, n, z bit for bit — an FTRL step with g = 0 would zero a
 *                    fresh weight for good.  Needs a minibatch compiled with the same number of
 *                    fields (xf_batch_compile_fielded*) and a v table of dim F k <= 4096; refused
 *                    with XF_PARITY_REFERENCE_ORDER and with xf_workspace_capture (the step
 *                    leaves the pulled w and gw for xf_workspace_fetch as it is). */
#define XF_FM_REFERENCE 0
#define XF_FM_CANONICAL 1
#define XF_FM_FIELD_AWARE 2
int xf_workspace_fm_mode(xf_workspace *ws, int mode);
/* fields of XF_FM_FIELD_AWARE: 1 .. 64 (a key's touched fields are one 64-bit mask) */
int xf_workspace_fm_fields(xf_workspace *ws, int fields);
/* copies of the last step's intermediates to host (parity hook): any pointer may be NULL */
int xf_workspace_fetch(xf_workspace *ws, float *wu, float *loss, float *g, size_t U,
                       size_t R);
/* optional per-kernel timing with HIP events recorded on the step's own stream:
 * ms_sum[5] = resolve, gather, forward, gradient, update, summed over *steps steps.
 * xf_lr_step fuses gather into resolve and update into gradient: slots 1 and 4 read 0. */
int xf_workspace_profile(xf_workspace *ws, int enable);
int xf_workspace_profile_read(xf_workspace *ws, double *ms_sum, long *steps);
int xf_stream_sync(void *stream);
/* measurement support: stream `bytes` of scratch with a known access width, `repeat` times
 * (kind 0/1/2 = read 4/8/16 B per lane, 3/4/5 = write 4/8/16 B per lane): calibrates the
 * rocprofv3 FETCH_SIZE / WRITE_SIZE counters (tools/pmc_traffic.py) */
int xf_calib_stream(int kind, size_t bytes, int repeat); /* == ps KVWorker::Wait */

/* ---------------------------------------------------------------- process group       */
/* One process per GPU.  Replaces ps-lite's postoffice / van as xflow uses them (main.cc:22-47,
 * scripts/local.sh:3-14) and the transport under KVWorker::Push/Pull: the exchange steps of
 * the sharded table are all-to-all-v's over RCCL (grouped ncclSend/ncclRecv per peer over
 * xGMI, asynchronous on the caller's stream).  The bootstrap is a TCP star around rank 0
 * (ps-lite's scheduler): it carries the ncclUniqueId and the small host-side collectives.
 * XF_TRANSPORT_HOST stages the exchange through the bootstrap sockets (tests: several ranks on
 * one GPU, or none). */
#define XF_TRANSPORT_RCCL 0
#define XF_TRANSPORT_HOST 1
/* RCCL when it comes up on every rank (library, communicator and one all-to-all-v on the device
 * are checked collectively), otherwise the host transport with a warning on rank 0's stderr;
 * xf_group_info reports which one the group runs on */
#define XF_TRANSPORT_AUTO 2
typedef struct xf_group xf_group;
/* rank < 0 / world <= 0 / addr NULL / port <= 0: from the environment — WORLD_SIZE | XF_WORLD |
 * DMLC_NUM_WORKER; RANK | XF_RANK | DMLC_RANK (absent: ranks are handed out in arrival order,
 * the process that binds the port first is rank 0, as ps-lite's scheduler numbers its nodes);
 * MASTER_ADDR | DMLC_PS_ROOT_URI (127.0.0.1); MASTER_PORT | DMLC_PS_ROOT_PORT (29512).
 * Collective: returns when all `world` processes have joined.  device: this process's GPU —
 * >= 0 a device index, -1 the current device, -2 by rank (LOCAL_RANK, else rank modulo the
 * visible devices; ranks handed out on arrival are only known inside this call). */
int xf_group_create(xf_group **out, int rank, int world, const char *addr, int port,
                    int transport, int device);
int xf_group_destroy(xf_group *g);
/* Give up on the group's communicators (ncclCommAbort): work of theirs stuck on a stream — a
 * peer has died — ends; device exchanges fail with XF_EIO afterwards.  The sharded trainer calls
 * it when a stream wait exceeds XF_COLLECTIVE_TIMEOUT_S. */
int xf_group_abort(xf_group *g);
int xf_group_info(const xf_group *g, int *rank, int *world, int *transport);
int xf_group_barrier(xf_group *g);
/* host-side collectives over the bootstrap (small payloads: counts, flags, metrics) */
int xf_group_allgather_host(xf_group *g, const void *in, size_t bytes, void *out /* world x */);
int xf_group_gatherv_host(xf_group *g, const void *in, size_t bytes, void *out_rank0,
                          const uint64_t *sizes_rank0);
/* all-to-all-v: send[...] holds one slice per destination rank (send_counts[p] elements of
 * elem_bytes, in rank order), recv gets one slice per source rank.  RCCL: device pointers,
 * asynchronous on `stream`.  Host transport: blocking; host_buffers != 0 says the pointers are
 * host memory (no GPU involved at all). */
int xf_group_alltoallv(xf_group *g, const void *send, const uint64_t *send_counts, void *recv,
                       const uint64_t *recv_counts, size_t elem_bytes, int host_buffers,
                       void *stream);
/* The same on one of the group's XF_GROUP_CHANNELS communicators (xf_group_alltoallv = channel
 * 0).  RCCL serialises the work of one communicator and needs every rank to enqueue on it in
 * the same order: exchanges that a rank issues from two streams independently of each other
 * (the sharded trainer's stale1 schedule) take a channel per stream.  Every rank must use the
 * same channel for the same exchange. */
#define XF_GROUP_CHANNELS 2
int xf_group_alltoallv_ch(xf_group *g, int channel, const void *send,
                          const uint64_t *send_counts, void *recv, const uint64_t *recv_counts,
                          size_t elem_bytes, int host_buffers, void *stream);

/* COLLECTIVE diagnostic: both channels driven at the same time from two streams of every rank
 * (grouped send / recv of `bytes` bytes with every rank, this one included), results checked. */
int xf_group_selftest(xf_group *g, size_t bytes);

/* The hash of the sources this library was built from (xflow_amd/build.py: source_hash); the
 * Python binding refuses a library whose hash differs from the sources next to it. */
const char *xf_source_hash(void);

/* The sort at the top of the reference's key build (lr_worker.cc:146-166: all_keys[(fid, sid)],
 * std::sort by fid) as a device routine: d_sorted_keys = d_keys[0..n) ascending, d_sorted_pos =
 * their positions, ascending inside a key (what a stable sort gives).  [lo, lo + span] = where
 * the keys lie (0, UINT64_MAX: anywhere); n < 2^30.  Hand-written (*by_hand = 1): a partition by
 * uniform key range + a range sorted in LDS; a range beyond the LDS (a power-law head, keys that
 * are no hashes) is merged from sorted parts, a skewed stream's hot keys get ranges of their own.
 * The library's radix sort (*by_hand = 0) beyond 3.3e7 keys and under xf_tune("key_build", 1).
 * Waits for the stream. */
int xf_sort_key_pos(const uint64_t *d_keys, uint32_t n, uint64_t lo, uint64_t span,
                    uint64_t *d_sorted_keys, uint32_t *d_sorted_pos, void *stream, int *by_hand);

/* Diagnostic (tools/kb_timeline.py): wall_clock64 stamps of the phases of the last keyed build
 * made with xf_tune("exp_knob", 200) (a library built with -DXF_EXPERIMENTS; empty otherwise):
 * [histogram | scatter | resolve] workgroups x slots;
 * returns the slots per workgroup, shape[3] = workgroups per kernel. */
int xf_kb_debug_read(unsigned long long *out, size_t cap, uint32_t *shape);

/* ---------------------------------------------------------------- sharded trainer     */
/* LRWorker / FMWorker::update across the ranks of a group: the table sharded by key range
 * (ps-lite's default slicer), examples by worker, one all-to-all-v each way per step (weights
 * back to the workers, gradients to the owners; the keys travel once, when the minibatch is
 * compiled).  The owner applies the ranks' pushes of a step in rank order after all pulls.
 * With a group of one rank (or g == NULL) it is the fused single-shard step. */
#define XF_SCHEDULE_SEQUENTIAL 0 /* Pull, compute, Push of step t before Pull(t+1) */
#define XF_SCHEDULE_STALE1 1     /* Push(t) overlaps Pull/forward/gradient of t+1 (one step stale) */
/* LR and FM (FM: three fp64 row sums per row instead of one; (loss, v_sum) back; with
 * XF_UPDATE_RANK_ORDERED the owner keeps one minibatch per worker and forms every worker's
 * gradient from the rows that worker's Pull returned, with XF_UPDATE_SUM_THEN_STEP it runs one
 * fused gradient + Push pass over all workers' rows).
 * Owner-compute dataflow: a minibatch's NONZEROS go to the key owners once, when it is
 * compiled; a step then runs the table-resident forward and gradient + Push at the owners and
 * exchanges only row-level scalars (fp64 partial row sums to the rows' workers, their losses
 * back) instead of a weight and a gradient per key.  Same results as XF_SCHEDULE_SEQUENTIAL
 * (every worker's gradient its own optimizer step, applied in rank order). */
#define XF_SCHEDULE_OWNER 2
/* The owner-compute dataflow with the gradient + Pushes of step t on a second HIP stream under
 * the exchanges of step t+1 (north_star: "overlapped with the next batch's forward on a second
 * HIP stream"): forward(t+1) reads the table BEFORE the Pushes of step t land, they are applied
 * while the row sums and losses of step t+1 travel, and forward(t+2) waits for them — weights
 * exactly one step stale, deterministic (events order the table's reader and writer), inside
 * ps-lite's asynchronous semantics; the results of XF_SCHEDULE_STALE1.  Same compiled
 * minibatches as XF_SCHEDULE_OWNER (xf_sharded_set_schedule switches between the two).
 * FM: under XF_UPDATE_RANK_ORDERED (every worker's gradient from the rows ITS Pull returned,
 * fm_worker.cc:226-242) the workers' two Pushes are what runs one step late; the fused pass of
 * XF_UPDATE_SUM_THEN_STEP reads the factors where they live at Push time and is refused here. */
#define XF_SCHEDULE_OWNER_STALE1 3
typedef struct {
  int32_t model;     /* 0 LR, 1 FM */
  int32_t optimizer; /* XF_OPT_* */
  int32_t k;         /* FM factors */
  int32_t schedule;  /* XF_SCHEDULE_* */
  uint64_t capacity; /* index positions of THIS rank's shard */
  uint64_t seed;
  float alpha, beta, lambda1, lambda2, lr;
  int32_t host_key_build; /* != 0: the sorted-unique-key build on the host (xf_batch_compile) */
  /* How the owner applies the ranks' pushes of one step:
   *   XF_UPDATE_RANK_ORDERED  every worker's gradient (its sum / its R) is its own optimizer
   *                           step, applied in rank order — one legal ps-lite interleaving
   *   XF_UPDATE_SUM_THEN_STEP the workers' sums added, ONE step with 1 / (all rows): the result
   *                           of one update() on the concatenation of the ranks' minibatches,
   *                           whatever the number of GPUs (XF_SCHEDULE_OWNER / _OWNER_STALE1
   *                           only: there the sums meet exactly, in fp64) */
  int32_t update_rule;
} xf_sharded_config;
#define XF_UPDATE_RANK_ORDERED 0
#define XF_UPDATE_SUM_THEN_STEP 1
void xf_sharded_config_default(xf_sharded_config *cfg);
typedef struct xf_sharded xf_sharded;
typedef struct xf_sbatch xf_sbatch;
int xf_sharded_create(xf_sharded **out, xf_group *g, const xf_sharded_config *cfg);
int xf_sharded_destroy(xf_sharded *st);
/* COLLECTIVE (every rank, same order): key build + the static part of the exchange */
int xf_sharded_compile(xf_sharded *st, xf_sbatch **out, const uint64_t *rowptr,
                       const uint64_t *keys, const int32_t *labels, size_t row_begin,
                       size_t row_end, int keep);
/* The same from DEVICE-resident arrays: the raw keys in CSR order, 32-bit row offsets (R + 1),
 * labels.  On the owner-compute dataflow the worker's side is a stable partition by key owner
 * on the device and ONE host wait (for the per-owner counts, which travel through the group's
 * all-to-all).  The arrays may be released when the call returns.  COLLECTIVE.  Replaces the
 * key build + the Pull's routing of lr_worker.cc:146-170 for a minibatch that is already in
 * HBM (nothing in the reference: its blocks live in host vectors). */
int xf_sharded_compile_dev(xf_sharded *st, xf_sbatch **out, const uint64_t *d_keys,
                           const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                           uint32_t NNZ, int keep);
/* The same with feature values (xf_batch_compile_valued_gpu / _dev; the host build with
 * host_key_build): LR, and FM after xf_sharded_set_fm_mode(XF_FM_CANONICAL or _FIELD_AWARE).  One
 * rank: the fused step.  Several ranks (COLLECTIVE): the generic build, then the static part of
 * the weight / gradient exchange as xf_sharded_compile — on XF_SCHEDULE_SEQUENTIAL and
 * XF_SCHEDULE_STALE1; the owner-compute schedules exchange the reference form's pooled row sums
 * and refuse (XF_EINVAL, the message names the schedule).  No LR cells are built.  A minibatch of
 * zero rows compiles and steps: a rank without rows still serves the others' Pulls.
 * xf_sharded_step / _predict take the result as any other. */
int xf_sharded_compile_valued(xf_sharded *st, xf_sbatch **out, const uint64_t *rowptr,
                              const uint64_t *keys, const float *vals, const int32_t *labels,
                              size_t row_begin, size_t row_end, int keep);
int xf_sharded_compile_valued_dev(xf_sharded *st, xf_sbatch **out, const uint64_t *d_keys,
                                  const float *d_vals, const uint32_t *d_rowptr,
                                  const int32_t *d_labels, uint32_t R, uint32_t NNZ, int keep);
/* The same with the nonzeros' fields (xf_batch_compile_fielded / _gpu / _dev; vals / d_vals may
 * be NULL) for an FM trainer after xf_sharded_set_fm_fields +
 * xf_sharded_set_fm_mode(XF_FM_FIELD_AWARE); one rank or several, as xf_sharded_compile_valued
 * (whose rules the trainer obeys with feature values).  The fgid range check comes before any
 * exchange, and the ranks agree on its outcome: an fgid outside [0, fields) on ONE rank is
 * XF_EINVAL on EVERY rank (the offender's message names the fgid, the others' the rank), and no
 * rank is left waiting in a collective. */
int xf_sharded_compile_fielded(xf_sharded *st, xf_sbatch **out, const uint64_t *rowptr,
                               const uint64_t *keys, const int32_t *fgid, const float *vals,
                               const int32_t *labels, size_t row_begin, size_t row_end, int keep);
int xf_sharded_compile_fielded_dev(xf_sharded *st, xf_sbatch **out, const uint64_t *d_keys,
                                   const int32_t *d_fgid, const float *d_vals,
                                   const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                                   uint32_t NNZ, int keep);
int xf_sbatch_free(xf_sbatch *b);
int xf_sbatch_dims(const xf_sbatch *b, uint32_t *R, uint32_t *NNZ, uint32_t *U,
                   uint64_t *n_owned /* keys of this minibatch (all ranks) this rank owns */);
/* xf_batch_cells_info of a one-rank trainer's minibatch; XF_EINVAL when it has no cells over the
 * table's rows (a minibatch with a key list that was not stepped yet, any FM minibatch) — which
 * build a compile took, for tests and tools */
int xf_sbatch_cells_info(const xf_sbatch *b, uint32_t *out);
int xf_sbatch_fwd_info(const xf_sbatch *b, uint32_t *out); /* xf_batch_fwd_info, likewise */
/* 1 when the minibatch came from the FM build against the tables' settled tiers
 * (xf_batch_compile_fm: one shard, every key settled), else 0; < 0: error */
int xf_sbatch_fm_keyed(const xf_sbatch *b);
/* COLLECTIVE: one update() of every rank; asynchronous on the trainer's stream */
int xf_sharded_step(xf_sharded *st, xf_sbatch *b);
/* COLLECTIVE: forward only over this rank's rows (ranks without rows pass an empty minibatch) */
int xf_sharded_predict(xf_sharded *st, xf_sbatch *b, float *pctr_out);
int xf_sharded_flush(xf_sharded *st);  /* apply an outstanding stale1 Push; synchronises */
int xf_sharded_defrag(xf_sharded *st); /* local table maintenance (flushes first) */
/* xf_table_evict of this rank's shard of the w table (flushes first; local to the rank, no
 * communication): LR with FTRL, on one rank or on schedule=sequential / stale1.  Refused with a
 * message: an FM trainer, optimizer=sgd, the owner-compute schedules on several ranks.  The
 * minibatches compiled before it rebuild their row numbers from their keys at their next step. */
int xf_sharded_evict(xf_sharded *st, float n_below, uint64_t *seen, uint64_t *dropped);
int xf_sharded_check(xf_sharded *st);  /* flush + the tables' sticky errors */
int xf_sharded_set_schedule(xf_sharded *st, int schedule);
/* the parity mode of the forward (xf_workspace_parity) for a one-rank trainer whose minibatches
 * carry a key list (host_key_build, or FM).  Set it BEFORE compiling the minibatches it is to
 * apply to: an FM minibatch compiled in the default mode against the tables' settled tiers
 * (xf_sbatch_fm_keyed) has no index of its key list, and the reference-order kernels refuse it
 * (the call says so and names this remedy) */
int xf_sharded_set_parity(xf_sharded *st, int mode);
/* the FM form of an FM trainer (one rank: xf_workspace_fm_mode of its fused step; several: kept
 * in the trainer, which picks the forward, the emitting gradient kernels and — field-aware — the
 * masked owner push by it), accepted only while its tables hold no key.  XF_FM_CANONICAL also starts an SGD v table from the hash-normal init (a constant
 * init would keep a key's k factors equal forever), and minibatches compiled from then on carry
 * a key list (xf_batch_compile_gpu / _dev).  Several ranks (or XF_SHARDED_GENERAL=1): on
 * XF_SCHEDULE_SEQUENTIAL and XF_SCHEDULE_STALE1, any world size, both optimizers; on the
 * owner-compute schedules (and so with XF_UPDATE_SUM_THEN_STEP): XF_EINVAL naming the schedule.
 * XF_FM_FIELD_AWARE needs xf_sharded_set_fm_fields first; the trainer's k (xf_sharded_config) is
 * then the WIDTH of a v row, fields x (factors per field), at most 4096; the v table starts
 * hash-normal for both optimizers, and minibatches come from xf_sharded_compile_fielded*. */
int xf_sharded_set_fm_mode(xf_sharded *st, int mode);
int xf_sharded_set_fm_fields(xf_sharded *st, int fields);
int xf_sharded_tables(xf_sharded *st, xf_table **w, xf_table **v);
int xf_sharded_stream(xf_sharded *st, void **stream);
/* ms_sum[6] = owner pull, weights exchange, forward, gradient, gradients exchange, owner
 * update (HIP events on the step's stream; sequential schedule) */
int xf_sharded_profile(xf_sharded *st, int enable);
int xf_sharded_profile_read(xf_sharded *st, double *ms_sum, long *steps);
/* Checkpoint of the sharded table (the reference never saves its model): every rank writes
 * <prefix>.shard-RRRRR-of-NNNNN (key-sorted (key, w, n, z) of its shard), rank 0 also
 * <prefix>.manifest.  Load reads the shards of ANY saved world size (or a single-GPU model
 * file saved by XFSaveModel) and keeps the keys this rank owns.  Both COLLECTIVE. */
int xf_sharded_save(xf_sharded *st, const char *prefix);
int xf_sharded_load(xf_sharded *st, const char *prefix);

/* ---------------------------------------------------------------- feature admission    */
/* A counting Bloom filter ahead of the key build (not in the reference; the FTRL paper's "Bloom
 * filter inclusion"): a key enters the model only once the filter has seen it `count` times.  It
 * filters a minibatch's CSR arrays: a nonzero whose key is not admitted is taken out of its row,
 * the row keeps its label and its other nonzeros, and the result goes to any *_dev compile.
 * State: 2^log2_slots saturating 8-bit counters in HBM, zero at creation; log2_slots in 2 .. 32,
 * hashes in 1 .. 8, count in 1 .. 255.  slot_j(key) = mix64(key ^ mix64(seed + j)) >>
 * (64 - log2_slots), j = 0 .. hashes - 1, mix64 = x += 0x9e3779b97f4a7c15, then the splitmix64
 * finaliser (xf_admit_slot: 0 for a log2_slots or j outside the ranges).
 * One apply = one minibatch, two phases.  Count (update != 0 only): every nonzero adds 1 to each
 * of its `hashes` counters, saturating at `count`: c[s] = min(count, c_old[s] + #{(nonzero, j):
 * slot_j(key) = s}) — two j of one key on one slot count twice per occurrence; independent of
 * order.  Test and compact (after the whole count): a nonzero is kept iff all its counters equal
 * `count`; kept nonzeros keep their order, rowptr is rebuilt, fgid / vals (may be NULL) are
 * compacted with the keys.  update == 0 (predict) only reads the counters.  count = 1 with update
 * keeps everything: the outputs equal the inputs byte for byte.
 * xf_admit_apply_dev: device arrays (d_rowptr row-relative u32, R + 1).  The outputs are device
 * arrays owned by the filter, valid until its next apply (NULL for fgid / vals that were not
 * given); *NNZ_out = kept nonzeros.  Waits for the stream.  R = 0 and NNZ = 0 are valid.
 * xf_admit_apply: the reader's host arrays and a row slice (as xf_batch_compile_gpu): uploads the
 * slice (rowptr rebased to u32; labels, when given, to *d_labels_out unchanged) and runs the same
 * kernels — there is one implementation, the device one.
 * xf_admit_export / _import: the 2^log2_slots counters as bytes.  xf_admit_save / _load: a file
 * whose header carries the four parameters; a load into a filter with other parameters is
 * XF_EINVAL naming both sets, a missing or damaged file XF_EIO naming the path.
 * xf_admit_stats: nonzeros seen / kept, summed over the update != 0 applies.
 *
 * One filter shared by the ranks of a group (xf_admit_create_shared, COLLECTIVE; g == NULL: a
 * plain filter; a group of one computes what a plain filter computes, through the routed kernels
 * — which is how tools/admit_leg.py times them without a transport): the same logical state, the counters sharded by slot range — per = 4 *
 * ceil(ceil(2^log2_slots / world) / 4) slots a rank, rank r owns [r * per, min((r + 1) * per,
 * 2^log2_slots)), possibly nothing (xf_admit_range, host code; xf_admit_range_of: this filter's).
 * xf_admit_apply_dev / _apply are COLLECTIVE on it (R = 0 / NNZ = 0 is a normal participant): the
 * minibatches that the ranks hand in at the same call are counted together — c[s] = min(count,
 * c_old[s] + the occurrences over ALL ranks' nonzeros) — and after the whole count every rank
 * filters its own minibatch.  The counters equal those of a one-worker filter applied to the
 * concatenation of the ranks' minibatches, rank r's output is what that filter keeps of r's
 * arrays: nothing depends on the world size.  Every rank passes the same `update`; differing
 * flags, or a rank whose arguments are refused, are XF_EINVAL naming the rank on EVERY rank, before
 * any exchange.  The slots travel by the group's all-to-all-v on the caller's stream, channel 0
 * (4 bytes out, 1 byte back per nonzero and hash); NNZ * hashes must stay below 2^32, world at
 * most 256.  xf_admit_export / _import move this rank's range; xf_admit_save (COLLECTIVE: rank 0
 * gathers the ranges over the bootstrap and writes) and xf_admit_load (COLLECTIVE: every rank
 * reads its own range) use the one-worker file unchanged, so a file moves between world sizes.
 * xf_admit_stats stays per rank. */
typedef struct xf_admit xf_admit;
uint64_t xf_admit_slot(uint64_t key, uint64_t seed, int log2_slots, int j);
int xf_admit_range(int log2_slots, int world, int rank, uint64_t *first, uint64_t *n);
int xf_admit_create_shared(xf_admit **out, xf_group *g, int log2_slots, int hashes, int count,
                           uint64_t seed);
int xf_admit_range_of(const xf_admit *a, uint64_t *first, uint64_t *n);
int xf_admit_create(xf_admit **out, int log2_slots, int hashes, int count, uint64_t seed);
int xf_admit_destroy(xf_admit *a);
int xf_admit_params(const xf_admit *a, int *log2_slots, int *hashes, int *count, uint64_t *seed);
int xf_admit_apply_dev(xf_admit *a, int update, const uint64_t *d_keys, const int32_t *d_fgid,
                       const float *d_vals, const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ,
                       void *stream, const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                       const float **d_vals_out, const uint32_t **d_rowptr_out,
                       uint32_t *NNZ_out);
int xf_admit_apply(xf_admit *a, int update, const uint64_t *rowptr, const uint64_t *keys,
                   const int32_t *fgid, const float *vals, const int32_t *labels,
                   size_t row_begin, size_t row_end, void *stream, const uint64_t **d_keys_out,
                   const int32_t **d_fgid_out, const float **d_vals_out,
                   const uint32_t **d_rowptr_out, const int32_t **d_labels_out, uint32_t *R_out,
                   uint32_t *NNZ_out);
int xf_admit_export(xf_admit *a, uint8_t *counters);
int xf_admit_import(xf_admit *a, const uint8_t *counters);
int xf_admit_save(xf_admit *a, const char *path);
int xf_admit_load(xf_admit *a, const char *path);
int xf_admit_stats(const xf_admit *a, uint64_t *nonzeros_seen, uint64_t *nonzeros_kept);

/* ---------------------------------------------------------------- negative subsampling */
/* Subsampling of the negatives with importance weights (not in the reference; the FTRL paper's
 * "Subsampling Training Data"): every positive row is kept, a negative row with probability
 * `keep`, and a kept negative's loss — hence its gradient — is multiplied by w = 1 / keep, so the
 * expected gradient is unchanged.  Like admission it filters a minibatch's CSR arrays ahead of any
 * key build, but it drops whole rows and keeps no state.
 * Sampling.  keep: a float in (0, 1]; seed; a 64-bit stream id per apply; a 64-bit ordinal per row.
 *   T = (uint64) floor((double)keep * 2^32)
 *   h(ordinal) = mix64(mix64(seed ^ stream) + ordinal), mix64 as for admission (64-bit wrapping)
 *   a row is kept iff label != 0 or (h >> 32) < T
 * and on nothing else: not the keys, the block boundaries, the ingest path or the launch shape.
 * xf_negsample_keep is that decision for a negative row as host code (0 or 1; 0 for a keep
 * outside (0, 1]), from the one definition the kernels use.
 * One apply = one minibatch: row i of the input has ordinal first_ordinal + i; kept rows keep their
 * order; rowptr (u32, row-relative), labels, keys and fgid / vals (may be NULL) are compacted
 * together.  R = 0 is valid, NNZ = 0 with R > 0 is valid, rows without nonzeros are kept or
 * dropped like any other row.  keep = 1 returns the inputs byte for byte.
 * xf_negsample_apply_dev: device arrays (d_rowptr R + 1 offsets, d_labels R).  The outputs are
 * device arrays owned by the sampler, valid until its next apply (NULL for fgid / vals that were
 * not given), written in the order of `stream`; *R_out / *NNZ_out: kept rows and their nonzeros.
 * One wait for the stream, for those two counts (none with R = 0).
 * xf_negsample_apply: the reader's host arrays and a row slice: uploads the slice (rowptr rebased
 * to u32) and runs the same kernels — one implementation, the device one.
 * xf_negsample_stats, summed over the applies: rows seen, rows kept, negatives seen, negatives
 * kept.  The sampler allocates on the device only in its first apply.
 * Weight.  xf_negsample_weight: w = fp32(1) / fp32(keep), one fp32 division on the host.  A trainer
 * takes w >= 1 through xf_workspace_neg_weight / xf_sharded_set_neg_weight (default 1).  In every
 * training step (xf_lr_step — cells, local, valued, local valued — and xf_lr_update_dev after its
 * LAST forward segment; xf_fm_step in the reference form with and without table-resident records,
 * canonical and field-aware, with and without values; xf_sharded_step on XF_SCHEDULE_SEQUENTIAL and
 * XF_SCHEDULE_STALE1), after the forward has written the rows' losses and before anything reads
 * them:  loss[r] = labels[r] != 0 ? loss[r] : fp32(w * loss[r])  — one fp32 multiply, contraction
 * off.  Everything downstream is as before: the gradient, 1 / R with R the rows of the minibatch as
 * compiled (the kept rows), the optimizer step; xf_workspace_fetch returns the weighted loss.
 * Predict never weights.  With w == 1 no kernel is launched: the step is launch for launch what it
 * was.  With w != 1 the LR steps on cells (xf_lr_step on a cells, local or local valued minibatch,
 * xf_lr_update_dev) store the weighted loss from the kernel that forms the loss; every other step
 * launches one small kernel for it (xf_weigh_negatives_launches counts those).
 * XF_EINVAL: w < 1 or not finite; xf_sharded_set_neg_weight with w != 1 on a several-rank
 * trainer on XF_SCHEDULE_OWNER / _OWNER_STALE1 (the loss is formed inside the owners' finalize
 * kernels), and xf_sharded_set_schedule to one of those two while w != 1. */
typedef struct xf_negsample xf_negsample;
int xf_negsample_create(xf_negsample **out, float keep, uint64_t seed);
int xf_negsample_destroy(xf_negsample *s);
int xf_negsample_params(const xf_negsample *s, float *keep, uint64_t *seed);
int xf_negsample_weight(const xf_negsample *s, float *weight);
int xf_negsample_keep(uint64_t seed, uint64_t stream, uint64_t ordinal, float keep);
int xf_negsample_apply_dev(xf_negsample *s, uint64_t stream_id, uint64_t first_ordinal,
                           const uint64_t *d_keys, const int32_t *d_fgid, const float *d_vals,
                           const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                           uint32_t NNZ, void *stream, const uint64_t **d_keys_out,
                           const int32_t **d_fgid_out, const float **d_vals_out,
                           const uint32_t **d_rowptr_out, const int32_t **d_labels_out,
                           uint32_t *R_out, uint32_t *NNZ_out);
int xf_negsample_apply(xf_negsample *s, uint64_t stream_id, uint64_t first_ordinal,
                       const uint64_t *rowptr, const uint64_t *keys, const int32_t *fgid,
                       const float *vals, const int32_t *labels, size_t row_begin, size_t row_end,
                       void *stream, const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                       const float **d_vals_out, const uint32_t **d_rowptr_out,
                       const int32_t **d_labels_out, uint32_t *R_out, uint32_t *NNZ_out);
int xf_negsample_stats(const xf_negsample *s, uint64_t *rows_seen, uint64_t *rows_kept,
                       uint64_t *neg_seen, uint64_t *neg_kept);
int xf_workspace_neg_weight(xf_workspace *ws, float weight);
/* launches of the separate weight kernel since the library was loaded: the LR steps on cells form
 * the weighted loss in the kernel that forms the loss and make none */
uint64_t xf_weigh_negatives_launches(void);
/* launches of the LR gradient (+ Push) kernels since the library was loaded, per kind — which
 * kernel a step chose is otherwise invisible (read-only, for tests): out[0] k_lr_grad_dense with
 * byte-masked stores, [1] k_lr_grad_dense with whole-line stores, [2] k_lr_grad_dense deriving
 * the old weight from (n, z) (each of those also counted in [0] or [1]), [3] the one-source
 * k_lr_grad_cells, [4] k_lr_grad_split_finish.  Host-side counters: nothing runs on the device. */
void xf_lr_grad_launches(uint64_t out[5]);
/* the kernel that forms the LR cells steps' losses, on partial row sums the caller holds (device
 * arrays): d_partial[(v * G + g) * W + i] is workgroup g's share of row v * W + i; loss[r] =
 * sigmoid(fp32(sum over g)) - label, weighted as above, pctr[r] the sigmoid (either may be NULL).
 * The forward makes G a multiple of 8; this entry takes any R, W, G (the tests' way in). */
int xf_cells_finalize_rows(const double *d_partial, const int32_t *d_labels, uint32_t R, uint32_t W,
                           uint32_t G, float neg_weight, float *d_loss, float *d_pctr,
                           void *stream);
int xf_sharded_set_neg_weight(xf_sharded *st, float weight);

/* ---------------------------------------------------------------- progressive validation */
/* The loss of every training row under the weights it met BEFORE it was trained on (the FTRL
 * paper's progressive validation; not in the reference): in the first epoch a held-out metric that
 * needs no second file, later the training curve.  The device only counts; every floating-point
 * figure is formed on the host in fp64 from the counts, so the device's result depends on nothing
 * but the rows' losses and labels and is compared with ==.
 * Rank.  loss[r] = sigmoid - label as a training step forms it; pos = labels[r] != 0;
 * q = |loss[r]| is the probability put on the wrong class (p for a negative, fl(1 - p) for a
 * positive).  SH = 23 - XF_PROGRESS_MANT, C = bits(0.5f) >> SH:
 *   q <  0.5f: rank = bits(q) >> SH                     (-0.0 ranks as 0)
 *   q >= 0.5f: rank = 2C - (bits(1.0f - q) >> SH)       (the subtraction is exact; q = 1: 2C)
 * XF_PROGRESS_RANKS = 2C + 1 ranks, monotone in q, rank(1 - q) = 2C - rank(q) wherever 1 - q is
 * exact: a positive's SCORE rank is 2C - rank, a negative's is rank, and equal p means equal score
 * rank.  A row whose loss is NaN or whose q > 1 has rank XF_PROGRESS_RANKS and is counted in
 * other[pos] alone.  xf_progress_rank is that function as host code, from the one definition the
 * kernel uses.
 * Counts.  counts[2][XF_PROGRESS_RANKS] (class 0 = label 0 first; indexed by the rank of q) and
 * other[2], 64-bit, on the device, summed over as many accumulates as the caller likes.
 * xf_progress_accumulate_dev: R rows of device arrays, one launch on `stream` (none with R = 0), no
 * wait.  xf_progress_read: copies the counts out in the order of the stream of the last accumulate,
 * zeroes them when reset != 0, and waits for that stream — the one wait.  xf_progress_launches: the
 * accumulate launches since the library was loaded.  xf_progress_shape: {rows of a workgroup, slots
 * and probes of its LDS table} of the kernel, for the tests that reach its overflow path.
 * Summary (host, no GPU): a negative row weighs w = neg_weight (>= 1, finite), a positive 1, so
 * the figures estimate the unsampled stream under negative subsampling.  A bucket's representative
 * m is the midpoint of its fp32 bounds — of q below C, of 1 - q above; 0.5 at C; 2^-25 in the
 * saturated bucket 2C — its row term -log1p(-m) below C and -ln(m) from C on.  Sums run per class
 * by ascending rank, sum += (double)count * term.
 *   rows_pos = P, rows_neg = w N, saturated, other (weighted rows)
 *   logloss = (sum_pos + w sum_neg) / (P + w N), natural log; logloss_bound = -ln(1 - 2^-(MANT+1))
 *     bounds its distance from the fp64 mean of -log1p(-q) over the rows outside bucket 2C
 *   auc = fl(U2) / fl(2 P N), U2 = sum over score ranks b of pos_b (2 neg_below_b + neg_b) in exact
 *     integers; auc_slack = fl(sum_b pos_b neg_b) / fl(2 P N): the exact tie-aware AUC of the rows'
 *     p lies within auc +- auc_slack.  w cancels.
 *   ctr = P / (P + w N); pctr = the weighted mean of the buckets' representative p
 * One class only: auc is NaN and nothing else is.  No rows: every mean is NaN; the call succeeds.
 * Tap.  xf_workspace_progress(ws, p) attaches a progress to a workspace (NULL: off, the default;
 * the caller keeps p alive).  Every training step then accumulates its losses after the forward has
 * written them and before the negatives' weight touches them — the places the weight names above.
 * The LR steps on cells with w != 1 then finalize with weight 1, accumulate, and launch the weight
 * kernel (same expression, same bits); at w = 1 they finalize as before and accumulate.  Predict
 * never accumulates.  With nothing attached a step is launch for launch what it was; with one
 * attached its tables and outputs are bit for bit the same.
 * xf_sharded_progress(st, enable): the trainer owns one (created at 1, freed at 0).  XF_EINVAL on a
 * several-rank trainer on XF_SCHEDULE_OWNER / _OWNER_STALE1 (the loss is formed inside the owners'
 * finalize kernels), and xf_sharded_set_schedule to one of those two while it is on.
 * xf_sharded_progress_read: flushes, then reads this rank's counts; merged != 0: COLLECTIVE, the
 * ranks' counts summed (xf_group_allgather_host), the sum on every rank.
 * xf_sharded_last_loss: the losses (weighted) the last step of minibatch b left, R of them, for the
 * tests (flushes). */
#define XF_PROGRESS_MANT 10
#define XF_PROGRESS_RANKS 258049u
typedef struct xf_progress xf_progress;
typedef struct {
  double rows_pos, rows_neg, saturated, other;
  double logloss, logloss_bound, auc, auc_slack, ctr, pctr;
} xf_progress_metrics;
int xf_progress_create(xf_progress **out);
int xf_progress_destroy(xf_progress *p);
uint32_t xf_progress_rank(float loss);
int xf_progress_accumulate_dev(xf_progress *p, const float *d_loss, const int32_t *d_labels,
                               uint32_t R, void *stream);
int xf_progress_read(xf_progress *p, uint64_t *counts, uint64_t *other, int reset);
uint64_t xf_progress_launches(void);
void xf_progress_shape(uint32_t out[3]);
int xf_progress_summary(const uint64_t *counts, const uint64_t *other, float neg_weight,
                        xf_progress_metrics *out);
int xf_workspace_progress(xf_workspace *ws, xf_progress *p);
int xf_sharded_progress(xf_sharded *st, int enable);
int xf_sharded_progress_read(xf_sharded *st, uint64_t *counts, uint64_t *other, int reset,
                             int merged);
int xf_sharded_last_loss(xf_sharded *st, xf_sbatch *b, float *loss, size_t R);

/* ---------------------------------------------------------------- sliced progressive validation */
/* Progressive validation's figures per value of ONE field (per site, advertiser, slot ...; the
 * FTRL paper's metrics by slice; not in the reference): where is the model miscalibrated, which
 * slice carries the loss.  A stage names every row's slice, a device table adds per slice.  The
 * device only adds integers, so its result depends on nothing but the rows' losses, labels and
 * ids and is compared with ==; every floating-point figure is formed on the host.
 * Slice id.  id[r] = the key of the lowest-position nonzero of row r whose fgid == F;
 * XF_SLICE_NONE = UINT64_MAX for a row without one.  A real key equal to that value is counted
 * with `none` (one key in 2^64).  A row whose offsets descend or leave the arrays counts as empty,
 * as in the other stages.  The id depends on nothing else: not the ingest path, the launch shape
 * or the block boundaries.
 * xf_slices_extract_dev: device arrays (d_rowptr row-relative u32, R + 1; d_keys, d_fgid NNZ), one
 * launch on `stream` (none with R = 0), no wait; *d_id_out: R ids in a device array owned by the
 * object, valid until its next extract.  The inputs pass through unchanged.  xf_slices_extract: the
 * reader's host arrays and a row slice, uploaded (rowptr rebased to u32) as xf_cross_apply does —
 * one implementation, the device one.
 * Counters.  XF_SLICE_WORDS = 7 64-bit words a slice: n[2], qsum[2], llsum[2] (class 0 = label 0
 * first) and other.  With rank = xf_progress_rank(loss), cls = (label != 0), q = |loss|:
 *   rank == XF_PROGRESS_RANKS (NaN, q > 1): other += 1, nothing else
 *   otherwise: n[cls] += 1; qsum[cls] += (uint32)(q * 2^31) — an fp32 multiply by a power of two
 *   and a truncating conversion, exact; llsum[cls] += ll_fix[rank]
 *   ll_fix[rank] = (uint32) llrint(term(rank) * 2^24), term the row term xf_progress_summary gives
 *   that rank (one definition, shared).  The library builds the XF_PROGRESS_RANKS words once per
 *   object and uploads them (1 MB); xf_slices_terms exports them (host code).
 * Table.  Open-addressed, 2^b entries of (key, 7 words) = 64 bytes, b in 2 .. 26, empty =
 * UINT64_MAX.  Home slot xf_slices_home(key, b) = mix64(key) >> (64 - b), mix64 as for admission
 * (one definition for host and device; 0 for b outside 2 .. 26); linear probing with wrap, probe
 * limit min(2^b, 128).  One `none` entry and one `overflow` entry sit beside the table: a row whose
 * key finds neither itself nor an empty slot within the limit is counted in `overflow`.  Always:
 * the sum of every entry, `none` and `overflow` equals the counters of the whole stream, and a
 * resident key's counters are exactly that key's.  Per-slice figures are complete exactly when
 * `overflow` is all zero.  The table does not grow and is not rehashed.
 * xf_slices_accumulate_dev: R rows of device arrays, one launch on `stream` (none with R = 0), no
 * wait.  xf_slices_read: compacts the occupied entries on the device in the order of the stream of
 * the last accumulate and copies out up to `cap` of them — 8 words each: the key, then the seven —
 * sorted by key ascending, with *n = the occupied entries and none[7] / overflow[7] (either may be
 * NULL); one wait.  entries == NULL: only *n, none and overflow (reset must be 0).  *n > cap:
 * XF_EINVAL, nothing reset.  reset != 0: the table is emptied after the copy (a second wait).
 * xf_slices_launches: the accumulate launches since the library was loaded.  xf_slices_shape:
 * {rows of an accumulate workgroup, entries and probes of its LDS table, the global probe limit's
 * cap, rows of an extract workgroup}, for the tests that aim at the edges.
 * Summary (host, no GPU), per slice in fp64, w the weight of a negative as in xf_progress_summary:
 *   rows    = n1 + w n0
 *   ctr     = n1 / rows
 *   pctr    = ((n1 2^31 - qsum1) + w qsum0) / 2^31 / rows     (n1 2^31 - qsum1 in exact integers)
 *   logloss = (llsum1 + w llsum0) / 2^24 / rows
 *   other   = other (rows, unweighted: they have no class)
 * logloss lies within logloss_bound = progress's bound + 2^-25 (the rounding of a fixed-point
 * term) of the fp64 mean of -log1p(-q) over the slice's rows outside the saturated bucket; pctr
 * within pctr_bound = 2^-31 (the truncation, a row) of the weighted mean of the rows' p.  No rows:
 * every mean is NaN; the call succeeds.  Per-slice AUC is out of scope.
 * Tap.  xf_workspace_slices(ws, s) attaches a slices object to a workspace (NULL: off, the
 * default; the caller keeps s alive); xf_workspace_slice_ids(ws, d_id, R) names the ids of the
 * NEXT training step's rows (a device array the caller keeps alive until that step has run; row r
 * of the minibatch as it was compiled).  The step accumulates right after progressive
 * validation's accumulate, on the same unweighted losses, and forgets the ids; a step without ids
 * accumulates nothing, as does one whose R differs from the ids' (XF_EINVAL naming both).  Needs a
 * progress attached (XF_EINVAL otherwise, at the step).  With nothing attached a step is launch
 * for launch what it was; with one attached its tables and outputs are bit for bit the same.
 * xf_sharded_slices(st, enable, F, b): the trainer owns one (created at 1, freed at 0); needs
 * xf_sharded_progress on, and inherits its refusals: XF_EINVAL on a several-rank trainer on
 * XF_SCHEDULE_OWNER / _OWNER_STALE1.  xf_sbatch_set_slices(b, d_id, R) copies the ids of this
 * rank's R rows, in the order of the trainer's stream, into memory the minibatch owns, so a cached
 * minibatch replays with its ids (NULL: none); a step on a minibatch without ids counts no slice.
 * Every step path hands the tap its labels in the minibatch's row order, the order of the ids.
 * Several ranks: each rank counts its own rows.  xf_sharded_slices_read: flushes, then as
 * xf_slices_read on this rank's table; merged != 0: COLLECTIVE, every rank's compacted entries to
 * every rank (xf_group_allgather_host), merged by key — the same list on every rank, which may be
 * longer than one table — with none and overflow summed; reset empties this rank's table. */
#define XF_SLICE_NONE 0xFFFFFFFFFFFFFFFFull
#define XF_SLICE_WORDS 7
typedef struct xf_slices xf_slices;
typedef struct {
  double rows, other, ctr, pctr, logloss, logloss_bound, pctr_bound;
} xf_slice_metrics;
uint64_t xf_slices_home(uint64_t key, int log2_slots);
int xf_slices_terms(uint32_t *out);
int xf_slices_check(int64_t field, int64_t log2_slots);
int xf_slices_summary(const uint64_t *words, float neg_weight, xf_slice_metrics *out);
int xf_slices_create(xf_slices **out, int32_t field, int log2_slots);
int xf_slices_destroy(xf_slices *s);
int xf_slices_params(const xf_slices *s, int32_t *field, int *log2_slots);
int xf_slices_extract_dev(xf_slices *s, const uint64_t *d_keys, const int32_t *d_fgid,
                          const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ, void *stream,
                          const uint64_t **d_id_out);
int xf_slices_extract(xf_slices *s, const uint64_t *rowptr, const uint64_t *keys,
                      const int32_t *fgid, size_t row_begin, size_t row_end, void *stream,
                      const uint64_t **d_id_out, uint32_t *R_out);
int xf_slices_accumulate_dev(xf_slices *s, const float *d_loss, const int32_t *d_labels,
                             const uint64_t *d_id, uint32_t R, void *stream);
int xf_slices_read(xf_slices *s, uint64_t *entries, uint64_t cap, uint64_t *n, uint64_t *none,
                   uint64_t *overflow, int reset);
uint64_t xf_slices_launches(void);
void xf_slices_shape(uint32_t out[5]);
int xf_workspace_slices(xf_workspace *ws, xf_slices *s);
int xf_workspace_slice_ids(xf_workspace *ws, const uint64_t *d_id, uint32_t R);
int xf_sharded_slices(xf_sharded *st, int enable, int32_t field, int log2_slots);
int xf_sbatch_set_slices(xf_sbatch *b, const uint64_t *d_id, uint32_t R);
int xf_sharded_slices_read(xf_sharded *st, uint64_t *entries, uint64_t cap, uint64_t *n,
                           uint64_t *none, uint64_t *overflow, int reset, int merged);

/* ---------------------------------------------------------------- held-out validation  */
/* A fixed, hash-chosen share of the training rows taken out of training, and a forward-only pass
 * that counts their losses (not in the reference): a held-out figure per epoch that needs no second
 * file.  Progressive validation is held out in the first epoch only; this is held out in every one.
 * Split.  share: a float in [0, 1); seed; a 64-bit stream id per split; a 64-bit ordinal per row.
 *   T = (uint64) floor((double)share * 2^32)
 *   h(ordinal) = mix64(mix64(seed ^ stream ^ XF_HOLDOUT_SALT) + ordinal), mix64 as for admission
 *     (64-bit wrapping); the salt makes the decision independent of xf_negsample_keep's on the same
 *     seed and stream
 *   a row is HELD iff (h >> 32) < T
 * and on nothing else: not the label, the keys, the block boundaries, the ingest path or the launch
 * shape.  xf_holdout_held is that decision as host code (0 or 1; 0 for a share outside [0, 1)),
 * from the one definition the kernels use.
 * One split = one minibatch: row i of the input has ordinal first_ordinal + i; the rows go, in
 * order (stable), into two compacted minibatches, *train and *held, each with its own row-relative
 * u32 rowptr (R + 1 offsets), its labels, keys and fgid / vals (NULL when not given).  R = 0,
 * NNZ = 0 and rows without nonzeros are ordinary inputs; a part without rows has R = 0 and the one
 * zero offset.  A row whose offsets descend or leave the arrays counts as empty, as in the other
 * stages; nothing is read or written out of bounds.  XF_EINVAL when the rows' lengths sum past NNZ
 * (rows that overlap).
 * xf_holdout_split_dev: device arrays.  The parts are device arrays owned by the object, valid
 * until its next split, written in the order of `stream`; both parts share one set of arrays, the
 * held part at a 256-byte boundary behind the train part.  One wait for the stream, for the counts
 * (none with R = 0).
 * xf_holdout_split: the reader's host arrays and a row slice: uploads the slice (rowptr rebased to
 * u32) and runs the same kernels — one implementation, the device one.
 * xf_holdout_stats, summed over the splits: rows seen, rows held, nonzeros held.  The object
 * allocates on the device only in its first split.  xf_holdout_shape: {rows of a tile, output
 * nonzeros of a copy chunk, the alignment of the held part in elements}, for the tests.
 * Early stop (host, no GPU).  xf_holdout_should_stop walks logloss[0 .. n), one value per validated
 * epoch: an epoch improves iff L < best - delta (strict; the first value that is not NaN and below
 * +inf improves); a NaN neither improves nor counts as an epoch without improvement.  *best (may be
 * NULL): the index of the best epoch, -1 for none.  Returns 1 iff patience > 0, at least `patience`
 * epochs since the best one did not improve, and logloss[n - 1] is not NaN; else 0 (also for
 * n <= 0, a NULL curve, or a delta that is negative or NaN).
 * Validate.  xf_lr_validate / xf_fm_validate: exactly the forward of xf_lr_predict / xf_fm_predict
 * on every path those support — the same launches in the same order, the pulls insert unseen keys
 * at first-touch state — but instead of copying pctr out they accumulate the losses the forward
 * left (loss = sigmoid - label, one fp32 subtraction), unweighted, into `p`: one
 * xf_progress_accumulate_dev launch, no host wait beyond those predict has.  Predict itself keeps
 * every bit and launch and never accumulates.
 * xf_sharded_holdout(st, enable): the trainer owns a SECOND xf_progress, apart from the one of
 * xf_sharded_progress (created at 1, freed at 0).  XF_EINVAL on a several-rank trainer on
 * XF_SCHEDULE_OWNER / _OWNER_STALE1 (the loss is formed inside the owners' finalize kernels), and
 * xf_sharded_set_schedule to one of those two while it is on.
 * xf_sharded_validate(st, b): xf_sharded_predict's forward of minibatch b, counted into that
 * progress.  COLLECTIVE like predict — ranks without rows call it with an empty minibatch — and it
 * flushes first.  xf_sharded_holdout_read: as xf_sharded_progress_read, of the second progress. */
#define XF_HOLDOUT_SALT 0x6a09e667f3bcc909ull /* (the fraction bits of sqrt 2) */
typedef struct xf_holdout xf_holdout;
typedef struct {
  const uint64_t *d_keys;
  const int32_t *d_fgid;
  const float *d_vals;
  const uint32_t *d_rowptr;
  const int32_t *d_labels;
  uint32_t R, NNZ;
} xf_holdout_part;
int xf_holdout_create(xf_holdout **out, float share, uint64_t seed);
int xf_holdout_destroy(xf_holdout *s);
int xf_holdout_params(const xf_holdout *s, float *share, uint64_t *seed);
int xf_holdout_held(uint64_t seed, uint64_t stream, uint64_t ordinal, float share);
int xf_holdout_split_dev(xf_holdout *s, uint64_t stream_id, uint64_t first_ordinal,
                         const uint64_t *d_keys, const int32_t *d_fgid, const float *d_vals,
                         const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                         uint32_t NNZ, void *stream, xf_holdout_part *train,
                         xf_holdout_part *held);
int xf_holdout_split(xf_holdout *s, uint64_t stream_id, uint64_t first_ordinal,
                     const uint64_t *rowptr, const uint64_t *keys, const int32_t *fgid,
                     const float *vals, const int32_t *labels, size_t row_begin, size_t row_end,
                     void *stream, xf_holdout_part *train, xf_holdout_part *held);
int xf_holdout_stats(const xf_holdout *s, uint64_t *rows_seen, uint64_t *rows_held,
                     uint64_t *nnz_held);
void xf_holdout_shape(uint32_t out[3]);
int xf_holdout_should_stop(const double *logloss, int n, int patience, double delta, int *best);
int xf_lr_validate(xf_table *w, xf_batch *b, xf_workspace *ws, xf_progress *p);
int xf_fm_validate(xf_table *w, xf_table *vt, xf_batch *b, xf_workspace *ws, xf_progress *p);
int xf_sharded_holdout(xf_sharded *st, int enable);
int xf_sharded_validate(xf_sharded *st, xf_sbatch *b);
int xf_sharded_holdout_read(xf_sharded *st, uint64_t *counts, uint64_t *other, int reset,
                            int merged);

/* ---------------------------------------------------------------- grouped AUC, held-out */
/* The AUC inside each value of ONE field (user, query, placement ...), averaged with the group's
 * rows as weight (GAUC; not in the reference), on the held-out rows: it rewards ordering the
 * impressions WITHIN a group, which a global AUC does not.  An AUC needs a group's rows ordered by
 * score, so the device keeps a log of records and a reduce sorts it.  The device only produces
 * integers, so its result depends on nothing but the multiset of records — not the order of the
 * appends, the launch shapes or how many appends the records came in — and is compared with ==.
 * Record.  A row leaves (id, code): id its slice id by xf_slices' rule for field F; with
 * rank = xf_progress_rank(loss), pos = (label != 0), C as in progressive validation:
 *   rank == XF_PROGRESS_RANKS (NaN, q > 1): counted in other[pos], no record
 *   otherwise id == XF_SLICE_NONE:          counted in none[pos], no record
 *   otherwise score = pos ? 2C - rank : rank (monotone in p: the score rank the global AUC uses),
 *             code = (score << 1) | pos, a uint32
 * xf_gauc_code is that function as host code, from the one definition the kernel uses; UINT32_MAX
 * for the `other` case.
 * Group figures.  XF_GAUC_WORDS = 4 64-bit words per distinct id: P and N, the group's positive
 * and negative records; U2 = the sum over the group's distinct scores b, ascending, of
 * pos_b (2 neg_below_b + neg_b); T = the sum of pos_b neg_b, the tie mass.  Exact integers; with
 * fewer than 2^30 records U2 < 2^60.
 * xf_gauc_append_dev: R rows of device arrays, one launch on `stream` (none with R = 0); the
 * records go to a device log of two arrays (ids u64, codes u32), none[2] and other[2] are counted
 * on the device.  The log grows on demand in the order of the stream; growing waits for the
 * stream, so xf_gauc_reserve(g, rows) sizes the log ahead and an append then waits for nothing.
 * xf_gauc_append: ready-made records from host arrays (a UINT32_MAX or otherwise impossible code
 * or the id XF_SLICE_NONE: XF_EINVAL); waits.  xf_gauc_export: the log as it stands (ids and codes
 * both NULL: only *n), one wait.
 * xf_gauc_reduce: the figures of everything appended so far: *n entries of (id, P, N, U2, T), five
 * words each, sorted by id ascending, and none[2] / other[2] (either may be NULL).  entries == NULL:
 * only *n and the two pairs (reset must be 0).  *n > cap: XF_EINVAL, nothing reset.  reset != 0:
 * the log and the counters are emptied after the copy.  Reducing twice without a reset gives the
 * same result; no records: *n = 0 and no launch; 2^30 records or more: XF_EINVAL.  The records are
 * sorted by code and then stably by id (two passes of xf_sort_key_pos); one segmented pass forms
 * the figures.  xf_gauc_launches: the pack launches since the library was loaded.  xf_gauc_shape:
 * {rows of a pack workgroup, records of a reduce workgroup}, for the tests that aim at the edges.
 * Summary (host, no GPU), fp64, the groups in the order given (ascending id; anything else is
 * XF_EINVAL).  A group is scored iff P > 0 and N > 0:
 *   auc_g = fl(U2) / fl(2 P N), slack_g = fl(T) / fl(2 P N), rows_g = P + N
 *   gauc = the sum over the scored groups of w_g * auc_g, w_g = fl(rows_g) / fl(rows_scored) the
 *   group's share of the scored groups' rows (one group alone weighs exactly 1: its gauc is its auc
 *   bit for bit); gauc_slack the same with slack_g; macro_auc = (sum of auc_g) / fl(groups_scored)
 *   groups, groups_scored, rows (every record), rows_scored, rows_one_class, none_rows, other_rows
 * No scored group: the three means are NaN and the call succeeds.  The exact tie-aware GAUC of the
 * rows' p lies within gauc +- gauc_slack (progress's argument for auc_slack, per group).  auc and
 * slack (may be NULL): n per-group values, NaN for a group that is not scored.
 * Tap.  On VALIDATE only, never on a training step or on predict.  xf_workspace_gauc(ws, g)
 * attaches an object (NULL: off, the default; the caller keeps g alive); xf_workspace_gauc_ids(ws,
 * d_id, R) names the ids of the NEXT xf_lr_validate / xf_fm_validate's rows (a device array the
 * caller keeps alive until that validate has run).  That validate appends right after its
 * xf_progress_accumulate_dev, from the same losses and labels, and forgets the ids; ids of another
 * R are XF_EINVAL naming both; a validate without ids appends nothing.  With nothing attached
 * validate, predict and every step are launch for launch and bit for bit what they were.
 * xf_sharded_gauc(st, enable): the trainer owns one (created at 1, freed at 0); needs
 * xf_sharded_holdout on and inherits its refusals.  xf_sharded_validate then appends the records
 * of a minibatch that carries ids (xf_sbatch_set_slices) on both of its paths.
 * xf_sharded_gauc_read: flushes, then reduces this rank's records; merged != 0: COLLECTIVE, the
 * ranks' exported records go to rank 0 (xf_group_gatherv_host) and are reduced there — a group's
 * rows are spread over the ranks, so figures of parts cannot be merged; rank 0 gets the result,
 * the others *n = 0 and zeros; reset empties every rank's log. */
#define XF_GAUC_WORDS 4
typedef struct xf_gauc xf_gauc;
typedef struct {
  double gauc, gauc_slack, macro_auc;
  uint64_t groups, groups_scored, rows, rows_scored, rows_one_class, none_rows, other_rows;
} xf_gauc_metrics;
uint32_t xf_gauc_code(float loss, int32_t label);
int xf_gauc_summary(const uint64_t *entries, uint64_t n, const uint64_t *none,
                    const uint64_t *other, xf_gauc_metrics *out, double *auc, double *slack);
int xf_gauc_create(xf_gauc **out);
int xf_gauc_destroy(xf_gauc *g);
int xf_gauc_reserve(xf_gauc *g, uint64_t rows);
int xf_gauc_append_dev(xf_gauc *g, const float *d_loss, const int32_t *d_labels,
                       const uint64_t *d_id, uint32_t R, void *stream);
int xf_gauc_append(xf_gauc *g, const uint64_t *ids, const uint32_t *codes, uint64_t n);
int xf_gauc_export(xf_gauc *g, uint64_t *ids, uint32_t *codes, uint64_t cap, uint64_t *n);
int xf_gauc_reduce(xf_gauc *g, uint64_t *entries, uint64_t cap, uint64_t *n, uint64_t *none,
                   uint64_t *other, int reset);
uint64_t xf_gauc_launches(void);
void xf_gauc_shape(uint32_t out[2]);
int xf_workspace_gauc(xf_workspace *ws, xf_gauc *g);
int xf_workspace_gauc_ids(xf_workspace *ws, const uint64_t *d_id, uint32_t R);
int xf_sharded_gauc(xf_sharded *st, int enable);
int xf_sharded_gauc_read(xf_sharded *st, uint64_t *entries, uint64_t cap, uint64_t *n,
                         uint64_t *none, uint64_t *other, int reset, int merged);

/* ---------------------------------------------------------------- feature crosses      */
/* Crossed features as a GPU stage ahead of the key build (not in the reference).  Like admission
 * and negative subsampling it works on a minibatch's CSR arrays and its result goes to any *_dev
 * compile; it keeps no state and ADDS nonzeros.  It reads the nonzeros' field ids (fgid).
 * Definition.  mix64 as for admission (add 0x9e3779b97f4a7c15, then the splitmix64 finaliser):
 *   salt(fa, fb)              = mix64((uint64)(uint32)fa << 32 | (uint32)fb)
 *   cross_key(ka, kb, fa, fb) = mix64(mix64(ka ^ salt(fa, fb)) + kb)          (64-bit wrapping)
 * xf_cross_key is that function as host code, from the one definition the kernels use.  The key
 * depends on the two field ids, not on the pair's place in the spec: reordering or extending a
 * spec leaves existing crossed keys, and a saved model, valid.
 * A spec is 1 .. 32 ordered pairs (fa_p, fb_p), fa != fb, both in 0 .. 2^31 - 1, no pair twice;
 * (a, b) and (b, a) are different pairs.  xf_cross_parse reads "2*3,16*17" (decimal, no blanks)
 * into arrays of `cap` entries; a malformed spec is XF_EINVAL naming the offending piece.
 * xf_cross_create checks the same rules, and fgid_base >= 0 with fgid_base + npairs <= 2^31.
 * One apply = one minibatch.  The output row is the input row, unchanged and in order, then for
 * p = 0, 1, ...: for every nonzero i of the row with fgid == fa_p, in row order, and every nonzero
 * j with fgid == fb_p, in row order, one nonzero with key cross_key(key_i, key_j, fa_p, fb_p), fgid
 * fgid_base + p and value fp32(val_i * val_j).  A multi-valued field gives all |A| x |B|
 * combinations; a row without a member on either side gains nothing from the pair; a row whose
 * offsets descend or leave the arrays has length 0.  Labels and the row count do not change.  A
 * spec none of whose fields occur returns the inputs byte for byte.  Nothing depends on the launch
 * shape: every output position is arithmetic on counts.
 * xf_cross_apply_dev: device arrays (d_rowptr row-relative u32, R + 1).  d_fgid is required (NULL:
 * XF_EINVAL); d_vals may be NULL, and then no values come out; want_fgid_out = 0: no fgid comes
 * out (LR and canonical FM do not read it).  The outputs are device arrays owned by the stage,
 * valid until its next apply, written in the order of `stream` and grown geometrically; *NNZ_out =
 * the output nonzeros.  The stage allocates on the device only in an apply.  R = 0 and NNZ = 0 are
 * valid.  One wait for the stream, for the total (none with R = 0), after the count and before the
 * emit, which is where the buffers grow.  The total is counted in 64 bits: 2^32 - 1 or more is
 * XF_EINVAL naming it, with nothing emitted and no buffer grown.  Rows that overlap (their lengths
 * sum to more than NNZ) are XF_EINVAL.
 * xf_cross_apply: the reader's host arrays and a row slice: uploads the slice (rowptr rebased to
 * u32; labels, when given, to *d_labels_out unchanged) and runs the same kernels — one
 * implementation, the device one.
 * xf_cross_stats, summed over the applies: rows seen, input nonzeros, crossed nonzeros.
 * xf_tune: cross_short_max (0 .. 64, default 64: rows of at most that many nonzeros take the
 * wave-per-row emit, longer ones the workgroup-per-row emit) and cross_lds_chunks (1 .. 2048,
 * default 2048: a long row of more 64-nonzero chunks keeps its member lists in a global scratch
 * instead of LDS) move rows between the emit's paths, for tests and measurements; the result is
 * the same. */
typedef struct xf_cross xf_cross;
uint64_t xf_cross_key(uint64_t ka, uint64_t kb, int32_t fa, int32_t fb);
int xf_cross_parse(const char *spec, int32_t *fa, int32_t *fb, int cap, int *npairs);
int xf_cross_create(xf_cross **out, const int32_t *fa, const int32_t *fb, int npairs,
                    int32_t fgid_base);
int xf_cross_destroy(xf_cross *x);
int xf_cross_params(const xf_cross *x, int32_t *fa, int32_t *fb, int cap, int *npairs,
                    int32_t *fgid_base);
int xf_cross_apply_dev(xf_cross *x, const uint64_t *d_keys, const int32_t *d_fgid,
                       const float *d_vals, const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ,
                       void *stream, int want_fgid_out, const uint64_t **d_keys_out,
                       const int32_t **d_fgid_out, const float **d_vals_out,
                       const uint32_t **d_rowptr_out, uint32_t *NNZ_out);
int xf_cross_apply(xf_cross *x, const uint64_t *rowptr, const uint64_t *keys, const int32_t *fgid,
                   const float *vals, const int32_t *labels, size_t row_begin, size_t row_end,
                   void *stream, int want_fgid_out, const uint64_t **d_keys_out,
                   const int32_t **d_fgid_out, const float **d_vals_out,
                   const uint32_t **d_rowptr_out, const int32_t **d_labels_out, uint32_t *R_out,
                   uint32_t *NNZ_out);
int xf_cross_stats(const xf_cross *x, uint64_t *rows_seen, uint64_t *nonzeros_in,
                   uint64_t *nonzeros_crossed);

/* ---------------------------------------------------------------- row normalisation    */
/* Instance-wise L2 normalisation as a GPU stage ahead of the key build (not in the reference;
 * libffm and xLearn apply it by default).  It is the LAST stage, behind the cross, which adds
 * nonzeros, and admission, which removes them: a row is given unit length over the nonzeros the
 * model receives.  It changes the values only; keys, fgid, offsets and labels are not touched.
 * Definition (csrc/xf_rownorm.h, one for the host and the kernel).  A row has nonzeros x_0 ..
 * x_{m-1} in row order; a key that occurs twice counts twice.
 *   s = the sum of (double)x_i * (double)x_i (each product exact in fp64), added by the pairwise
 *       tree over the positions in row order, padded with +0.0 to a power of two: level 0 adds
 *       positions (0,1), (2,3), ...; level 1 adds those sums in adjacent pairs; and so on.  Every
 *       addend is >= 0, so the padding changes no bit: the result depends on the row alone, never
 *       on a launch shape.
 *   s > 0 and finite:  rs = 1.0 / sqrt(s), y_i = (float)((double)x_i * rs) — division, square root
 *       and product IEEE fp64 (no fast-math, no contraction); |y_i| <= 1 up to the last rounding,
 *       also for a row of subnormals.
 *   otherwise:  y_i = x_i bit for bit: an empty row, a row of zeros, a row that holds a NaN or an
 *       infinity.  Such rows stay the model's business.
 * xf_rownorm_create: kind must be XF_ROWNORM_L2 (anything else: XF_EINVAL); nothing is allocated
 * on the device before the first apply.
 * xf_rownorm_apply_dev: device arrays (d_rowptr row-relative u32, R + 1; the caller guarantees
 * rowptr[0] = 0, ascending, rowptr[R] = NNZ — the kernel still treats a row whose offsets descend
 * or leave the arrays as empty, so it never reads or writes outside them).  Runs on `stream` with
 * no host wait; R = 0 launches nothing.  *d_vals_out: NNZ normalised values, *d_sumsq_out (may be
 * NULL: then the sums are not written): the R values of s.  Both are device arrays owned by the
 * stage, grown geometrically, written in the order of `stream` and valid until the next apply on
 * the object.  The inputs are never written.  A row of any length up to NNZ takes the same entry.
 * xf_rownorm_apply: rows [row_begin, row_end) of a block's host arrays: checks the offsets on the
 * CPU (descending ones are XF_EINVAL and the object lives on), uploads the slice with an uploader
 * of its own (rowptr rebased to u32; keys, fgid when given and labels when given unchanged) and
 * calls the device entry.  vals is required where there are nonzeros.
 * xf_rownorm_row: the definition as host code: y[0 .. m) from x[0 .. m) (y may be x), *sumsq = s.
 * A NULL x or y with m > 0 is XF_EINVAL naming the argument.
 * xf_rownorm_stats, summed over the applies: rows seen (counted on the host) and rows scaled
 * (counted on the device; reading it is the one wait of the stage).
 * xf_rownorm_shape: {lanes that share a row, rows of a workgroup}.  xf_rownorm_launches: kernels
 * launched by the stage in this process. */
enum { XF_ROWNORM_L2 = 1 };
typedef struct xf_rownorm xf_rownorm;
int xf_rownorm_create(xf_rownorm **out, int kind);
int xf_rownorm_destroy(xf_rownorm *n);
int xf_rownorm_apply_dev(xf_rownorm *n, const float *d_vals, const uint32_t *d_rowptr, uint32_t R,
                         uint32_t NNZ, void *stream, const float **d_vals_out,
                         const double **d_sumsq_out);
int xf_rownorm_apply(xf_rownorm *n, const uint64_t *rowptr, const uint64_t *keys,
                     const int32_t *fgid, const float *vals, const int32_t *labels,
                     size_t row_begin, size_t row_end, void *stream, const uint64_t **d_keys_out,
                     const int32_t **d_fgid_out, const float **d_vals_out,
                     const uint32_t **d_rowptr_out, const int32_t **d_labels_out, uint32_t *R_out,
                     uint32_t *NNZ_out, const double **d_sumsq_out);
int xf_rownorm_row(const float *x, size_t m, float *y, double *sumsq);
int xf_rownorm_stats(const xf_rownorm *n, uint64_t *rows_seen, uint64_t *rows_scaled);
void xf_rownorm_shape(uint32_t out[2]);
uint64_t xf_rownorm_launches(void);

/* ---------------------------------------------------------------- metrics             */
/* Base::calculate_auc (base.h:84-110): reference-format logloss (mean of y*log2 p +
 * (1-y)*log2(1-p), negative), AUC by descending-pctr rank sum, plus the conventional
 * natural-log logloss (positive).  acc_logloss_inout is the never-reset member. */
int xf_auc_logloss(const int32_t *labels, const float *pctr, size_t n,
                   float *acc_logloss_inout, float *auc, int *tp, int *fp,
                   double *nat_logloss);

/* ---------------------------------------------------------------- worker-level C API  */
/* Signatures of src/c_api/c_api.h:26-29 kept verbatim.  The handle owns an LR or FM
 * worker (XFSetParam "model") whose table lives on the current HIP device. */
int XFCreate(void **h, const char *train_path, const char *test_path);
int XFStartTrain(void **h);
/* additive (the reference has no equivalents) */
int XFDestroy(void **h);
/* names: model(0 LR,1 FM) epochs block_size_mb core_num k optimizer(ftrl|sgd) capacity
 *        rank pred_path alpha beta lambda1 lambda2 lr seed cache_batches key_build(gpu|host)
 *        update(rank_ordered|sum_then_step: with schedule=owner)
 *        parity(exact|reference_order: the forward's row sums in the reference's own fp32
 *        order — one worker, checking mode)
 *        fm_mode(reference|canonical: FM's second-order term as the reference writes it, or
 *        Rendle's per-factor form — xf_workspace_fm_mode; canonical: model 1, one worker —
 *        |field_aware: a key keeps k factors per field and a pair interacts through the vectors
 *        each holds for the other's field; model 1, one worker, parity=exact, with fields=N)
 *        fields(1 .. 64, fields x k <= 4096: the number of field-group ids, fgid in [0, fields))
 *        feature_values(off|on: a nonzero contributes x = val, the third field of
 *        fgid:fid:val, instead of 1 — model 0, or model 1 with fm_mode=canonical or
 *        field_aware; one worker,
 *        parity=exact, block_cache=0, ingest=host)
 *        model_in model_out (model file to load before / save after training)
 *        block_cache(0|1) block_cache_dir (binarized block cache of the text files)
 *        ingest(host|gpu: the text of a block tokenised and hashed on the GPU, xf_ingest_*;
 *        blocks that are not of the common shape go to the host parser; core_num 1, no block
 *        cache.  gpu_fields: the same, and the tokeniser also reads fgid and the feature value
 *        when fm_mode=field_aware / feature_values=on need them, xf_ingest_set_fields).  XFGetMetric: ... blocks_gpu blocks_host (how the blocks were parsed)
 *        admit_count(0 off | 1 .. 255: feature admission, xf_admit_* — every block compiled from
 *        text is counted and filtered before its key build, every test block filtered; a key
 *        enters the tables once the filter has seen it that many times; one worker, core_num 1,
 *        key_build=gpu, parity=exact) admit_log2_slots(2 .. 32, default 26) admit_hashes(1 .. 8,
 *        default 3); the filter's seed is `seed`; XFSaveModel writes <path>.admit beside the
 *        model, XFLoadModel needs it.  XFGetMetric: admit_seen admit_kept (nonzeros)
 *        admit_shared(0|1: the workers of a group share one filter, xf_admit_create_shared, which
 *        lifts "one worker" — every turn of the training loop and of predict applies collectively,
 *        the empty minibatch where a rank has no rows; not with schedule=owner / owner_stale1)
 *        neg_keep(r in (0, 1], default 1 = off: negative subsampling, xf_negsample_* — every
 *        TRAINING block is sampled before admission and its key build: a row with label 0 is kept
 *        iff xf_negsample_keep(seed, (epoch << 32) | rank, the row's index in this rank's training
 *        file in this epoch, r), every other row always; the trainer weights a kept negative's loss
 *        by 1 / r (xf_sharded_set_neg_weight); test blocks are never sampled; core_num 1,
 *        key_build=gpu, parity=exact, not with schedule=owner / owner_stale1 on several workers;
 *        nothing is saved with the model).  XFGetMetric: neg_seen neg_kept (negative rows)
 *        rows_kept; rows_trained counts kept rows
 *        cross(SPEC, e.g. 2*3,16*17; default off: feature crosses, xf_cross_* — every block gains
 *        its crossed nonzeros on the GPU: training after negative subsampling and before
 *        admission, predict before admission; every rank crosses its own rows, on every schedule;
 *        core_num 1, key_build=gpu, parity=exact, not with ingest=gpu (use ingest=gpu_fields); the
 *        spec is not saved with the model: predict needs the same cross=)
 *        cross_fgid_base(N, default 0: the crossed nonzeros' fgids are N + the pair's index; read
 *        only with fm_mode=field_aware, where N + pairs <= fields).  XFGetMetric: cross_in
 *        cross_out (nonzeros into and out of the stage)
 *        row_norm(off|l2, default off: row normalisation, xf_rownorm_* — every minibatch of this
 *        rank's own rows, training, the held part of holdout and predict, is given unit L2 length
 *        per row on the GPU as the last stage, behind the cross and admission; needs
 *        feature_values=on, core_num 1, key_build=gpu, parity=exact; the setting is not saved
 *        with the model: predict needs the same row_norm=; rank 0 prints "row_norm: rows = ...
 *        scaled = ... left = ..." after training).  XFGetMetric: norm_rows norm_rows_scaled
 *        progress(0|1, default 0: progressive validation, xf_progress_* — every training step
 *        counts its rows' losses under the weights it is about to change, with no host wait inside
 *        an epoch; at the end of every epoch, replayed ones included, the counts are read, summed
 *        over the workers and reset, and rank 0 prints one line "progress epoch E: rows = ...
 *        logloss = ... (+- bound) auc = ... (+- slack) ctr = ... pctr = ..." and, when nonzero,
 *        saturated / other; a negative weighs 1 / neg_keep; not with schedule=owner / owner_stale1
 *        on several workers).  XFGetMetric: progress_logloss progress_auc progress_auc_slack
 *        progress_ctr progress_pctr progress_rows (the last epoch) progress_logloss_first
 *        progress_auc_first (epoch 0: the held-out figure)
 *        progress_by(F, a field id in 0 .. 2^31 - 1; default off: sliced progressive validation,
 *        xf_slices_* — with progress=1, every TRAINING block's rows are named by the key of their
 *        first nonzero of field F, after negative subsampling and before the cross; the ids travel
 *        with the compiled minibatch, so replayed epochs count too; after the "progress epoch" line
 *        rank 0 prints "progress slices epoch E: field = F slices = S rows = ... none_rows = ...
 *        overflow_rows = ..." — weighted rows; a note when overflow is not empty — and the
 *        progress_top heaviest slices by weighted rows, ties by key, each as "  key = 0x... rows =
 *        ... ctr = ... pctr = ... logloss = ..."; core_num 1, key_build=gpu, parity=exact, not
 *        with ingest=gpu (use ingest=gpu_fields), progress's own refusals; nothing is saved with
 *        the model) progress_slots(b in 2 .. 26, default 16: every worker's table has 2^b entries
 *        of 64 bytes) progress_top(N >= 0, default 10) progress_slices_out(PATH: rank 0 appends one
 *        tab-separated line per slice and epoch, by key: epoch, key (0x...), n0, n1, other, ctr,
 *        pctr, logloss).  XFGetMetric (the last epoch): slices slice_rows slice_none_rows
 *        slice_overflow_rows (weighted rows; slice_rows = entries + none + overflow =
 *        progress_rows)
 *        holdout(r in [0, 1), default 0 = off: held-out validation, xf_holdout_* — every TRAINING
 *        block is split first, on the GPU: a row is held iff xf_holdout_held(seed, rank, the row's
 *        index in this rank's training file, r) — no epoch in the stream: the same rows in every
 *        epoch — and only the train part is trained on.  With neg_keep < 1 the sampler then
 *        numbers the rows of the TRAIN part (a second running count): neg_keep's ordinal changes
 *        only when both are on.  The held part goes through the cross and through admission
 *        without being counted, after the block's train part, is compiled once and kept in HBM
 *        whatever cache_batches says.  After the flush of every holdout_every-th epoch and of the
 *        last one the held minibatches are scored with xf_sharded_validate, the counts are summed
 *        over the workers and rank 0 prints "holdout epoch E: rows = ... logloss = ... (+- bound)
 *        auc = ... (+- slack) ctr = ... pctr = ..." (E counts from 0, as progress's; unweighted).
 *        core_num 1, key_build=gpu, parity=exact, not with schedule=owner / owner_stale1 on several
 *        workers; nothing is saved with the model) holdout_every(E >= 1, default 1)
 *        early_stop(P >= 0, default 0 = off; needs holdout: training ends after P validated epochs
 *        without an improvement by xf_holdout_should_stop's rule; rank 0 prints "early stop after
 *        epoch E: best epoch B logloss = ..."; that epoch counts as the last one — eviction's
 *        after-the-last-epoch pass, save and predict follow) early_stop_delta(d >= 0, default 0).
 *        XFGetMetric: holdout_rows holdout_logloss holdout_auc holdout_auc_slack holdout_ctr
 *        holdout_pctr (the last validated epoch) holdout_logloss_first holdout_best_epoch
 *        holdout_best_logloss epochs_run; rows_trained excludes held rows
 *        holdout_by(F in 0 .. 2^31 - 1, default off; needs holdout > 0: the grouped AUC of the
 *        held rows, xf_gauc_* — a held row's group is the key of its first nonzero of field F, named
 *        on the GPU as the split hands the held part over, before the cross and admission; every
 *        validated epoch appends the held rows' records, and after the "holdout epoch E:" line the
 *        records are reduced — merged on rank 0 over the workers — and rank 0 prints "holdout groups
 *        epoch E: field = F groups = G scored = S rows = ... scored_rows = ... none_rows = ... gauc =
 *        ... (+- slack) macro_auc = ..." (and other_rows = ... when there are any).  core_num 1,
 *        key_build=gpu, ingest=host or gpu_fields; the early-stop rule keeps reading the logloss;
 *        nothing is saved with the model) holdout_groups_out(PATH: rank 0 appends one tab-separated
 *        line per group and epoch, by key: epoch, key (0x...), P, N, auc, slack).  XFGetMetric (the
 *        last validated epoch): holdout_gauc holdout_gauc_slack holdout_macro_auc holdout_groups
 *        holdout_groups_scored holdout_gauc_rows (the scored groups' rows) */
int XFSetParam(void *h, const char *name, const char *value);
/* after XFStartTrain: logloss_ref, logloss_nat, auc, tp, fp, rows_trained, train_seconds,
 * examples_per_sec, keys */
int XFGetMetric(void *h, const char *name, double *value);
/* model file (the reference never saves its model): key-sorted (key, w, n, z) dumps of the
 * worker's tables; XFPredict scores the test file with the current tables, no training */
int XFSaveModel(void *h, const char *path);
int XFLoadModel(void *h, const char *path);
int XFPredict(void *h);
/* the worker's tables, for export/checkpoint (NULL v for LR) */
int XFGetTables(void *h, xf_table **w, xf_table **v);

#ifdef __cplusplus
}
#endif
#endif /* XFLOW_AMD_H_ */
