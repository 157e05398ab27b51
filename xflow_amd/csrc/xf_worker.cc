// xf_worker.cc — LRWorker / FMWorker and the XFCreate / XFStartTrain C API.
//
// Mirrors the reference's worker surface (same public members and call order):
//   xflow::LRWorker  src/model/lr/lr_worker.{h,cc}  (ctor(train,test), epochs, train(),
//                    batch_training(), update(), predict(), calculate_pctr())
//   xflow::FMWorker  src/model/fm/fm_worker.{h,cc}
//   xflow::Server    src/model/server.h:22-31        (which optimizer serves w and v)
//   XFCreate/XFStartTrain  src/c_api/c_api.{h,cc}
// but every Pull / Push / loss / gradient runs on the GPU through the extern "C" shim
// (xf_table_*, xf_lr_step, xf_fm_step).  What stays on the host is what north_star keeps
// there: the libsvm-format block reader and the per-block key build.
#include <hip/hip_runtime_api.h>
#include <unistd.h>

#include "xf_worker.h"
#include "xf_slices.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <fstream>
#include <initializer_list>
#include <iostream>

namespace xf {
int model_write(const char *path, xf_table *tw, xf_table *tv, int k);
int model_read(const char *path, xf_table *tw, xf_table *tv, int k, uint32_t shard,
               uint32_t nshards);
}  // namespace xf

namespace xflow_amd {

static double now_s() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

Worker::Worker(int model, const char *train_file, const char *test_file)
    : model_(model), train_file_path(train_file ? train_file : ""),
      test_file_path(test_file ? test_file : "") {}

Worker::~Worker() {
  for (std::thread &t : closers_) t.join();
  for (xf_block *b : blocks_)
    if (b) xf_block_destroy(b);
  for (xf_ingest *g : ingest_)
    if (g) xf_ingest_destroy(g);
  for (xf_sbatch *b : cache_) xf_sbatch_free(b);
  for (xf_sbatch *b : held_) xf_sbatch_free(b);
  if (split_) xf_holdout_destroy(split_);
  if (admit_) xf_admit_destroy(admit_);
  if (sample_) xf_negsample_destroy(sample_);
  if (cross_) xf_cross_destroy(cross_);
  if (norm_) xf_rownorm_destroy(norm_);
  if (slicer_) xf_slices_destroy(slicer_);
  if (gslicer_) xf_slices_destroy(gslicer_);
  if (sharded_) xf_sharded_destroy(sharded_);  // owns the tables
  if (group_) xf_group_destroy(group_);
}

static const char *env_first(std::initializer_list<const char *> names) {
  for (const char *n : names) {
    const char *v = getenv(n);
    if (v && *v) return v;
  }
  return nullptr;
}

// xflow::Server (server.h:22-31): app 0 serves w, app 1 serves v; FTRL by default, the SGD
// handlers are the commented-out alternative (server.h:25,29).  ps::Start / MyRank
// (main.cc:22-47): with more than one worker (world=, or WORLD_SIZE / DMLC_NUM_WORKER in the
// environment, as scripts/local.sh sets it) this process joins the group — one process per
// GPU — and its tables are one key-range shard of the parameter table.
int Worker::create_tables() {
  // (row_norm's refusals by its own name, also where XFLoadModel builds the tables: ahead of the
  // warm-up below, which would refuse a valued minibatch on key_build=host in its own words)
  XF_TRY(check_rownorm());
  if (sharded_) {
    XF_TRY(create_admit());
    XF_TRY(create_negsample());
    XF_TRY(create_holdout());
    XF_TRY(create_cross());
    return create_rownorm();
  }
  int w = world;
  if (w <= 0) {
    const char *v = env_first({"WORLD_SIZE", "XF_WORLD", "DMLC_NUM_WORKER"});
    w = v ? atoi(v) : 1;
  }
  if (w > 1) {
    XF_TRY(xf_group_create(&group_, rank_given_ ? rank : -1, w, nullptr, 0,
                           transport, -2));
    int r = 0;
    XF_TRY(xf_group_info(group_, &r, &w, nullptr));
    rank = r;  // ps::MyRank(): selects <prefix>-%05d (lr_worker.cc:208-210)
  }
  world = w;
  xf_sharded_config c;
  xf_sharded_config_default(&c);
  c.model = model_;
  c.optimizer = optimizer;
  c.k = v_width();  // (field_aware: fields x k)
  c.schedule = schedule;
  c.capacity = capacity;
  c.seed = seed;
  c.alpha = alpha;
  c.beta = beta;
  c.lambda1 = lambda1;
  c.lambda2 = lambda2;
  c.lr = learning_rate;
  c.host_key_build = key_build_gpu && parity == XF_PARITY_EXACT_SUMS ? 0 : 1;
  c.update_rule = update_rule;
  XF_TRY(xf_sharded_create(&sharded_, group_, &c));
  if (parity != XF_PARITY_EXACT_SUMS) XF_TRY(xf_sharded_set_parity(sharded_, parity));
  if (fm_mode == XF_FM_FIELD_AWARE) XF_TRY(xf_sharded_set_fm_fields(sharded_, fields));
  if (fm_mode != XF_FM_REFERENCE) XF_TRY(xf_sharded_set_fm_mode(sharded_, fm_mode));
  if (progress) XF_TRY(xf_sharded_progress(sharded_, 1));
  if (progress_by_set) {
    XF_TRY(xf_sharded_slices(sharded_, 1, (int32_t)progress_by, progress_slots));
    if (!slicer_) XF_TRY(xf_slices_create(&slicer_, (int32_t)progress_by, xf::kSlicesMinLog2));
  }
  XF_TRY(xf_sharded_tables(sharded_, &table_w_, &table_v_));
  // One update() and one predict of a two-row minibatch on a private single-shard trainer: the
  // first launch of a kernel loads its code object and the builders size their scratch on first
  // use (~45 ms together) — start-up work, done here instead of inside the first block of the
  // training loop.  The real tables are not touched.
  {
    xf_sharded_config wc = c;
    wc.capacity = 1024;
    xf_sharded *warm = nullptr;
    XF_TRY(xf_sharded_create(&warm, nullptr, &wc));
    const uint64_t rp[3] = {0, 2, 4}, keys[4] = {11, 12, 12, 13};
    const int32_t lab[2] = {0, 1};
    float p[2];
    xf_sbatch *b = nullptr;
    const float vals[4] = {1.0f, 0.5f, 0.25f, 2.0f};
    const int32_t fg[4] = {0, fields - 1, 0, fields - 1};
    const bool ffm = fm_mode == XF_FM_FIELD_AWARE;
    int rc = ffm ? xf_sharded_set_fm_fields(warm, fields) : XF_OK;
    if (rc == XF_OK && fm_mode != XF_FM_REFERENCE) rc = xf_sharded_set_fm_mode(warm, fm_mode);
    // (neg_keep < 1: the weight kernel's first launch belongs here too — after the parameter's
    // own check, so that a bad value is refused by its name)
    if (rc == XF_OK) rc = check_negsample();
    if (rc == XF_OK && neg_keep < 1.0f) rc = xf_sharded_set_neg_weight(warm, 1.0f / neg_keep);
    if (rc == XF_OK && progress) rc = xf_sharded_progress(warm, 1);  // (its kernel's first launch)
    if (rc == XF_OK) rc = compile_rows(warm, &b, 0, rp, keys, fg, vals, lab, 0, 2, 1);
    if (rc == XF_OK && progress_by_set) {  // (the two slices kernels' first launches)
      const int32_t sf[4] = {(int32_t)progress_by, 0, 0, (int32_t)progress_by};
      const uint64_t *ids = nullptr;
      uint32_t R = 0;
      void *stream = nullptr;
      rc = xf_sharded_slices(warm, 1, (int32_t)progress_by, xf::kSlicesMinLog2);
      if (rc == XF_OK) rc = xf_sharded_stream(warm, &stream);
      if (rc == XF_OK) rc = xf_slices_extract(slicer_, rp, keys, sf, 0, 2, stream, &ids, &R);
      if (rc == XF_OK) rc = xf_sbatch_set_slices(b, ids, R);
    }
    if (rc == XF_OK) rc = xf_sharded_step(warm, b);
    if (rc == XF_OK) rc = xf_sharded_predict(warm, b, p);
    if (b) xf_sbatch_free(b);
    xf_sharded_destroy(warm);
    XF_TRY(rc);
  }
  XF_TRY(create_admit());
  XF_TRY(create_negsample());
  XF_TRY(create_holdout());
  XF_TRY(create_cross());
  return create_rownorm();
}

static int world_from_env(int world) {
  if (world > 0) return world;
  const char *v = env_first({"WORLD_SIZE", "XF_WORLD", "DMLC_NUM_WORKER"});
  return v ? atoi(v) : 1;
}

// Feature admission is a filter in front of ONE worker's key build on the GPU: each rank of a
// group would count only its own shard of the data (and rank 0's predict would test keys other
// ranks admitted) — unless the ranks share one filter (admit_shared=1: xf_admit_create_shared,
// every apply collective); core_num > 1 slices a block after it was read, the host key build and
// the reference-order forward take host arrays.  All refused by name, before any rendezvous.
int Worker::check_admit() const {
  if (admit_count == 0) return XF_OK;
  XF_REQUIRE(admit_count >= 1 && admit_count <= 255,
             "XFStartTrain: admit_count must be 0 (off) or in 1 .. 255 (8-bit counters), not %d",
             admit_count);
  XF_REQUIRE(admit_log2_slots >= 2 && admit_log2_slots <= 32,
             "XFStartTrain: admit_log2_slots must be in 2 .. 32, not %d", admit_log2_slots);
  XF_REQUIRE(admit_hashes >= 1 && admit_hashes <= 8,
             "XFStartTrain: admit_hashes must be in 1 .. 8, not %d", admit_hashes);
  const int w = sharded_ ? world : world_from_env(world);
  XF_REQUIRE(w <= 1 || admit_shared, "XFStartTrain: admit_count=%d runs on one worker only "
             "(world %d): every rank would count its own shard of the data (admit_shared=1 shares "
             "one filter between the ranks)", admit_count, w);
  // (the owner-compute schedules compile through a path of their own, compile_owner: admission
  // inside that dataflow is not built)
  XF_REQUIRE(w <= 1 || (schedule != XF_SCHEDULE_OWNER && schedule != XF_SCHEDULE_OWNER_STALE1),
             "XFStartTrain: admit_count=%d admit_shared=1 together with schedule=owner / "
             "owner_stale1 (world %d): use schedule=sequential or stale1", admit_count, w);
  XF_REQUIRE(core_num <= 1, "XFStartTrain: admit_count=%d needs core_num=1, not core_num=%d",
             admit_count, core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: admit_count=%d together with key_build=host: the "
             "filtered minibatch is born on the GPU (use key_build=gpu)", admit_count);
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: admit_count=%d together with "
             "parity=reference_order: that mode builds its keys on the host", admit_count);
  return XF_OK;
}

int Worker::create_admit() {
  if (admit_count == 0 || admit_) return XF_OK;
  XF_TRY(check_admit());
  // (admit_shared=1: one filter on the worker's group — COLLECTIVE; one worker has no group)
  if (admit_shared)
    return xf_admit_create_shared(&admit_, group_, admit_log2_slots, admit_hashes, admit_count,
                                  seed);
  return xf_admit_create(&admit_, admit_log2_slots, admit_hashes, admit_count, seed);
}

// Negative subsampling drops rows of a training block on the GPU ahead of the key build: core_num
// > 1 slices a block after it was read, the host key build and the reference-order forward take
// host arrays, and on several workers the owner-compute schedules form the loss inside the owners'
// finalize kernels, where no weight is applied.  All refused by name, before any rendezvous.
int Worker::check_negsample() const {
  XF_REQUIRE(neg_keep > 0.0f && neg_keep <= 1.0f,
             "XFStartTrain: neg_keep must be in (0, 1] (the share of the negatives that is kept), "
             "not %g", (double)neg_keep);
  if (neg_keep == 1.0f) return XF_OK;
  XF_REQUIRE(core_num <= 1, "XFStartTrain: neg_keep=%g needs core_num=1, not core_num=%d",
             (double)neg_keep, core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: neg_keep=%g together with key_build=host: the sampled "
             "minibatch is born on the GPU (use key_build=gpu)", (double)neg_keep);
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: neg_keep=%g together with "
             "parity=reference_order: that mode builds its keys on the host", (double)neg_keep);
  const int w = sharded_ ? world : world_from_env(world);
  XF_REQUIRE(w <= 1 || (schedule != XF_SCHEDULE_OWNER && schedule != XF_SCHEDULE_OWNER_STALE1),
             "XFStartTrain: neg_keep=%g together with schedule=owner / owner_stale1 (world %d): the "
             "owners form the loss unweighted (use schedule=sequential or stale1)",
             (double)neg_keep, w);
  return XF_OK;
}

// Progressive validation taps the loss between a step's forward and its gradient: on several
// workers the owner-compute schedules form it inside the owners' finalize kernels.  Refused by
// name, before any rendezvous.
int Worker::check_progress() const {
  XF_REQUIRE(progress == 0 || progress == 1, "XFStartTrain: progress must be 0 or 1, not %d",
             progress);
  if (!progress) return XF_OK;
  const int w = sharded_ ? world : world_from_env(world);
  XF_REQUIRE(w <= 1 || (schedule != XF_SCHEDULE_OWNER && schedule != XF_SCHEDULE_OWNER_STALE1),
             "XFStartTrain: progress=1 together with schedule=owner / owner_stale1 (world %d): the "
             "owners form the loss where no tap reads it (use schedule=sequential or stale1)", w);
  return XF_OK;
}

// Table eviction judges the n of an FTRL row of dim 1: FM's v rows and SGD rows have no such
// predicate, and the owner-compute schedules' minibatches are not covered (xf_sharded_evict).
// Refused by name, before any rendezvous.
int Worker::check_evict() const {
  XF_REQUIRE(evict_n >= 0.0f, "XFStartTrain: evict_n must be 0 (off), a positive number or inf, "
             "not %g", (double)evict_n);
  XF_REQUIRE(evict_every >= 1, "XFStartTrain: evict_every must be >= 1 (epochs), not %d",
             evict_every);
  if (evict_n == 0.0f) return XF_OK;
  XF_REQUIRE(model_ == 0, "XFStartTrain: evict_n=%g with model 1 (FM): only LR tables are evicted "
             "(an FM key's v row is not zero when its w is)", (double)evict_n);
  XF_REQUIRE(optimizer == XF_OPT_FTRL, "XFStartTrain: evict_n=%g together with optimizer=sgd: an "
             "SGD row keeps no n to judge it by (use optimizer=ftrl)", (double)evict_n);
  const int w = sharded_ ? world : world_from_env(world);
  XF_REQUIRE(w <= 1 || (schedule != XF_SCHEDULE_OWNER && schedule != XF_SCHEDULE_OWNER_STALE1),
             "XFStartTrain: evict_n=%g together with schedule=owner / owner_stale1 (world %d): "
             "eviction is not built for the owner-compute schedules (use schedule=sequential or "
             "stale1)", (double)evict_n, w);
  return XF_OK;
}

// the end of an epoch, after the flush, in place of the boundary's defrag: every rank evicts its
// shard (local); the counts summed over the ranks; one line on rank 0
int Worker::evict_epoch(int epoch) {
  uint64_t mine[2] = {0, 0};
  XF_TRY(xf_sharded_evict(sharded_, evict_n, &mine[0], &mine[1]));
  XF_TRY(xf_table_size(table_w_, &keys_seen_));  // (defrag_if_grown's inflow starts from here)
  uint64_t sum[2] = {mine[0], mine[1]};
  if (world > 1) {
    std::vector<uint64_t> all(2 * (size_t)world);
    XF_TRY(xf_group_allgather_host(group_, mine, sizeof(mine), all.data()));
    sum[0] = sum[1] = 0;
    for (int r = 0; r < world; ++r) {
      sum[0] += all[2 * (size_t)r];
      sum[1] += all[2 * (size_t)r + 1];
    }
  }
  evict_seen_ += sum[0];
  evict_dropped_ += sum[1];
  if (rank == 0)
    std::cout << "evict epoch " << epoch + 1 << ": rows = " << sum[0] << " dropped = " << sum[1]
              << std::endl;
  return XF_OK;
}

// Sliced progressive validation names a training block's rows on the GPU ahead of the key build,
// from the nonzeros' field ids: core_num > 1 slices a block after it was read, the host key build
// and the reference-order forward take host arrays, ingest=gpu hands out no fgid, and the counters
// sit where progressive validation taps the losses.  All refused by name, before any rendezvous.
int Worker::check_slices() const {
  if (!progress_by_set) return XF_OK;
  XF_REQUIRE(progress_by >= 0 && progress_by <= 0x7fffffffll,
             "XFStartTrain: progress_by must be a field id in 0 .. 2147483647, not %lld",
             progress_by);
  XF_REQUIRE(progress_slots >= xf::kSlicesMinLog2 && progress_slots <= xf::kSlicesMaxLog2,
             "XFStartTrain: progress_slots must be in %d .. %d (the slice table has 2^b entries), "
             "not %d", xf::kSlicesMinLog2, xf::kSlicesMaxLog2, progress_slots);
  XF_REQUIRE(progress_top >= 0, "XFStartTrain: progress_top must be >= 0, not %d", progress_top);
  XF_REQUIRE(progress == 1, "XFStartTrain: progress_by=%lld together with progress=0: the slices "
             "are counted where progressive validation taps the losses (use progress=1)",
             progress_by);
  XF_REQUIRE(!ingest_gpu, "XFStartTrain: progress_by=%lld together with ingest=gpu: the GPU "
             "tokeniser hands out no fgid (use ingest=gpu_fields)", progress_by);
  XF_REQUIRE(core_num <= 1, "XFStartTrain: progress_by=%lld needs core_num=1, not core_num=%d",
             progress_by, core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: progress_by=%lld together with key_build=host: the "
             "rows are named on the GPU (use key_build=gpu)", progress_by);
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: progress_by=%lld together with "
             "parity=reference_order: that mode builds its keys on the host", progress_by);
  return XF_OK;
}

// the end of an epoch, after the progress line: the epoch's slices, merged over the ranks, and reset
int Worker::slices_epoch(int epoch) {
  if (!progress_by_set) return XF_OK;
  constexpr size_t E = XF_SLICE_WORDS + 1;
  const int merged = world > 1;
  uint64_t n = 0;
  XF_TRY(xf_sharded_slices_read(sharded_, nullptr, 0, &n, nullptr, nullptr, 0, merged));
  std::vector<uint64_t> entries(std::max<uint64_t>(n, 1) * E);
  uint64_t none[XF_SLICE_WORDS], overflow[XF_SLICE_WORDS];
  XF_TRY(xf_sharded_slices_read(sharded_, entries.data(), std::max<uint64_t>(n, 1), &n, none,
                                overflow, 1, merged));
  float weight = 1.0f;
  if (sample_) XF_TRY(xf_negsample_weight(sample_, &weight));
  struct Row {
    uint64_t key;
    const uint64_t *w;
    xf_slice_metrics m;
  };
  std::vector<Row> rows((size_t)n);
  double total = 0.0;
  for (size_t i = 0; i < (size_t)n; ++i) {
    rows[i].key = entries[i * E];
    rows[i].w = &entries[i * E + 1];
    XF_TRY(xf_slices_summary(rows[i].w, weight, &rows[i].m));
    total += rows[i].m.rows;
  }
  xf_slice_metrics mn, mo;
  XF_TRY(xf_slices_summary(none, weight, &mn));
  XF_TRY(xf_slices_summary(overflow, weight, &mo));
  slices_last_[0] = (double)n;
  slices_last_[1] = total + mn.rows + mo.rows;
  slices_last_[2] = mn.rows;
  slices_last_[3] = mo.rows;
  slices_have_ = true;
  if (rank != 0) return XF_OK;
  const bool incomplete = mo.rows != 0 || mo.other != 0;
  printf("progress slices epoch %d: field = %lld slices = %llu rows = %.12g none_rows = %.12g "
         "overflow_rows = %.12g%s\n", epoch, progress_by, (unsigned long long)n, slices_last_[1],
         mn.rows, mo.rows,
         incomplete ? " (the table is full: per-slice figures are incomplete, raise progress_slots)"
                    : "");
  if (!progress_slices_out.empty()) {  // one line per slice, by key
    FILE *f = fopen(progress_slices_out.c_str(), "a");
    XF_REQUIRE(f, "progress_slices_out: cannot append to %s", progress_slices_out.c_str());
    for (const Row &r : rows)
      fprintf(f, "%d\t0x%016llx\t%llu\t%llu\t%llu\t%.17g\t%.17g\t%.17g\n", epoch,
              (unsigned long long)r.key, (unsigned long long)r.w[0], (unsigned long long)r.w[1],
              (unsigned long long)r.w[6], r.m.ctr, r.m.pctr, r.m.logloss);
    fclose(f);
  }
  // the heaviest slices: weighted rows descending, ties by key ascending (the entries are by key)
  std::stable_sort(rows.begin(), rows.end(),
                   [](const Row &a, const Row &b) { return a.m.rows > b.m.rows; });
  for (size_t i = 0; i < rows.size() && i < (size_t)progress_top; ++i)
    printf("  key = 0x%016llx rows = %.12g ctr = %.6f pctr = %.6f logloss = %.6f\n",
           (unsigned long long)rows[i].key, rows[i].m.rows, rows[i].m.ctr, rows[i].m.pctr,
           rows[i].m.logloss);
  fflush(stdout);
  return XF_OK;
}

// the end of an epoch, after the flush: the epoch's counts, summed over the ranks, and reset
int Worker::progress_epoch(int epoch) {
  if (!progress) return XF_OK;
  std::vector<uint64_t> counts(2 * (size_t)XF_PROGRESS_RANKS);
  uint64_t other[2] = {0, 0};
  XF_TRY(xf_sharded_progress_read(sharded_, counts.data(), other, 1, world > 1));
  float weight = 1.0f;
  if (sample_) XF_TRY(xf_negsample_weight(sample_, &weight));
  XF_TRY(xf_progress_summary(counts.data(), other, weight, &progress_last_));
  if (!progress_have_) progress_first_ = progress_last_;
  progress_have_ = true;
  if (rank != 0) return XF_OK;
  const xf_progress_metrics &m = progress_last_;
  char line[512];
  int at = snprintf(line, sizeof(line),
                    "progress epoch %d: rows = %.12g logloss = %.6f (+- %.1e) auc = %.6f (+- %.1e) "
                    "ctr = %.6f pctr = %.6f", epoch, m.rows_pos + m.rows_neg, m.logloss,
                    m.logloss_bound, m.auc, m.auc_slack, m.ctr, m.pctr);
  if (m.saturated != 0 && at < (int)sizeof(line))
    at += snprintf(line + at, sizeof(line) - at, " saturated = %.17g", m.saturated);
  if (m.other != 0 && at < (int)sizeof(line))
    snprintf(line + at, sizeof(line) - at, " other = %.17g", m.other);
  std::cout << line << std::endl;
  return XF_OK;
}

int Worker::create_negsample() {
  if (neg_keep == 1.0f || sample_) return XF_OK;
  XF_TRY(check_negsample());
  XF_TRY(xf_negsample_create(&sample_, neg_keep, seed));
  float weight = 1.0f;
  XF_TRY(xf_negsample_weight(sample_, &weight));
  XF_TRY(xf_sharded_set_neg_weight(sharded_, weight));
  // the sampler's first launches, on two rows of a private sampler: start-up work like the two-row
  // update of create_tables (the worker's own sampler keeps its statistics clean)
  xf_negsample *warm = nullptr;
  XF_TRY(xf_negsample_create(&warm, neg_keep, seed));
  static const uint64_t rp[3] = {0, 2, 4}, keys[4] = {11, 12, 12, 13};
  static const int32_t lab[2] = {0, 1};
  void *stream = nullptr;
  int rc = xf_sharded_stream(sharded_, &stream);
  const uint64_t *fk = nullptr;
  const uint32_t *fr = nullptr;
  const int32_t *fl = nullptr;
  uint32_t R = 0, NNZ = 0;
  if (rc == XF_OK)
    rc = xf_negsample_apply(warm, 0, 0, rp, keys, nullptr, nullptr, lab, 0, 2, stream, &fk,
                            nullptr, nullptr, &fr, &fl, &R, &NNZ);
  if (rc == XF_OK) rc = xf_stream_sync(stream);
  xf_negsample_destroy(warm);
  return rc;
}

int Worker::sample_dev(size_t first_row, const uint64_t **d_keys, const int32_t **d_fgid,
                       const float **d_vals, const uint32_t **d_rowptr, const int32_t **d_labels,
                       uint32_t *R, uint32_t *NNZ) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  // (with holdout on the sampler numbers the rows of the TRAIN part: split_dev's running count)
  return xf_negsample_apply_dev(sample_, sample_stream_,
                                split_ ? train_block_first_ : ordinal_ + first_row, *d_keys,
                                fm_mode == XF_FM_FIELD_AWARE || cross_ || slicer_ ? *d_fgid : nullptr,
                                feature_values ? *d_vals : nullptr, *d_rowptr, *d_labels, *R, *NNZ,
                                stream, d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ);
}

// Held-out validation splits a training block on the GPU ahead of every other stage: core_num > 1
// slices a block after it was read (a row would have no file-wide index), the host key build and
// the reference-order forward take host arrays, and on several workers the owner-compute schedules
// form the loss inside the owners' finalize kernels.  All refused by name, before any rendezvous.
int Worker::check_holdout() const {
  XF_REQUIRE(holdout >= 0.0f && holdout < 1.0f,
             "XFStartTrain: holdout must be in [0, 1) (the share of the training rows that is held "
             "out; 0 = off), not %g", (double)holdout);
  XF_REQUIRE(holdout_every >= 1, "XFStartTrain: holdout_every must be >= 1 (epochs), not %d",
             holdout_every);
  XF_REQUIRE(early_stop >= 0, "XFStartTrain: early_stop must be >= 0 (validated epochs without "
             "improvement; 0 = off), not %d", early_stop);
  XF_REQUIRE(early_stop_delta >= 0.0, "XFStartTrain: early_stop_delta must be >= 0, not %g",
             early_stop_delta);
  XF_REQUIRE(early_stop == 0 || holdout > 0.0f, "XFStartTrain: early_stop=%d without holdout: "
             "the rule reads the held-out logloss (use holdout=r)", early_stop);
  if (holdout == 0.0f) return XF_OK;
  XF_REQUIRE(core_num <= 1, "XFStartTrain: holdout=%g needs core_num=1, not core_num=%d",
             (double)holdout, core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: holdout=%g together with key_build=host: the split "
             "minibatch is born on the GPU (use key_build=gpu)", (double)holdout);
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: holdout=%g together with "
             "parity=reference_order: that mode builds its keys on the host", (double)holdout);
  const int w = sharded_ ? world : world_from_env(world);
  XF_REQUIRE(w <= 1 || (schedule != XF_SCHEDULE_OWNER && schedule != XF_SCHEDULE_OWNER_STALE1),
             "XFStartTrain: holdout=%g together with schedule=owner / owner_stale1 (world %d): the "
             "owners' finalize kernels form the loss where no tap reads it (use schedule=sequential "
             "or stale1)", (double)holdout, w);
  return XF_OK;
}

// The grouped AUC names the held part's rows on the GPU from the nonzeros' field ids, as sliced
// progressive validation names the training rows: the same requirements, and held-out validation
// on.  All refused by name, before any rendezvous.
int Worker::check_gauc() const {
  if (!holdout_by_set) return XF_OK;
  XF_REQUIRE(holdout_by >= 0 && holdout_by <= 0x7fffffffll,
             "XFStartTrain: holdout_by must be a field id in 0 .. 2147483647, not %lld", holdout_by);
  XF_REQUIRE(holdout > 0.0f, "XFStartTrain: holdout_by=%lld without holdout: the groups are those "
             "of the held-out rows (use holdout=r)", holdout_by);
  XF_REQUIRE(!ingest_gpu, "XFStartTrain: holdout_by=%lld together with ingest=gpu: the GPU "
             "tokeniser hands out no fgid (use ingest=gpu_fields)", holdout_by);
  XF_REQUIRE(core_num <= 1, "XFStartTrain: holdout_by=%lld needs core_num=1, not core_num=%d",
             holdout_by, core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: holdout_by=%lld together with key_build=host: the "
             "rows are named on the GPU (use key_build=gpu)", holdout_by);
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: holdout_by=%lld together with "
             "parity=reference_order: that mode builds its keys on the host", holdout_by);
  return XF_OK;
}

// after the holdout line of a validated epoch: the held rows' records reduced — on several ranks
// merged on rank 0 — and reset, the summary to every rank (the metrics), rank 0 prints
int Worker::gauc_epoch(int epoch) {
  if (!gslicer_) return XF_OK;
  constexpr size_t E = XF_GAUC_WORDS + 1;
  const int merged = world > 1;
  uint64_t n = 0, none[2] = {0, 0}, other[2] = {0, 0};
  XF_TRY(xf_sharded_gauc_read(sharded_, nullptr, 0, &n, nullptr, nullptr, 0, merged));
  std::vector<uint64_t> entries(std::max<uint64_t>(n, 1) * E);
  XF_TRY(xf_sharded_gauc_read(sharded_, entries.data(), std::max<uint64_t>(n, 1), &n, none, other,
                              1, merged));
  std::vector<double> auc((size_t)n + 1), slack((size_t)n + 1);
  xf_gauc_metrics m;
  XF_TRY(xf_gauc_summary(entries.data(), n, none, other, &m, auc.data(), slack.data()));
  if (merged) {  // (rank 0 reduced: its summary is everybody's)
    std::vector<xf_gauc_metrics> all((size_t)world);
    XF_TRY(xf_group_allgather_host(group_, &m, sizeof(m), all.data()));
    m = all[0];
  }
  gauc_last_ = m;
  gauc_have_ = true;
  if (rank != 0) return XF_OK;
  printf("holdout groups epoch %d: field = %lld groups = %llu scored = %llu rows = %llu "
         "scored_rows = %llu none_rows = %llu gauc = %.6f (+- %.1e) macro_auc = %.6f",
         epoch, holdout_by, (unsigned long long)m.groups, (unsigned long long)m.groups_scored,
         (unsigned long long)m.rows, (unsigned long long)m.rows_scored,
         (unsigned long long)m.none_rows, m.gauc, m.gauc_slack, m.macro_auc);
  if (m.other_rows) printf(" other_rows = %llu", (unsigned long long)m.other_rows);
  printf("\n");
  fflush(stdout);
  if (!holdout_groups_out.empty()) {  // one line per group, by key
    FILE *f = fopen(holdout_groups_out.c_str(), "a");
    XF_REQUIRE(f, "holdout_groups_out: cannot append to %s", holdout_groups_out.c_str());
    for (size_t i = 0; i < (size_t)n; ++i)
      fprintf(f, "%d\t0x%016llx\t%llu\t%llu\t%.17g\t%.17g\n", epoch,
              (unsigned long long)entries[i * E], (unsigned long long)entries[i * E + 1],
              (unsigned long long)entries[i * E + 2], auc[i], slack[i]);
    fclose(f);
  }
  return XF_OK;
}

int Worker::create_holdout() {
  XF_TRY(check_holdout());
  if (holdout == 0.0f || split_) return XF_OK;
  XF_TRY(xf_holdout_create(&split_, holdout, seed));
  XF_TRY(xf_sharded_holdout(sharded_, 1));
  if (holdout_by_set) {
    XF_TRY(xf_slices_create(&gslicer_, (int32_t)holdout_by, xf::kSlicesMinLog2));
    XF_TRY(xf_sharded_gauc(sharded_, 1));
  }
  // the split's first launches, on two rows of a private object: start-up work like the two-row
  // update of create_tables (the worker's own object keeps its statistics clean)
  xf_holdout *warm = nullptr;
  XF_TRY(xf_holdout_create(&warm, holdout, seed));
  static const uint64_t rp[3] = {0, 2, 4}, keys[4] = {11, 12, 12, 13};
  static const int32_t lab[2] = {0, 1};
  void *stream = nullptr;
  int rc = xf_sharded_stream(sharded_, &stream);
  xf_holdout_part tr, he;
  if (rc == XF_OK)
    rc = xf_holdout_split(warm, 0, 0, rp, keys, nullptr, nullptr, lab, 0, 2, stream, &tr, &he);
  if (rc == XF_OK) rc = xf_stream_sync(stream);
  xf_holdout_destroy(warm);
  return rc;
}

// the held part of a training block: through the cross and through admission with update = 0
// (filtered, not counted, as test rows are), compiled with keep = 1 onto the held list — AFTER the
// block's train part has been compiled, so the filter has counted the block's train rows when it
// looks at the held ones (on a file of one block: the filter the test file will meet).  Only while
// the first epoch runs: an epoch that reads the text again drops it.  Without rows: no minibatch
// on one worker, the empty minibatch in a group.
int Worker::keep_held(const xf_holdout_part &held) {
  if (held_complete_ || (held.R == 0 && world <= 1)) return XF_OK;
  xf_sbatch *hb = nullptr;
  if (!held.d_rowptr && !admit_) {  // (a turn without rows of this rank's own)
    XF_TRY(compile_no_rows(sharded_, &hb, 1));
  } else {
    // (the rows' groups, named as the split hands them over: neither the cross nor admission adds
    // or removes rows, so the ids fit the minibatch compiled below)
    const uint64_t *ids = nullptr;
    if (gslicer_ && held.R && held.d_rowptr) {
      void *stream = nullptr;
      XF_TRY(xf_sharded_stream(sharded_, &stream));
      XF_TRY(xf_slices_extract_dev(gslicer_, held.d_keys, held.d_fgid, held.d_rowptr, held.R,
                                   held.NNZ, stream, &ids));
    }
    XF_TRY(compile_staged_dev(&hb, 0, held.d_keys, held.d_fgid, held.d_vals, held.d_rowptr,
                              held.d_labels, held.R, held.NNZ, 1));
    if (ids && hb) XF_TRY(xf_sbatch_set_slices(hb, ids, held.R));
  }
  if (hb) held_.push_back(hb);
  return XF_OK;
}

int Worker::split_dev(size_t first_row, const uint64_t **d_keys, const int32_t **d_fgid,
                      const float **d_vals, const uint32_t **d_rowptr, const int32_t **d_labels,
                      uint32_t *R, uint32_t *NNZ) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  xf_holdout_part tr, he;
  XF_TRY(xf_holdout_split_dev(split_, (uint64_t)(uint32_t)rank, ordinal_ + first_row, *d_keys,
                              fm_mode == XF_FM_FIELD_AWARE || cross_ || slicer_ || gslicer_
                                  ? *d_fgid : nullptr,
                              feature_values ? *d_vals : nullptr, *d_rowptr, *d_labels, *R, *NNZ,
                              stream, &tr, &he));
  pending_held_ = he;  // (the caller compiles the train part, then keep_held(pending_held_))
  train_block_first_ = train_ordinal_;
  train_ordinal_ += tr.R;
  *d_keys = tr.d_keys;
  *d_fgid = tr.d_fgid;
  *d_vals = tr.d_vals;
  *d_rowptr = tr.d_rowptr;
  *d_labels = tr.d_labels;
  *R = tr.R;
  *NNZ = tr.NNZ;
  return XF_OK;
}

// rows [start, end) of host arrays: uploaded by the split; the train part then takes the stages a
// sampled block takes (a train part without rows is a block without rows)
int Worker::compile_split(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                          const int32_t *fgid, const float *vals, const int32_t *labels,
                          size_t start, size_t end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  xf_holdout_part tr, he;
  XF_TRY(xf_holdout_split(split_, (uint64_t)(uint32_t)rank, ordinal_ + start, rowptr, keys,
                          fm_mode == XF_FM_FIELD_AWARE || cross_ || slicer_ || gslicer_ ? fgid
                                                                                         : nullptr,
                          feature_values ? vals : nullptr, labels, start, end, stream, &tr, &he));
  train_block_first_ = train_ordinal_;
  train_ordinal_ += tr.R;
  const uint64_t *dk = tr.d_keys;
  const int32_t *dfg = tr.d_fgid, *dl = tr.d_labels;
  const float *dv = tr.d_vals;
  const uint32_t *drp = tr.d_rowptr;
  uint32_t R = tr.R, NNZ = tr.NNZ;
  if (sample_) XF_TRY(sample_dev(0, &dk, &dfg, &dv, &drp, &dl, &R, &NNZ));
  XF_TRY(compile_sampled_dev(b, dk, dfg, dv, drp, dl, R, NNZ, keep));
  return keep_held(he);
}

// the end of an epoch, after the flush and before table maintenance: every holdout_every-th epoch
// and after the last one the held list is scored forward-only, the counts are summed over the
// ranks and reset, and rank 0 prints one line; then the early-stop rule, from the merged counts —
// every rank decides alike
int Worker::holdout_epoch(int epoch, bool last, bool *stop) {
  *stop = false;
  if (!split_) return XF_OK;
  held_complete_ = true;
  if ((epoch + 1) % holdout_every != 0 && !last) return XF_OK;
  for (xf_sbatch *hb : held_) XF_TRY(xf_sharded_validate(sharded_, hb));
  XF_TRY(xf_sharded_check(sharded_));
  std::vector<uint64_t> counts(2 * (size_t)XF_PROGRESS_RANKS);
  uint64_t other[2] = {0, 0};
  XF_TRY(xf_sharded_holdout_read(sharded_, counts.data(), other, 1, world > 1));
  XF_TRY(xf_progress_summary(counts.data(), other, 1.0f, &holdout_last_));  // (never weighted)
  if (holdout_curve_.empty()) holdout_first_ = holdout_last_;
  holdout_curve_.push_back(holdout_last_.logloss);
  holdout_epochs_.push_back(epoch);
  const xf_progress_metrics &m = holdout_last_;
  if (rank == 0) {
    char line[512];
    int at = snprintf(line, sizeof(line),
                      "holdout epoch %d: rows = %.12g logloss = %.6f (+- %.1e) auc = %.6f (+- %.1e) "
                      "ctr = %.6f pctr = %.6f", epoch, m.rows_pos + m.rows_neg, m.logloss,
                      m.logloss_bound, m.auc, m.auc_slack, m.ctr, m.pctr);
    if (m.saturated != 0 && at < (int)sizeof(line))
      at += snprintf(line + at, sizeof(line) - at, " saturated = %.17g", m.saturated);
    if (m.other != 0 && at < (int)sizeof(line))
      snprintf(line + at, sizeof(line) - at, " other = %.17g", m.other);
    std::cout << line << std::endl;
  }
  XF_TRY(gauc_epoch(epoch));
  int best = -1;
  const int s = xf_holdout_should_stop(holdout_curve_.data(), (int)holdout_curve_.size(),
                                       early_stop, early_stop_delta, &best);
  if (s && !last) {
    *stop = true;
    if (rank == 0) {
      char line[256];
      snprintf(line, sizeof(line), "early stop after epoch %d: best epoch %d logloss = %.6f", epoch,
               best >= 0 ? holdout_epochs_[best] : -1, best >= 0 ? holdout_curve_[best] : NAN);
      std::cout << line << std::endl;
    }
  }
  return XF_OK;
}

int Worker::compile_sampled_dev(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                                const float *d_vals, const uint32_t *d_rowptr,
                                const int32_t *d_labels, uint32_t R, uint32_t NNZ, int keep) {
  *b = nullptr;
  if (R == 0 && world <= 1) return XF_OK;  // (every row dropped: a block without rows)
  return compile_staged_dev(b, 1, d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ, keep);
}

// Feature crosses add nonzeros to a block on the GPU ahead of the key build, from the nonzeros'
// field ids: core_num > 1 slices a block after it was read, the host key build and the
// reference-order forward take host arrays, and ingest=gpu hands out no fgid.  Every schedule and
// any number of workers: a rank crosses its own rows and the trainers see keys only.  All refused
// by name, before any rendezvous.
int Worker::check_cross() const {
  if (cross_spec.empty()) return XF_OK;
  int32_t fa[32], fb[32];
  int npairs = 0;
  XF_TRY(xf_cross_parse(cross_spec.c_str(), fa, fb, 32, &npairs));
  XF_REQUIRE(core_num <= 1, "XFStartTrain: cross=%s needs core_num=1, not core_num=%d",
             cross_spec.c_str(), core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: cross=%s together with key_build=host: the crossed "
             "minibatch is born on the GPU (use key_build=gpu)", cross_spec.c_str());
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: cross=%s together with "
             "parity=reference_order: that mode builds its keys on the host", cross_spec.c_str());
  XF_REQUIRE(!ingest_gpu, "XFStartTrain: cross=%s together with ingest=gpu: the GPU tokeniser "
             "hands out no fgid (use ingest=gpu_fields)", cross_spec.c_str());
  if (fm_mode == XF_FM_FIELD_AWARE)
    XF_REQUIRE(cross_fgid_base >= 0 && (long)cross_fgid_base + npairs <= (long)fields,
               "XFStartTrain: cross_fgid_base=%d with %d pairs needs fields >= %ld, not fields=%d "
               "(fm_mode=field_aware: a crossed nonzero's fgid is cross_fgid_base + its pair's "
               "index)", cross_fgid_base, npairs, (long)cross_fgid_base + npairs, fields);
  return XF_OK;
}

int Worker::create_cross() {
  if (cross_spec.empty() || cross_) return XF_OK;
  XF_TRY(check_cross());
  int32_t fa[32], fb[32];
  int npairs = 0;
  XF_TRY(xf_cross_parse(cross_spec.c_str(), fa, fb, 32, &npairs));
  // (the base is read only with fm_mode=field_aware: no other mode looks at a nonzero's fgid)
  const int32_t base = fm_mode == XF_FM_FIELD_AWARE ? cross_fgid_base : 0;
  XF_TRY(xf_cross_create(&cross_, fa, fb, npairs, base));
  // the stage's first launches, on two rows of a private stage: start-up work like the two-row
  // update of create_tables (the worker's own stage keeps its statistics clean)
  xf_cross *warm = nullptr;
  XF_TRY(xf_cross_create(&warm, fa, fb, npairs, base));
  const uint64_t rp[3] = {0, 2, 4}, keys[4] = {11, 12, 12, 13};
  const int32_t fg[4] = {fa[0], fb[0], fa[0], fb[0]};
  void *stream = nullptr;
  int rc = xf_sharded_stream(sharded_, &stream);
  const uint64_t *fk = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, NNZ = 0;
  if (rc == XF_OK)
    rc = xf_cross_apply(warm, rp, keys, fg, nullptr, nullptr, 0, 2, stream, 0, &fk, nullptr,
                        nullptr, &fr, nullptr, &R, &NNZ);
  if (rc == XF_OK) rc = xf_stream_sync(stream);
  xf_cross_destroy(warm);
  return rc;
}

// Row normalisation rescales a minibatch's values on the GPU immediately ahead of the key build:
// without feature values there is nothing to scale, core_num > 1 slices a block after it was
// read, and the host key build and the reference-order forward take host arrays.  All refused by
// name, before any rendezvous.
int Worker::check_rownorm() const {
  if (!row_norm) return XF_OK;
  XF_REQUIRE(feature_values, "XFStartTrain: row_norm=l2 needs feature_values=on: without values "
             "every nonzero is 1 and a row has nothing to scale");
  XF_REQUIRE(core_num <= 1, "XFStartTrain: row_norm=l2 needs core_num=1, not core_num=%d",
             core_num);
  XF_REQUIRE(key_build_gpu, "XFStartTrain: row_norm=l2 together with key_build=host: the "
             "normalised minibatch is born on the GPU (use key_build=gpu)");
  XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS, "XFStartTrain: row_norm=l2 together with "
             "parity=reference_order: that mode builds its keys on the host");
  return XF_OK;
}

int Worker::create_rownorm() {
  if (!row_norm || norm_) return XF_OK;
  XF_TRY(check_rownorm());
  XF_TRY(xf_rownorm_create(&norm_, XF_ROWNORM_L2));
  // the stage's first launch, on two rows of a private stage: start-up work like the two-row
  // update of create_tables (the worker's own stage keeps its statistics clean)
  xf_rownorm *warm = nullptr;
  XF_TRY(xf_rownorm_create(&warm, XF_ROWNORM_L2));
  static const uint64_t rp[3] = {0, 2, 4}, keys[4] = {11, 12, 12, 13};
  static const float vals[4] = {1.0f, 0.5f, 0.25f, 2.0f};
  void *stream = nullptr;
  int rc = xf_sharded_stream(sharded_, &stream);
  const uint64_t *fk = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, NNZ = 0;
  if (rc == XF_OK)
    rc = xf_rownorm_apply(warm, rp, keys, nullptr, vals, nullptr, 0, 2, stream, &fk, nullptr, &fv,
                          &fr, nullptr, &R, &NNZ, nullptr);
  if (rc == XF_OK) rc = xf_stream_sync(stream);
  xf_rownorm_destroy(warm);
  return rc;
}

// rows [start, end) of host arrays through row normalisation alone: uploaded by the stage, then
// the _dev compile of the worker's mode
int Worker::compile_normed(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                           const int32_t *fgid, const float *vals, const int32_t *labels,
                           size_t start, size_t end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *fk = nullptr;
  const int32_t *ff = nullptr, *fl = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, NNZ = 0;
  XF_TRY(xf_rownorm_apply(norm_, rowptr, keys, fm_mode == XF_FM_FIELD_AWARE ? fgid : nullptr, vals,
                          labels, start, end, stream, &fk, &ff, &fv, &fr, &fl, &R, &NNZ, nullptr));
  return compile_dev_mode(b, fk, ff, fv, fr, fl, R, NNZ, keep);
}

// the stages that follow sampling, on device arrays: the cross, when on (a block without rows has
// nothing to cross), admission, when on, and the _dev compile of the worker's mode
int Worker::compile_staged_dev(xf_sbatch **b, int update, const uint64_t *d_keys,
                               const int32_t *d_fgid, const float *d_vals,
                               const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                               uint32_t NNZ, int keep) {
  // (training blocks only: the rows' slices, named before the cross adds its nonzeros; neither
  // the cross nor admission drops or reorders rows, so the ids fit the minibatch compiled below)
  const uint64_t *ids = nullptr;
  const uint32_t id_rows = R;
  if (slicer_ && update && R) {
    void *stream = nullptr;
    XF_TRY(xf_sharded_stream(sharded_, &stream));
    XF_TRY(xf_slices_extract_dev(slicer_, d_keys, d_fgid, d_rowptr, R, NNZ, stream, &ids));
  }
  if (cross_ && R) {
    void *stream = nullptr;
    XF_TRY(xf_sharded_stream(sharded_, &stream));
    const int32_t *ff = nullptr;
    const float *fv = nullptr;
    XF_TRY(xf_cross_apply_dev(cross_, d_keys, d_fgid, feature_values ? d_vals : nullptr, d_rowptr,
                              R, NNZ, stream, fm_mode == XF_FM_FIELD_AWARE, &d_keys, &ff, &fv,
                              &d_rowptr, &NNZ));
    d_fgid = ff;
    d_vals = fv;
  }
  if (admit_)
    XF_TRY(compile_admitted_dev(b, update, d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ,
                                keep));
  else
    XF_TRY(compile_dev_arrays(b, d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ, keep));
  if (ids && *b) XF_TRY(xf_sbatch_set_slices(*b, ids, id_rows));
  return XF_OK;
}

// rows [start, end) of host arrays through the cross: uploaded by the stage, then as above
int Worker::compile_crossed(xf_sbatch **b, int update, const uint64_t *rowptr,
                            const uint64_t *keys, const int32_t *fgid, const float *vals,
                            const int32_t *labels, size_t start, size_t end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *fk = nullptr;
  const int32_t *ff = nullptr, *fl = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, NNZ = 0;
  XF_TRY(xf_cross_apply(cross_, rowptr, keys, fgid, feature_values ? vals : nullptr, labels, start,
                        end, stream, fm_mode == XF_FM_FIELD_AWARE, &fk, &ff, &fv, &fr, &fl, &R,
                        &NNZ));
  if (admit_) return compile_admitted_dev(b, update, fk, ff, fv, fr, fl, R, NNZ, keep);
  return compile_dev_arrays(b, fk, ff, fv, fr, fl, R, NNZ, keep);
}

int Worker::compile_sampled(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                            const int32_t *fgid, const float *vals, const int32_t *labels,
                            size_t start, size_t end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *fk = nullptr;
  const int32_t *ff = nullptr, *fl = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, NNZ = 0;
  XF_TRY(xf_negsample_apply(sample_, sample_stream_, ordinal_ + start, rowptr, keys,
                            fm_mode == XF_FM_FIELD_AWARE || cross_ || slicer_ ? fgid : nullptr,
                            feature_values ? vals : nullptr, labels, start, end, stream, &fk, &ff,
                            &fv, &fr, &fl, &R, &NNZ));
  return compile_sampled_dev(b, fk, ff, fv, fr, fl, R, NNZ, keep);
}

// a rank without rows of its own still takes part in the (collective) step: the empty minibatch
int Worker::compile_no_rows(xf_sharded *trainer, xf_sbatch **b, int keep) {
  static const uint64_t kNoRows[1] = {0};
  return xf_sharded_compile(trainer, b, kNoRows, nullptr, (const int32_t *)kNoRows, 0, 0, keep);
}

// the compile of the worker's mode on rows [start, end) of a block's host arrays (fgid and vals
// are looked at only in the modes that read them); update: the admission filter counts the keys
int Worker::compile_rows(xf_sharded *trainer, xf_sbatch **b, int update, const uint64_t *rowptr,
                         const uint64_t *keys, const int32_t *fgid, const float *vals,
                         const int32_t *labels, size_t start, size_t end, int keep) {
  // (sliced progressive validation: training rows of this rank's own.  Under negative subsampling
  // the block is on the device when its rows are named — compile_staged_dev; otherwise here)
  // (held-out validation: a training block of this rank's own is split first, on the device; in
  // a group a turn without rows still adds the empty minibatch to the held list, so that every
  // rank validates equally often)
  if (split_ && update && trainer == sharded_) {
    if (rowptr && end > start)
      return compile_split(b, rowptr, keys, fgid, vals, labels, start, end, keep);
    if (world > 1) {  // (the train part first, as compile_split does)
      XF_TRY(compile_rows_unsliced(trainer, b, update, rowptr, keys, fgid, vals, labels, start, end,
                                   keep));
      return keep_held(xf_holdout_part{});
    }
  }
  if (slicer_ && !sample_ && update && trainer == sharded_ && rowptr && end > start)
    return compile_sliced(b, rowptr, keys, fgid, vals, labels, start, end, keep);
  return compile_rows_unsliced(trainer, b, update, rowptr, keys, fgid, vals, labels, start, end,
                               keep);
}

int Worker::compile_sliced(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                           const int32_t *fgid, const float *vals, const int32_t *labels,
                           size_t start, size_t end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *ids = nullptr;
  uint32_t R = 0;
  XF_TRY(xf_slices_extract(slicer_, rowptr, keys, fgid, start, end, stream, &ids, &R));
  XF_TRY(compile_rows_unsliced(sharded_, b, 1, rowptr, keys, fgid, vals, labels, start, end, keep));
  if (*b) XF_TRY(xf_sbatch_set_slices(*b, ids, R));
  return XF_OK;
}

int Worker::compile_rows_unsliced(xf_sharded *trainer, xf_sbatch **b, int update,
                                  const uint64_t *rowptr, const uint64_t *keys, const int32_t *fgid,
                                  const float *vals, const int32_t *labels, size_t start,
                                  size_t end, int keep) {
  // (training blocks only — predict passes update 0 — and only rows of this rank's own)
  if (sample_ && update && trainer == sharded_ && rowptr && end > start)
    return compile_sampled(b, rowptr, keys, fgid, vals, labels, start, end, keep);
  // (rows of this rank's own, training and predict; a rank without rows has nothing to cross)
  if (cross_ && trainer == sharded_ && rowptr && end > start)
    return compile_crossed(b, update, rowptr, keys, fgid, vals, labels, start, end, keep);
  if (admit_ && trainer == sharded_) {  // (core_num 1: filtered, compiled from device arrays)
    // (a rank without rows of its own — a shared filter — is in the collective apply all the same)
    if (!rowptr)
      return compile_admitted_dev(b, update, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                                  keep);
    return compile_admitted(b, update, rowptr, keys, fgid, vals, labels, start, end, keep);
  }
  // (row normalisation with no other stage on: rows of this rank's own, training and predict)
  if (norm_ && trainer == sharded_ && rowptr && end > start)
    return compile_normed(b, rowptr, keys, fgid, vals, labels, start, end, keep);
  if (fm_mode == XF_FM_FIELD_AWARE)
    return xf_sharded_compile_fielded(trainer, b, rowptr, keys, fgid,
                                      feature_values ? vals : nullptr, labels, start, end, keep);
  if (feature_values)
    return xf_sharded_compile_valued(trainer, b, rowptr, keys, vals, labels, start, end, keep);
  if (end > start)
    return xf_sharded_compile(trainer, b, rowptr, keys, labels, start, end, keep);
  return compile_no_rows(trainer, b, keep);
}

// row normalisation, when on — the last stage, over the nonzeros the model receives — and the _dev
// compile of the worker's mode on device arrays
int Worker::compile_dev_arrays(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                               const float *d_vals, const uint32_t *d_rowptr,
                               const int32_t *d_labels, uint32_t R, uint32_t NNZ, int keep) {
  if (norm_ && R) {
    void *stream = nullptr;
    XF_TRY(xf_sharded_stream(sharded_, &stream));
    XF_TRY(xf_rownorm_apply_dev(norm_, d_vals, d_rowptr, R, NNZ, stream, &d_vals, nullptr));
  }
  return compile_dev_mode(b, d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ, keep);
}

int Worker::compile_dev_mode(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                             const float *d_vals, const uint32_t *d_rowptr,
                             const int32_t *d_labels, uint32_t R, uint32_t NNZ, int keep) {
  if (fm_mode == XF_FM_FIELD_AWARE)
    return xf_sharded_compile_fielded_dev(sharded_, b, d_keys, d_fgid,
                                          feature_values ? d_vals : nullptr, d_rowptr, d_labels, R,
                                          NNZ, keep);
  if (feature_values)
    return xf_sharded_compile_valued_dev(sharded_, b, d_keys, d_vals, d_rowptr, d_labels, R, NNZ,
                                         keep);
  return xf_sharded_compile_dev(sharded_, b, d_keys, d_rowptr, d_labels, R, NNZ, keep);
}

int Worker::compile_admitted_dev(xf_sbatch **b, int update, const uint64_t *d_keys,
                                 const int32_t *d_fgid, const float *d_vals,
                                 const uint32_t *d_rowptr, const int32_t *d_labels, uint32_t R,
                                 uint32_t NNZ, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *fk = nullptr;
  const int32_t *ff = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t kept = 0;
  XF_TRY(xf_admit_apply_dev(admit_, update, d_keys,
                            fm_mode == XF_FM_FIELD_AWARE ? d_fgid : nullptr,
                            feature_values ? d_vals : nullptr, d_rowptr, R, NNZ, stream, &fk, &ff,
                            &fv, &fr, &kept));
  return compile_dev_arrays(b, fk, ff, fv, fr, d_labels, R, kept, keep);
}

int Worker::compile_admitted(xf_sbatch **b, int update, const uint64_t *rowptr,
                             const uint64_t *keys, const int32_t *fgid, const float *vals,
                             const int32_t *labels, size_t row_begin, size_t row_end, int keep) {
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  const uint64_t *fk = nullptr;
  const int32_t *ff = nullptr, *fl = nullptr;
  const float *fv = nullptr;
  const uint32_t *fr = nullptr;
  uint32_t R = 0, kept = 0;
  XF_TRY(xf_admit_apply(admit_, update, rowptr, keys,
                        fm_mode == XF_FM_FIELD_AWARE ? fgid : nullptr,
                        feature_values ? vals : nullptr, labels, row_begin, row_end, stream, &fk,
                        &ff, &fv, &fr, &fl, &R, &kept));
  return compile_dev_arrays(b, fk, ff, fv, fr, fl, R, kept, keep);
}

// ingest = gpu_fields: what the tokeniser reads beside the fid is what the model needs — fgid for
// field-aware FM, the third field with feature values; neither: the tokeniser of ingest = gpu
int Worker::set_ingest_fields(xf_ingest *g) {
  return xf_ingest_set_fields(g, ingest_fields && (fm_mode == XF_FM_FIELD_AWARE ||
                                                   !cross_spec.empty() || progress_by_set ||
                                                   holdout_by_set),
                              ingest_fields && feature_values);
}

// ingest = gpu: the two staging buffers (pinning 2 x block_size of host memory costs tens of ms)
// and the tokeniser's first launches: start-up work like the two-row update of create_tables
int Worker::start_ingest() {
  if (!gpu_ingest_applies()) return XF_OK;  // (nothing is pinned for a path that will not run)
  for (int i = 0; i < 2; ++i) {
    if (!ingest_[i] && xf_ingest_create(&ingest_[i], (size_t)block_size << 20) != XF_OK) {
      // (a block size the tokeniser does not take, or no memory to pin: the host parser's run)
      fprintf(stderr, "xflow_amd: ingest=%s is not available (%s): the host parser reads the text\n",
              ingest_fields ? "gpu_fields" : "gpu", xf_last_error());
      ingest_gpu = ingest_fields = false;
      return XF_OK;
    }
    XF_TRY(set_ingest_fields(ingest_[i]));
  }
  static const char two_rows[] = "0\t1:2:0.5 3:4:1\n1\t5:6:0.25\n";
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  uint32_t R = 0, NNZ = 0;
  int ok = 0;
  return xf_ingest_block(ingest_[0], two_rows, sizeof(two_rows) - 1, stream, nullptr, nullptr,
                         nullptr, &R, &NNZ, &ok);
}

// percent: settle the table when more than that share of its keys has arrived since the last
// time (5 at the epoch boundaries; inside the first epoch, one worker: 30 — the key build of
// the blocks still to come finds settled keys where they sit in LDS, arrival keys by a probe
// per nonzero, and a defrag is a sort of the table's keys)
int Worker::defrag_if_grown(int percent) {
  uint64_t n = 0, settled = 0;
  XF_TRY(xf_table_size(table_w_, &n));
  // (the settled tier as the table reports it: the first minibatch's build may have settled the
  // table already)
  XF_TRY(xf_table_settled(table_w_, &settled));
  settled = std::min(n, settled);
  const uint64_t arrived = n - settled, fresh = n - std::min(n, keys_seen_);
  keys_seen_ = n;
  // grown by `percent` since the table was last settled — or (inside an epoch) the inflow has
  // stopped: the last minibatch brought less than 0.1 % new keys while more than 0.5 % of the
  // table's keys still sit in the arrival index, where every minibatch that meets them pays the
  // first-touch path for them (measured, DESIGN 3: a defrag of 1e7 keys 1.1 ms, the path ~0.15 ms
  // per minibatch at 14 % unsettled keys)
  const bool grown = n > settled + settled / 100 * percent + (percent > 5 ? 4096 : 0);
  const bool settled_down = percent > 5 && arrived * 200 > n && fresh * 1000 < n && arrived > 4096;
  if (grown || settled_down) XF_TRY(xf_sharded_defrag(sharded_));
  return XF_OK;
}

// "does any rank still have a block?" — the ranks' files differ in length, the steps are
// collective: a rank that has run out keeps stepping empty minibatches until all are done
int Worker::any_rank(bool mine, bool *any) {
  *any = mine;
  if (world <= 1) return XF_OK;
  const int32_t flag = mine ? 1 : 0;
  std::vector<int32_t> all(world);
  XF_TRY(xf_group_allgather_host(group_, &flag, 4, all.data()));
  for (int32_t f : all)
    if (f) *any = true;
  return XF_OK;
}

int Worker::open_reader(xf_reader **rd, const char *path, size_t cap, bool *writes_cache) {
  if (writes_cache) *writes_cache = false;
  if (!block_cache) return xf_reader_open(rd, path, cap);
  std::string base = path;
  if (!block_cache_dir.empty()) {
    const size_t slash = base.find_last_of('/');
    base = block_cache_dir + "/" + (slash == std::string::npos ? base : base.substr(slash + 1));
  }
  const std::string cpath = base + ".xfcsr" + std::to_string(cap);
  int from_cache = 0;
  XF_TRY(xf_reader_open_cached(rd, path, cap, cpath.c_str(), &from_cache));
  if (writes_cache) *writes_cache = !from_cache;
  return XF_OK;
}

// batch_training (lr_worker.cc:179-205, fm_worker.cc:247-275)
int Worker::batch_training() {
  // init push of key 0 with a zero gradient (lr_worker.cc:180-182, fm_worker.cc:248-252): on
  // the shard that owns key 0
  if (xf_shard_of(0, (uint32_t)world) == (uint32_t)rank) {
    const uint64_t key0 = 0;
    const float zero = 0.0f;
    XF_TRY(xf_table_push(table_w_, &key0, 1, &zero));
    if (model_ == 1) {
      std::vector<float> zv(v_width(), 0.0f);
      XF_TRY(xf_table_push(table_v_, &key0, 1, zv.data()));
    }
  }
  // the builders' scratch arena for a block's worth of nonzeros (a token is at least four bytes of
  // text), sized before the clock starts instead of growing over the first blocks
  XF_TRY(xf_scratch_reserve(((size_t)block_size << 20) / 4 * 40 + ((size_t)64 << 20)));
  // ... and the first block's cells (4 bytes per nonzero, 8 when the minibatches are kept for
  // replay, + the cell offsets): set aside now, not mapped by the driver under the first build
  XF_TRY(xf_batch_pool_reserve(((size_t)block_size << 20) / 4 * 8 + ((size_t)16 << 20)));
  // ... and what the table's maintenance step inside the epoch (defrag_if_grown) would allocate
  if (world <= 1 && model_ == 0 && table_w_) XF_TRY(xf_table_prepare_defrag(table_w_));
  const double t0 = now_s();
  rows_trained_ = 0;
  blocks_gpu = blocks_host = 0;
  evict_seen_ = evict_dropped_ = 0;
  for (xf_sbatch *b : cache_) xf_sbatch_free(b);  // a second XFStartTrain starts from the files
  cache_.clear();
  for (xf_sbatch *b : held_) xf_sbatch_free(b);
  held_.clear();
  held_complete_ = false;
  holdout_curve_.clear();
  holdout_epochs_.clear();
  epochs_run_ = 0;
  bool cached = false;
  // compiled minibatches are kept in HBM for the epochs that replay them — with one epoch
  // there is none: the batches are one-shot (no key-sorted copy, their blobs go back to the pool)
  const int keep = cache_batches != 0 && epochs > 1;
  for (int epoch = 0; epoch < epochs; ++epoch) {
    if (cached) {
      // The compiled batches depend only on the file, so later epochs replay them from
      // HBM instead of re-reading and re-sorting the text (the reference re-opens and
      // re-parses per epoch, lr_worker.cc:184).  Every rank holds the same number of them.
      for (xf_sbatch *b : cache_) {
        XF_TRY(xf_sharded_step(sharded_, b));
        uint32_t R = 0;
        xf_sbatch_dims(b, &R, nullptr, nullptr, nullptr);
        rows_trained_ += R;
      }
      XF_TRY(xf_sharded_check(sharded_));
    } else {
      // ingest = gpu: the text tokenised and hashed on the GPU (xf_ingest.hip), compiled from
      // device arrays — unless this rank's shard file cannot be mapped (empty, not a regular
      // file): the host reader below yields zero rows for such a file and the rank still joins
      // every collective with empty minibatches
      // (negative subsampling: this epoch's stream of decisions, the file's rows numbered from 0)
      ordinal_ = train_ordinal_ = 0;
      sample_stream_ = (uint64_t)epoch << 32 | (uint32_t)rank;
      bool took = false;
      if (gpu_ingest_applies()) XF_TRY(text_epoch(epoch, keep, &took));
      if (took) {
        cached = keep != 0;
        goto epoch_done;
      }
      xf_reader *rd = nullptr;
      const bool trace = getenv("XF_TRACE_WORKER") != nullptr;  // per-block timeline on stderr
      const double te0 = now_s();
      bool writes_cache = false;
      XF_TRY(open_reader(&rd, train_data_path, (size_t)block_size << 20, &writes_cache));
      if (feature_values && xf_reader_set_values(rd, 1) != XF_OK) {
        xf_reader_close(rd);
        return XF_EINVAL;
      }
      if (trace) fprintf(stderr, "epoch %d: reader open %.2f ms\n", epoch, (now_s() - te0) * 1e3);
      // The text of block i+1 is parsed on a second host thread while the GPU builds the keys
      // of block i and trains on it: two caller-owned blocks go round between the two threads.
      struct Parsed {
        xf_block *blk = nullptr;
        size_t rows = 0, nnz = 0;
        const uint64_t *rowptr = nullptr, *keys = nullptr;
        const int32_t *labels = nullptr;
        const int32_t *fgid = nullptr;  // (fm_mode = field_aware)
        const float *vals = nullptr;  // (feature_values)
        int rc = XF_OK;
        std::string err;
      };
      Parsed slot[2];
      const Parsed none;  // (a rank whose file has ended: no arrays)
      for (int i = 0; i < 2; ++i) {
        int rc = blocks_[i] ? XF_OK : xf_block_create(&blocks_[i]);
        if (rc != XF_OK) {
          xf_reader_close(rd);
          return rc;
        }
        slot[i].blk = blocks_[i];
      }
      std::mutex mu;
      std::condition_variable cv;
      int filled[2] = {0, 0};  // 0 = free for the parser, 1 = parsed, waiting for the trainer
      bool stop = false;
      int trainer_dev = 0;
      (void)hipGetDevice(&trainer_dev);
      std::thread parser([&, trainer_dev] {
        // the block arrays are page-locked by this thread: on the trainer's GPU, not on
        // device 0 (the current device is per thread; every rank of a node would otherwise
        // create a context on GPU 0)
        (void)hipSetDevice(trainer_dev);
        for (int k = 0;; k ^= 1) {
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || !filled[k]; });
            if (stop) return;
          }
          Parsed &p = slot[k];
          p.rc = xf_reader_next_into(rd, p.blk, &p.rows, &p.nnz, &p.rowptr, &p.keys, &p.fgid,
                                     &p.labels);
          if (p.rc == XF_OK && feature_values) p.rc = xf_block_values(p.blk, &p.vals);
          if (p.rc != XF_OK) p.err = xf_last_error();  // the message is thread-local
          const bool last = p.rc != XF_OK || p.rows == 0;
          {
            std::lock_guard<std::mutex> lk(mu);
            filled[k] = 1;
          }
          cv.notify_all();
          if (last) return;
        }
      });
      int rc = XF_OK;
      bool mine_done = false;
      for (int k = 0; rc == XF_OK;) {
        Parsed *p = nullptr;
        const double tw0 = now_s();
        if (!mine_done) {
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return filled[k] != 0; });
          }
          p = &slot[k];
          if (p->rc != XF_OK) {
            rc = xf::set_error(p->rc, "%s", p->err.c_str());
            break;  // (a parse error ends this rank; its peers time out on the next exchange)
          }
          if (p->rows == 0) mine_done = true;
        }
        bool any = false;
        rc = any_rank(!mine_done, &any);
        if (rc != XF_OK || !any) break;
        const size_t rows = mine_done ? 0 : p->rows;
        const double tw1 = now_s();
        double t_compile = 0, t_step = 0;
        const size_t thread_size = rows / core_num;  // remainder dropped, lr_worker.cc:190
        for (int i = 0; i < core_num && rc == XF_OK; ++i) {
          const size_t start = i * thread_size, end = (i + 1) * thread_size;
          if (end == start && world <= 1) continue;
          xf_sbatch *b = nullptr;
          const double tc0 = now_s();
          // a rank without rows of its own still takes part in the (collective) step
          const Parsed &m = p ? *p : none;
          rc = compile_rows(sharded_, &b, 1, m.rowptr, m.keys, m.fgid, m.vals, m.labels, start, end,
                            keep);
          if (rc != XF_OK) break;
          const double tc1 = now_s();
          // (b == nullptr: negative subsampling dropped every row of the block — no minibatch)
          if (b) rc = xf_sharded_step(sharded_, b);
          if (rc == XF_OK) rc = xf_sharded_check(sharded_);
          t_compile += tc1 - tc0;
          t_step += now_s() - tc1;
          if (rc != XF_OK) {
            if (b) xf_sbatch_free(b);
            break;
          }
          uint32_t kept_rows = 0;  // (under negative subsampling: the kept rows)
          if (b) xf_sbatch_dims(b, &kept_rows, nullptr, nullptr, nullptr);
          rows_trained_ += sample_ || split_ ? (long)kept_rows : (long)(end - start);
          if (keep && b) cache_.push_back(b);
          else if (b)
            xf_sbatch_free(b);
        }
        ordinal_ += rows;
        // (the table's maintenance step inside an epoch: local to the shard, but its flush is
        // collective — one worker only)
        if (rc == XF_OK && world <= 1 && model_ == 0) rc = defrag_if_grown(30);
        if (trace)
          fprintf(stderr, "block: %zu rows  waited for the parser %.2f ms  key build %.2f ms  "
                  "step+check %.2f ms\n", rows, (tw1 - tw0) * 1e3, t_compile * 1e3, t_step * 1e3);
        if (!mine_done) {
          {
            std::lock_guard<std::mutex> lk(mu);
            filled[k] = 0;
          }
          cv.notify_all();
          k ^= 1;
        }
      }
      const double te1 = now_s();
      {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
      }
      cv.notify_all();
      parser.join();
      // unmapping a GB of text takes tens of ms: not on the training loop's clock (a reader
      // that is writing the block cache finishes the file when it closes: that one now)
      if (writes_cache) xf_reader_close(rd);
      else
      {
        for (std::thread &t : closers_) t.join();  // (the previous epoch's: long done)
        closers_.clear();
        closers_.emplace_back([rd] { xf_reader_close(rd); });
      }
      if (trace)
        fprintf(stderr, "epoch %d: blocks done after %.2f ms, reader and block buffers released "
                "in %.2f ms\n", epoch, (te1 - te0) * 1e3, (now_s() - te1) * 1e3);
      if (rc != XF_OK) return rc;
      cached = keep != 0;
    }
  epoch_done:
    // table maintenance at the epoch boundary: when this epoch inserted a noticeable share of
    // the keys, renumber the state rows in key order for the epochs that replay them.  The
    // flush is collective (every rank, every epoch); the defrag itself is local to the shard.
    const double tf0 = now_s();
    XF_TRY(xf_sharded_flush(sharded_));
    XF_TRY(progress_epoch(epoch));
    XF_TRY(slices_epoch(epoch));
    // (holdout: the held list scored; an early stop makes this epoch the last one)
    bool stopped = false;
    XF_TRY(holdout_epoch(epoch, epoch + 1 == epochs, &stopped));
    const bool last = stopped || epoch + 1 == epochs;
    // (evict_n: the eviction settles the table itself; after the LAST epoch too, so that the
    // model that is saved and scored holds no evictable row)
    if (evict_n > 0.0f && ((epoch + 1) % evict_every == 0 || last))
      XF_TRY(evict_epoch(epoch));
    else if (!last)
      XF_TRY(defrag_if_grown(5));
    epochs_run_ = epoch + 1;
    if (getenv("XF_TRACE_WORKER"))
      fprintf(stderr, "epoch %d: flush + table maintenance %.2f ms\n", epoch, (now_s() - tf0) * 1e3);
    if ((epoch + 1) % 30 == 0) std::cout << "epoch : " << epoch << std::endl;  // :202
    if (stopped) break;
  }
  XF_TRY(xf_sharded_flush(sharded_));
  train_seconds_ = now_s() - t0;
  return XF_OK;
}

// One epoch from the text with the GPU tokeniser (ingest = gpu, gpu_fields).  A staging thread copies the
// next block's text from the mapped file into pinned memory (several host threads: a 64 MiB
// block is ~2 ms) while the GPU tokenises, compiles and steps the current one; two staging /
// tokeniser buffers go round between the two threads.  A block the tokeniser hands back (not of
// the common shape, xf_ingest.hip) is parsed from the staged text by the host parser: the same
// arrays, the reference's quirks in one place.  Block boundaries are the reader's (a1).
// the conditions of the GPU tokeniser's epoch that do not depend on the file
bool Worker::gpu_ingest_applies() const {
  return (ingest_gpu || ingest_fields) && core_num == 1 && !block_cache;
}

// *took = false: this rank's shard file is not a mapped regular file — nothing was done
int Worker::text_epoch(int epoch, int keep, bool *took) {
  *took = false;
  const bool trace = getenv("XF_TRACE_WORKER") != nullptr;
  const double te0 = now_s();
  xf_reader *rd = nullptr;
  XF_TRY(xf_reader_open(&rd, train_data_path, (size_t)block_size << 20));
  struct ReaderGuard {
    xf_reader *r;
    ~ReaderGuard() {
      if (r) xf_reader_close(r);
    }
  } rguard{rd};
  {
    int mapped = 0;
    XF_TRY(xf_reader_mapped(rd, &mapped));
    if (!mapped) return XF_OK;  // (xf_reader_peek_text / copy_text work on a mapping)
  }
  *took = true;
  // (the blocks the tokeniser hands back are parsed through this reader: with their values)
  if (feature_values) XF_TRY(xf_reader_set_values(rd, 1));
  const bool ffm = fm_mode == XF_FM_FIELD_AWARE;
  for (int i = 0; i < 2; ++i) {
    if (!ingest_[i]) XF_TRY(xf_ingest_create(&ingest_[i], (size_t)block_size << 20));
    XF_TRY(set_ingest_fields(ingest_[i]));
  }
  if (!blocks_[0]) XF_TRY(xf_block_create(&blocks_[0]));
  void *stream = nullptr;
  XF_TRY(xf_sharded_stream(sharded_, &stream));
  struct Staged {
    size_t len = 0;
    int rc = XF_OK;
    std::string err;
  } slot[2];
  std::mutex mu;
  std::condition_variable cv;
  int filled[2] = {0, 0};  // 0 = free for the staging thread, 1 = staged
  bool stop = false;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int copy_threads = std::max(2, std::min(16, xf::parse_threads()));
  std::thread stager([&, dev] {
    (void)hipSetDevice(dev);
    // the staged text goes up on this thread's own stream: the copy of block i + 1 (64 MiB: ~2.5 ms
    // of PCIe) runs while the GPU tokenises, compiles and steps block i
    hipStream_t up = nullptr;
    if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) up = nullptr;
    struct StreamGuard {
      hipStream_t s;
      ~StreamGuard() {
        if (s) {
          (void)hipStreamSynchronize(s);
          (void)hipStreamDestroy(s);
        }
      }
    } sguard{up};
    for (int k = 0;; k ^= 1) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !filled[k]; });
        if (stop) return;
      }
      Staged &p = slot[k];
      char *buf = nullptr;
      size_t cap = 0;
      p.len = 0;
      p.rc = xf_ingest_staging(ingest_[k], &buf, &cap);
      if (p.rc == XF_OK) p.rc = xf_reader_copy_text(rd, buf, cap, &p.len, copy_threads);
      if (p.rc == XF_OK && p.len) p.rc = xf_reader_skip_text(rd);
      if (p.rc == XF_OK && p.len && up) p.rc = xf_ingest_upload(ingest_[k], p.len, up);
      if (p.rc != XF_OK) p.err = xf_last_error();
      const bool last = p.rc != XF_OK || p.len == 0;
      {
        std::lock_guard<std::mutex> lk(mu);
        filled[k] = 1;
      }
      cv.notify_all();
      if (last) return;
    }
  });
  int rc = XF_OK;
  bool mine_done = false;
  for (int k = 0; rc == XF_OK;) {
    Staged *p = nullptr;
    const double tw0 = now_s();
    if (!mine_done) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return filled[k] != 0; });
      }
      p = &slot[k];
      if (p->rc != XF_OK) {
        rc = xf::set_error(p->rc, "%s", p->err.c_str());
        break;
      }
      if (p->len == 0) mine_done = true;
    }
    bool any = false;
    rc = any_rank(!mine_done, &any);
    if (rc != XF_OK || !any) break;
    const double tw1 = now_s();
    xf_sbatch *b = nullptr;
    size_t rows = 0;
    bool on_gpu = false;
    if (!mine_done) {
      const uint64_t *dk = nullptr;
      const uint32_t *drp = nullptr;
      const int32_t *dl = nullptr;
      uint32_t R = 0, NNZ = 0;
      int ok = 0;
      rc = xf_ingest_block(ingest_[k], nullptr, p->len, stream, &dk, &drp, &dl, &R, &NNZ, &ok);
      if (rc == XF_OK && ok) {
        const int32_t *dfg = nullptr;
        const float *dv = nullptr;
        rc = xf_ingest_fields(ingest_[k], &dfg, &dv);
        rows = R;
        if (rc == XF_OK && split_) rc = split_dev(0, &dk, &dfg, &dv, &drp, &dl, &R, &NNZ);
        if (rc == XF_OK && (sample_ || split_)) {
          if (sample_) rc = sample_dev(0, &dk, &dfg, &dv, &drp, &dl, &R, &NNZ);
          if (rc == XF_OK) rc = compile_sampled_dev(&b, dk, dfg, dv, drp, dl, R, NNZ, keep);
          if (rc == XF_OK && split_) rc = keep_held(pending_held_);
        } else if (rc == XF_OK)
          rc = compile_staged_dev(&b, 1, dk, dfg, dv, drp, dl, R, NNZ, keep);
        on_gpu = true;
        ++blocks_gpu;
      } else if (rc == XF_OK) {  // not of the common shape: the host parser's
        char *buf = nullptr;
        size_t nnz = 0;
        const uint64_t *rowptr = nullptr, *keys = nullptr;
        const int32_t *fgid = nullptr, *labels = nullptr;
        const float *vals = nullptr;
        rc = xf_ingest_staging(ingest_[k], &buf, nullptr);
        if (rc == XF_OK)
          rc = xf_reader_parse_text(rd, buf, p->len, blocks_[0], &rows, &nnz, &rowptr, &keys,
                                    &fgid, &labels);
        if (rc == XF_OK && feature_values) rc = xf_block_values(blocks_[0], &vals);
        // (under admission, with fields or with values, on one worker a block without rows is no
        // minibatch: b stays null; a plain one, and any of a group's turns, is the empty minibatch)
        if (rc == XF_OK && (rows || world > 1 || !(admit_ || ffm || feature_values)))
          rc = compile_rows(sharded_, &b, 1, rowptr, keys, fgid, vals, labels, 0, rows, keep);
        ++blocks_host;
      }
    } else {  // a rank without rows of its own still takes part in the (collective) step
      // (... and, with a shared admission filter, in the collective apply in front of it)
      rc = compile_rows(sharded_, &b, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, keep);
    }
    const double tc1 = now_s();
    if (rc == XF_OK && b) rc = xf_sharded_step(sharded_, b);
    if (rc == XF_OK) rc = xf_sharded_check(sharded_);
    if (rc != XF_OK) {
      if (b) xf_sbatch_free(b);
      break;
    }
    uint32_t kept_rows = 0;  // (under negative subsampling: the kept rows)
    if (b) xf_sbatch_dims(b, &kept_rows, nullptr, nullptr, nullptr);
    rows_trained_ += sample_ || split_ ? (long)kept_rows : (long)rows;
    ordinal_ += rows;
    if (keep && b) cache_.push_back(b);
    else if (b)
      xf_sbatch_free(b);
    if (world <= 1 && model_ == 0) rc = defrag_if_grown(30);
    if (trace)
      fprintf(stderr, "block: %zu rows  waited for the parser %.2f ms  key build %.2f ms  "
              "step+check %.2f ms  (%s)\n", rows, (tw1 - tw0) * 1e3, (tc1 - tw1) * 1e3,
              (now_s() - tc1) * 1e3, on_gpu ? "tokenised on the GPU" : "parsed on the host");
    if (!mine_done) {
      {
        std::lock_guard<std::mutex> lk(mu);
        filled[k] = 0;
      }
      cv.notify_all();
      k ^= 1;
    }
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  stager.join();
  if (trace)
    fprintf(stderr, "epoch %d: blocks done after %.2f ms (%ld tokenised on the GPU, %ld parsed on "
            "the host)\n", epoch, (now_s() - te0) * 1e3, blocks_gpu, blocks_host);
  return rc;
}

// predict + calculate_pctr (lr_worker.cc:25-98, fm_worker.cc:25-124).  As in the reference
// only rank 0 scores its test file (lr_worker.cc:212-215) — against the WHOLE table: the other
// ranks serve its Pulls (`reader` == false: they step empty minibatches until rank 0 is done).
int Worker::predict(int rank, int block, bool reader) {
  std::ofstream md;
  xf_reader *rd = nullptr;
  if (reader) {
    char name[1200];
    if (pred_path.empty()) snprintf(name, sizeof(name), "pred_%d_%d.txt", rank, block);
    else
      snprintf(name, sizeof(name), "%s", pred_path.c_str());
    md.open(name);
    if (!md.is_open()) std::cout << "open pred file failure!" << std::endl;
    snprintf(test_data_path, sizeof(test_data_path), "%s-%05d", test_file_path.c_str(), rank);
    // 4 MiB blocks for LR (lr_worker.cc:80), 2 MiB for FM (fm_worker.cc:106)
    const size_t cap = model_ == 0 ? ((size_t)4 << 20) : ((size_t)2 << 20);
    XF_TRY(open_reader(&rd, test_data_path, cap));
    if (feature_values && xf_reader_set_values(rd, 1) != XF_OK) {
      xf_reader_close(rd);
      return XF_EINVAL;
    }
  }
  struct ReaderGuard {  // every return path closes the reader
    xf_reader *r;
    ~ReaderGuard() {
      if (r) xf_reader_close(r);
    }
  } rd_guard{rd};
  std::vector<int32_t> all_labels;
  std::vector<float> all_pctr, pctr;
  bool mine_done = !reader;
  while (true) {
    size_t rows = 0, nnz = 0;
    const uint64_t *rowptr = nullptr, *keys = nullptr;
    const int32_t *fgid = nullptr, *labels = nullptr;
    const float *vals = nullptr;
    if (!mine_done) {
      XF_TRY(xf_reader_next(rd, &rows, &nnz, &rowptr, &keys, &fgid, &labels));
      if (feature_values) XF_TRY(xf_reader_values(rd, &vals));
      if (rows == 0) mine_done = true;
    }
    bool any = false;
    XF_TRY(any_rank(!mine_done, &any));
    if (!any) break;
    const size_t thread_size = rows / core_num;
    for (int i = 0; i < core_num; ++i) {
      const size_t start = i * thread_size, end = (i + 1) * thread_size;
      if (end == start && world <= 1) continue;
      xf_sbatch *b = nullptr;
      // (update 0: a key the admission filter has not admitted is neither scored nor inserted)
      XF_TRY(compile_rows(sharded_, &b, 0, rowptr, keys, fgid, vals, labels, start, end, 0));
      struct BatchGuard {  // ... and frees the minibatch
        xf_sbatch *b;
        ~BatchGuard() { xf_sbatch_free(b); }
      } b_guard{b};
      pctr.resize(end - start);
      XF_TRY(xf_sharded_predict(sharded_, b, pctr.data()));
      for (size_t r = 0; r < end - start; ++r) {
        const int label = labels[start + r];
        all_labels.push_back(label);
        all_pctr.push_back(pctr[r]);
        md << pctr[r] << "\t" << 1 - label << "\t" << label << std::endl;  // :67
      }
    }
  }
  XF_TRY(xf_sharded_check(sharded_));
  if (!reader) return XF_OK;
  md.close();
  // Base::calculate_auc (base.h:84-110) and its stdout line
  XF_TRY(xf_auc_logloss(all_labels.data(), all_pctr.data(), all_labels.size(), &logloss_acc_,
                        &auc_, &tp_, &fp_, &logloss_nat_));
  std::cout << "logloss: " << logloss_acc_ << "\t";
  if (isnan(auc_)) std::cout << "tp_n = " << tp_ << std::endl;
  else
    std::cout << "auc = " << auc_ << "\ttp = " << tp_ << " fp = " << fp_ << std::endl;
  return XF_OK;
}

// train (lr_worker.cc:207-217, fm_worker.cc:277-287)
int Worker::train() {
  if (fm_mode == XF_FM_CANONICAL && !sharded_) {  // before any rendezvous of a group
    XF_REQUIRE(model_ == 1, "XFStartTrain: fm_mode=canonical needs model 1 (FM), not model %d",
               model_);
    int w = world;
    if (w <= 0) {
      const char *v = env_first({"WORLD_SIZE", "XF_WORLD", "DMLC_NUM_WORKER"});
      w = v ? atoi(v) : 1;
    }
    XF_REQUIRE(w <= 1, "XFStartTrain: fm_mode=canonical runs on one worker only (world %d)", w);
    XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS,
               "XFStartTrain: fm_mode=canonical has no parity=reference_order mode");
  }
  if (fm_mode == XF_FM_FIELD_AWARE && !sharded_) {  // before any rendezvous of a group
    XF_REQUIRE(model_ == 1, "XFStartTrain: fm_mode=field_aware needs model 1 (FM), not model %d",
               model_);
    XF_REQUIRE(fields >= 1 && fields <= 64,
               "XFStartTrain: fm_mode=field_aware needs fields in 1 .. 64 (a key's touched fields "
               "are one 64-bit mask), not fields=%d", fields);
    XF_REQUIRE(v_dim_ >= 1 && (long)fields * v_dim_ <= 4096,
               "XFStartTrain: fm_mode=field_aware: fields x k = %d x %d exceeds 4096, the widest "
               "row of a table", fields, v_dim_);
    int w = world;
    if (w <= 0) {
      const char *v = env_first({"WORLD_SIZE", "XF_WORLD", "DMLC_NUM_WORKER"});
      w = v ? atoi(v) : 1;
    }
    XF_REQUIRE(w <= 1, "XFStartTrain: fm_mode=field_aware runs on one worker only (world %d)", w);
    XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS,
               "XFStartTrain: fm_mode=field_aware has no parity=reference_order mode");
    XF_REQUIRE(!ingest_gpu, "XFStartTrain: fm_mode=field_aware together with ingest=gpu: the GPU "
               "tokeniser hands out no fgid (use ingest=gpu_fields)");
  }
  if (feature_values && !sharded_) {  // next to the canonical mode's: before any rendezvous
    XF_REQUIRE(model_ == 0 || fm_mode != XF_FM_REFERENCE,
               "XFStartTrain: feature_values=on with model 1 (FM) needs fm_mode=canonical or "
               "field_aware (the reference form's pooled sums have no meaning with values)");
    int w = world;
    if (w <= 0) {
      const char *v = env_first({"WORLD_SIZE", "XF_WORLD", "DMLC_NUM_WORKER"});
      w = v ? atoi(v) : 1;
    }
    XF_REQUIRE(w <= 1, "XFStartTrain: feature_values=on runs on one worker only (world %d)", w);
    XF_REQUIRE(parity == XF_PARITY_EXACT_SUMS,
               "XFStartTrain: feature_values=on has no parity=reference_order mode");
    XF_REQUIRE(!block_cache, "XFStartTrain: feature_values=on together with block_cache=1: the "
               "block cache carries no values");
    XF_REQUIRE(!ingest_gpu, "XFStartTrain: feature_values=on together with ingest=gpu: the GPU "
               "tokeniser carries no values (use ingest=gpu_fields)");
  }
  XF_TRY(check_admit());  // before any rendezvous of a group
  XF_TRY(check_negsample());
  XF_TRY(check_gauc());  // (ahead of the holdout's own: the refusals they share name holdout_by)
  gauc_have_ = false;
  XF_TRY(check_holdout());
  XF_TRY(check_progress());
  progress_have_ = false;
  XF_TRY(check_slices());
  slices_have_ = false;
  XF_TRY(check_evict());
  XF_TRY(check_cross());
  XF_TRY(check_rownorm());
  XF_TRY(create_tables());
  XF_TRY(start_ingest());
  std::cout << "my rank is = " << rank << std::endl;
  snprintf(train_data_path, sizeof(train_data_path), "%s-%05d", train_file_path.c_str(), rank);
  if (!model_in.empty()) {  // resume from a model file (XFLoadModel)
    void *self = this;
    XF_TRY(XFLoadModel(self, model_in.c_str()));
  }
  XF_TRY(batch_training());
  if (norm_ && rank == 0) {  // (the training minibatches and the held ones; predict follows)
    uint64_t rows = 0, scaled = 0;
    XF_TRY(xf_rownorm_stats(norm_, &rows, &scaled));
    char line[160];
    snprintf(line, sizeof(line), "row_norm: rows = %llu scaled = %llu left = %llu",
             (unsigned long long)rows, (unsigned long long)scaled,
             (unsigned long long)(rows - scaled));
    std::cout << line << std::endl;
  }
  if (!model_out.empty()) {
    void *self = this;
    XF_TRY(XFSaveModel(self, model_out.c_str()));
  }
  if (rank == 0) std::cout << (model_ == 0 ? "LR AUC: " : "FM AUC: ") << std::endl;
  if (rank == 0 || world > 1) XF_TRY(predict(rank, 0, rank == 0));
  std::cout << "train end......" << std::endl;
  return XF_OK;
}

// one worker: one file at `path`; several: one file per shard + a manifest (xf_sharded_save)
int Worker::save_model(const char *path) {
  // the filter's counters beside the model; with admission off a file saved under the same name
  // earlier is stale, like the manifest below
  const std::string apath = std::string(path) + ".admit";
  if (admit_) XF_TRY(xf_admit_save(admit_, apath.c_str()));
  else
    (void)unlink(apath.c_str());
  if (world > 1) return xf_sharded_save(sharded_, path);
  XF_TRY(xf_sharded_flush(sharded_));
  XF_TRY(xf::model_write(path, table_w_, table_v_, v_width()));
  // a sharded checkpoint saved under the same name earlier is stale now: without this its
  // manifest would send a later load to the old shard files
  (void)unlink((std::string(path) + ".manifest").c_str());
  return XF_OK;
}

// a single file or a sharded checkpoint of ANY world size: every rank keeps the keys it owns
int Worker::load_model(const char *path) {
  XF_TRY(xf_sharded_load(sharded_, path));
  // with admission on the model comes with its filter (a missing file: XF_EIO naming it)
  if (admit_) XF_TRY(xf_admit_load(admit_, (std::string(path) + ".admit").c_str()));
  return XF_OK;
}

int Worker::set_param(const char *name, const char *value) {
  XF_REQUIRE(name && value, "XFSetParam: null argument");
  const std::string n = name;
  if (n == "model") {
    XF_REQUIRE(!sharded_, "XFSetParam: model cannot change after training started");
    model_ = atoi(value);
    XF_REQUIRE(model_ == 0 || model_ == 1, "XFSetParam: model must be 0 (LR) or 1 (FM)");
  } else if (n == "epochs") epochs = atoi(value);
  else if (n == "block_size_mb") block_size = atoi(value);
  else if (n == "core_num") core_num = atoi(value) > 0 ? atoi(value) : 1;
  else if (n == "k") v_dim_ = atoi(value);
  else if (n == "optimizer") {
    if (!strcmp(value, "ftrl")) optimizer = XF_OPT_FTRL;
    else if (!strcmp(value, "sgd")) optimizer = XF_OPT_SGD;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: optimizer must be ftrl or sgd");
  } else if (n == "capacity") capacity = strtoull(value, nullptr, 10);
  else if (n == "rank") {
    rank = atoi(value);
    rank_given_ = true;
  } else if (n == "world") world = atoi(value);
  else if (n == "transport") {
    if (!strcmp(value, "rccl")) transport = XF_TRANSPORT_RCCL;
    else if (!strcmp(value, "host")) transport = XF_TRANSPORT_HOST;
    else if (!strcmp(value, "auto")) transport = XF_TRANSPORT_AUTO;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: transport must be rccl, host or auto");
  } else if (n == "schedule") {
    if (!strcmp(value, "sequential")) schedule = XF_SCHEDULE_SEQUENTIAL;
    else if (!strcmp(value, "stale1")) schedule = XF_SCHEDULE_STALE1;
    else if (!strcmp(value, "owner")) schedule = XF_SCHEDULE_OWNER;
    else if (!strcmp(value, "owner_stale1")) schedule = XF_SCHEDULE_OWNER_STALE1;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: schedule must be sequential, stale1 or owner "
                           "(owner_stale1: the owner-compute dataflow, overlapped)");
  }
  else if (n == "pred_path") pred_path = value;
  else if (n == "alpha") alpha = (float)atof(value);
  else if (n == "beta") beta = (float)atof(value);
  else if (n == "lambda1") lambda1 = (float)atof(value);
  else if (n == "lambda2") lambda2 = (float)atof(value);
  else if (n == "lr") learning_rate = (float)atof(value);
  else if (n == "seed") seed = strtoull(value, nullptr, 10);
  else if (n == "cache_batches") cache_batches = atoi(value);
  else if (n == "parse_threads") return xf_tune("parse_threads", atof(value));
  else if (n == "ingest") {
    if (!strcmp(value, "gpu")) ingest_gpu = true, ingest_fields = false;
    else if (!strcmp(value, "gpu_fields")) ingest_gpu = false, ingest_fields = true;
    else if (!strcmp(value, "host")) ingest_gpu = ingest_fields = false;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: ingest must be gpu, gpu_fields or host");
  }
  else if (n == "block_cache") block_cache = atoi(value);
  else if (n == "block_cache_dir") block_cache_dir = value;
  else if (n == "model_in") model_in = value;
  else if (n == "model_out") model_out = value;
  else if (n == "update") {
    if (!strcmp(value, "rank_ordered")) update_rule = XF_UPDATE_RANK_ORDERED;
    else if (!strcmp(value, "sum_then_step")) update_rule = XF_UPDATE_SUM_THEN_STEP;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: update must be rank_ordered or sum_then_step");
  } else if (n == "parity") {
    if (!strcmp(value, "exact")) parity = XF_PARITY_EXACT_SUMS;
    else if (!strcmp(value, "reference_order")) parity = XF_PARITY_REFERENCE_ORDER;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: parity must be exact or reference_order");
  } else if (n == "fm_mode") {
    XF_REQUIRE(!sharded_, "XFSetParam: fm_mode cannot change after training started");
    if (!strcmp(value, "reference")) fm_mode = XF_FM_REFERENCE;
    else if (!strcmp(value, "canonical")) fm_mode = XF_FM_CANONICAL;
    else if (!strcmp(value, "field_aware")) fm_mode = XF_FM_FIELD_AWARE;
    else
      return xf::set_error(XF_EINVAL,
                           "XFSetParam: fm_mode must be reference, canonical or field_aware");
  } else if (n == "fields") {
    XF_REQUIRE(!sharded_, "XFSetParam: fields cannot change after training started");
    fields = atoi(value);
  } else if (n == "feature_values") {
    XF_REQUIRE(!sharded_, "XFSetParam: feature_values cannot change after training started");
    if (!strcmp(value, "on")) feature_values = true;
    else if (!strcmp(value, "off")) feature_values = false;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: feature_values must be on or off, not '%s'",
                           value);
  } else if (n == "neg_keep") {
    XF_REQUIRE(!sample_, "XFSetParam: neg_keep cannot change once the sampler exists");
    neg_keep = strtof(value, nullptr);
  } else if (n == "holdout") {
    XF_REQUIRE(!split_, "XFSetParam: holdout cannot change once the split stage exists");
    holdout = strtof(value, nullptr);
  } else if (n == "holdout_by") {
    XF_REQUIRE(!sharded_, "XFSetParam: holdout_by cannot change after training started");
    char *end = nullptr;
    const long long f = strtoll(value, &end, 10);
    XF_REQUIRE(end != value && *end == '\0', "XFSetParam: holdout_by must be a field id, not '%s'",
               value);
    holdout_by = f;
    holdout_by_set = true;
  } else if (n == "holdout_groups_out") {
    holdout_groups_out = value;
  } else if (n == "holdout_every") {
    holdout_every = atoi(value);
  } else if (n == "early_stop") {
    early_stop = atoi(value);
  } else if (n == "early_stop_delta") {
    early_stop_delta = strtod(value, nullptr);
  } else if (n == "progress") {
    XF_REQUIRE(!sharded_, "XFSetParam: progress cannot change after training started");
    XF_REQUIRE(!strcmp(value, "0") || !strcmp(value, "1"),
               "XFSetParam: progress must be 0 or 1, not %s", value);
    progress = atoi(value);
  } else if (n == "progress_by") {
    XF_REQUIRE(!sharded_, "XFSetParam: progress_by cannot change after training started");
    char *end = nullptr;
    const long long f = strtoll(value, &end, 10);
    XF_REQUIRE(end != value && *end == '\0', "XFSetParam: progress_by must be a field id, not '%s'",
               value);
    progress_by = f;
    progress_by_set = true;
  } else if (n == "progress_slots") {
    XF_REQUIRE(!sharded_, "XFSetParam: progress_slots cannot change after training started");
    progress_slots = atoi(value);
  } else if (n == "progress_top") {
    progress_top = atoi(value);
  } else if (n == "progress_slices_out") {
    progress_slices_out = value;
  } else if (n == "evict_n") {
    char *end = nullptr;
    const float x = strtof(value, &end);  // ("inf" parses: every zero-weight row goes)
    XF_REQUIRE(end != value && *end == '\0' && x >= 0.0f,
               "XFSetParam: evict_n must be 0 (off), a positive number or inf, not '%s'", value);
    evict_n = x;
  } else if (n == "evict_every") {
    XF_REQUIRE(atoi(value) >= 1, "XFSetParam: evict_every must be >= 1 (epochs), not %s", value);
    evict_every = atoi(value);
  } else if (n == "cross") {
    XF_REQUIRE(!cross_, "XFSetParam: cross cannot change once the stage exists");
    cross_spec = value;
  } else if (n == "row_norm") {
    const bool on = !strcmp(value, "l2");
    XF_REQUIRE(on || !strcmp(value, "off"), "XFSetParam: row_norm must be l2 or off, not '%s'",
               value);
    // (the stages are created with the tables: from then on the worker runs with or without one)
    XF_REQUIRE(!sharded_ || on == row_norm,
               "XFSetParam: row_norm cannot change once the stage exists");
    row_norm = on;
  } else if (n == "cross_fgid_base") {
    XF_REQUIRE(!cross_, "XFSetParam: cross_fgid_base cannot change once the stage exists");
    cross_fgid_base = atoi(value);
  } else if (n == "admit_count") {
    XF_REQUIRE(!admit_, "XFSetParam: admit_count cannot change once the filter exists");
    admit_count = atoi(value);
  } else if (n == "admit_log2_slots") {
    XF_REQUIRE(!admit_, "XFSetParam: admit_log2_slots cannot change once the filter exists");
    admit_log2_slots = atoi(value);
  } else if (n == "admit_shared") {
    XF_REQUIRE(!admit_, "XFSetParam: admit_shared cannot change once the filter exists");
    XF_REQUIRE(!strcmp(value, "0") || !strcmp(value, "1"),
               "XFSetParam: admit_shared must be 0 or 1, not %s", value);
    admit_shared = atoi(value);
  } else if (n == "admit_hashes") {
    XF_REQUIRE(!admit_, "XFSetParam: admit_hashes cannot change once the filter exists");
    admit_hashes = atoi(value);
  } else if (n == "key_build") {
    if (!strcmp(value, "gpu")) key_build_gpu = true;
    else if (!strcmp(value, "host")) key_build_gpu = false;
    else
      return xf::set_error(XF_EINVAL, "XFSetParam: key_build must be gpu or host");
  }
  else
    return xf::set_error(XF_EINVAL, "XFSetParam: unknown parameter '%s'", name);
  return XF_OK;
}

int Worker::get_metric(const char *name, double *value) {
  XF_REQUIRE(name && value, "XFGetMetric: null argument");
  const std::string n = name;
  if (n == "logloss_ref") *value = logloss_acc_;
  else if (n == "logloss_nat") *value = logloss_nat_;
  else if (n == "auc") *value = auc_;
  else if (n == "tp") *value = tp_;
  else if (n == "fp") *value = fp_;
  else if (n == "rows_trained") *value = (double)rows_trained_;
  else if (n == "blocks_gpu") *value = (double)blocks_gpu;
  else if (n == "blocks_host") *value = (double)blocks_host;
  else if (n == "neg_seen" || n == "neg_kept" || n == "rows_kept") {
    uint64_t rows_kept = 0, seen = 0, kept = 0;
    if (sample_) XF_TRY(xf_negsample_stats(sample_, nullptr, &rows_kept, &seen, &kept));
    *value = (double)(n == "neg_seen" ? seen : n == "neg_kept" ? kept : rows_kept);
  } else if (n == "slices" || n == "slice_rows" || n == "slice_none_rows" ||
             n == "slice_overflow_rows") {
    XF_REQUIRE(slices_have_, "XFGetMetric: %s: no epoch has been summarised (progress_by=F, after "
               "XFStartTrain)", name);
    *value = slices_last_[n == "slices" ? 0 : n == "slice_rows" ? 1 : n == "slice_none_rows" ? 2 : 3];
  } else if (n == "epochs_run") {
    *value = (double)epochs_run_;
  } else if (n == "holdout_gauc" || n == "holdout_gauc_slack" || n == "holdout_macro_auc" ||
             n == "holdout_groups" || n == "holdout_groups_scored" || n == "holdout_gauc_rows") {
    XF_REQUIRE(gauc_have_, "XFGetMetric: %s: no epoch has been reduced (holdout_by=F, after a "
               "validated epoch)", name);
    const xf_gauc_metrics &m = gauc_last_;
    *value = n == "holdout_gauc" ? m.gauc : n == "holdout_gauc_slack" ? m.gauc_slack
             : n == "holdout_macro_auc" ? m.macro_auc : n == "holdout_groups" ? (double)m.groups
             : n == "holdout_groups_scored" ? (double)m.groups_scored : (double)m.rows_scored;
  } else if (n.rfind("holdout_", 0) == 0) {
    XF_REQUIRE(!holdout_curve_.empty(), "XFGetMetric: %s: no epoch has been validated (holdout=r, "
               "after XFStartTrain)", name);
    const xf_progress_metrics &m = holdout_last_;
    int best = -1;
    xf_holdout_should_stop(holdout_curve_.data(), (int)holdout_curve_.size(), 0, early_stop_delta,
                           &best);
    if (n == "holdout_rows") *value = m.rows_pos + m.rows_neg;
    else if (n == "holdout_logloss") *value = m.logloss;
    else if (n == "holdout_auc") *value = m.auc;
    else if (n == "holdout_auc_slack") *value = m.auc_slack;
    else if (n == "holdout_ctr") *value = m.ctr;
    else if (n == "holdout_pctr") *value = m.pctr;
    else if (n == "holdout_logloss_first") *value = holdout_first_.logloss;
    else if (n == "holdout_best_epoch") *value = best >= 0 ? (double)holdout_epochs_[best] : -1.0;
    else if (n == "holdout_best_logloss") *value = best >= 0 ? holdout_curve_[best] : NAN;
    else
      return xf::set_error(XF_EINVAL, "XFGetMetric: unknown metric '%s'", name);
  } else if (n.rfind("progress_", 0) == 0) {
    const bool first = n.size() > 6 && n.compare(n.size() - 6, 6, "_first") == 0;
    const std::string what = n.substr(9, n.size() - 9 - (first ? 6 : 0));
    const xf_progress_metrics &m = first ? progress_first_ : progress_last_;
    XF_REQUIRE(progress_have_, "XFGetMetric: %s: no epoch has been summarised (progress=1, after "
               "XFStartTrain)", name);
    if (what == "logloss") *value = m.logloss;
    else if (what == "auc") *value = m.auc;
    else if (!first && what == "auc_slack") *value = m.auc_slack;
    else if (!first && what == "ctr") *value = m.ctr;
    else if (!first && what == "pctr") *value = m.pctr;
    else if (!first && what == "rows") *value = m.rows_pos + m.rows_neg;
    else
      return xf::set_error(XF_EINVAL, "XFGetMetric: unknown metric '%s'", name);
  } else if (n == "cross_in" || n == "cross_out") {
    uint64_t in = 0, crossed = 0;
    if (cross_) XF_TRY(xf_cross_stats(cross_, nullptr, &in, &crossed));
    *value = (double)(n == "cross_in" ? in : in + crossed);
  } else if (n == "norm_rows" || n == "norm_rows_scaled") {
    uint64_t rows = 0, scaled = 0;
    if (norm_) XF_TRY(xf_rownorm_stats(norm_, &rows, &scaled));
    *value = (double)(n == "norm_rows" ? rows : scaled);
  } else if (n == "admit_seen" || n == "admit_kept") {
    uint64_t seen = 0, kept = 0;
    if (admit_) XF_TRY(xf_admit_stats(admit_, &seen, &kept));
    *value = (double)(n == "admit_seen" ? seen : kept);
  } else if (n == "evict_seen") *value = (double)evict_seen_;
  else if (n == "evict_dropped") *value = (double)evict_dropped_;
  else if (n == "train_seconds") *value = train_seconds_;
  else if (n == "examples_per_sec") *value = train_seconds_ > 0 ? rows_trained_ / train_seconds_ : 0;
  else if (n == "keys") {
    uint64_t k = 0;
    if (table_w_) XF_TRY(xf_table_size(table_w_, &k));
    *value = (double)k;
  } else
    return xf::set_error(XF_EINVAL, "XFGetMetric: unknown metric '%s'", name);
  return XF_OK;
}

}  // namespace xflow_amd

// ------------------------------------------------------------------------------- C API
// c_api.h:26-41: the handle is an XFlow object owning the worker.
extern "C" int XFCreate(void **h, const char *train_path, const char *test_path) {
  XF_REQUIRE(h && train_path && test_path, "XFCreate: null argument");
  *h = new xflow_amd::Worker(0, train_path, test_path);
  return XF_OK;
}

extern "C" int XFStartTrain(void **h) {
  XF_REQUIRE(h && *h, "XFStartTrain: null handle");
  return reinterpret_cast<xflow_amd::Worker *>(*h)->train();
}

extern "C" int XFDestroy(void **h) {
  if (h && *h) {
    delete reinterpret_cast<xflow_amd::Worker *>(*h);
    *h = nullptr;
  }
  return XF_OK;
}

extern "C" int XFSetParam(void *h, const char *name, const char *value) {
  XF_REQUIRE(h, "XFSetParam: null handle");
  return reinterpret_cast<xflow_amd::Worker *>(h)->set_param(name, value);
}

extern "C" int XFGetMetric(void *h, const char *name, double *value) {
  XF_REQUIRE(h, "XFGetMetric: null handle");
  return reinterpret_cast<xflow_amd::Worker *>(h)->get_metric(name, value);
}

// ---- model file (xf_modelfile.cc; per shard and resharding on load when the worker is sharded)
extern "C" int XFSaveModel(void *h, const char *path) {
  XF_REQUIRE(h && path, "XFSaveModel: null argument");
  xflow_amd::Worker *wk = reinterpret_cast<xflow_amd::Worker *>(h);
  XF_REQUIRE(wk->table_w(), "XFSaveModel: nothing trained or loaded yet");
  return wk->save_model(path);
}

extern "C" int XFLoadModel(void *h, const char *path) {
  XF_REQUIRE(h && path, "XFLoadModel: null argument");
  xflow_amd::Worker *wk = reinterpret_cast<xflow_amd::Worker *>(h);
  XF_TRY(wk->ensure_tables());
  wk->note_external_keys();
  return wk->load_model(path);
}

// score the test file with the current tables (no training): predict + AUC/logloss
extern "C" int XFPredict(void *h) {
  XF_REQUIRE(h, "XFPredict: null handle");
  xflow_amd::Worker *wk = reinterpret_cast<xflow_amd::Worker *>(h);
  XF_TRY(wk->ensure_tables());
  return wk->predict(wk->rank, 0, wk->rank == 0);
}

extern "C" int XFGetTables(void *h, xf_table **w, xf_table **v) {
  XF_REQUIRE(h, "XFGetTables: null handle");
  xflow_amd::Worker *wk = reinterpret_cast<xflow_amd::Worker *>(h);
  if (w) *w = wk->table_w();
  if (v) *v = wk->table_v();
  return XF_OK;
}
