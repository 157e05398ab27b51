// xf_worker.h — the worker classes (see xf_worker.cc).
#ifndef XF_WORKER_H_
#define XF_WORKER_H_

#include <string>
#include <thread>
#include <vector>

#include "xf_common.h"

namespace xflow_amd {

// One class serves both models (model 0 = LRWorker, model 1 = FMWorker of the reference);
// LRWorker / FMWorker below keep the reference's constructor shape.
class Worker {
 public:
  Worker(int model, const char *train_file, const char *test_file);
  virtual ~Worker();

  int train();                       // lr_worker.cc:207-217
  int batch_training();              // lr_worker.cc:179-205
  int predict(int rank, int block, bool reader = true);  // lr_worker.cc:73-98

  int set_param(const char *name, const char *value);
  int get_metric(const char *name, double *value);
  int ensure_tables() { return create_tables(); }
  void note_external_keys() {}  // (the tables count their keys themselves)
  xf_table *table_w() { return table_w_; }
  xf_table *table_v() { return table_v_; }
  int save_model(const char *path);
  int load_model(const char *path);

 public:
  int epochs = 60;  // lr_worker.h:63

  // reference constants, now parameters
  int rank = 0;          // ps::MyRank(): given (rank=), from the environment, or handed out
  int world = 0;         // workers == GPUs; 0: WORLD_SIZE / XF_WORLD / DMLC_NUM_WORKER, else 1
  int transport = 0;                     // XF_TRANSPORT_*: RCCL; host = through the bootstrap sockets (tests)
  int schedule = XF_SCHEDULE_SEQUENTIAL; // order of Push(t) and Pull(t+1) when world > 1
  int core_num = 1;      // slices per block; 1 = the deterministic reference schedule
  int block_size = 2;    // MiB, lr_worker.h:68
  int v_dim_ = 10;       // fm_worker.h:92
  int optimizer = XF_OPT_FTRL;  // server.h:24,28
  uint64_t capacity = 1ull << 22;
  float alpha = 5e-2f, beta = 1.0f, lambda1 = 5e-5f, lambda2 = 10.0f;  // ftrl.h:17-20
  float learning_rate = 0.001f;                                       // sgd.h:16
  uint64_t seed = 0;
  int cache_batches = 1;
  bool key_build_gpu = true;  // key build of update() on the GPU (xf_batch_compile_gpu)
  int parity = 0;             // XF_PARITY_*: the forward's row sums (one worker)
  int fm_mode = 0;            // XF_FM_*: FM's second-order term (canonical, field_aware: one worker)
  int fields = 0;             // fm_mode = field_aware: field-group ids, 1 .. 64 (fgid in [0, fields))
  int v_width() const { return fm_mode == XF_FM_FIELD_AWARE ? fields * v_dim_ : v_dim_; }
  bool feature_values = false;  // a nonzero contributes x = val, not 1 (one worker)
  int update_rule = 0;        // XF_UPDATE_*: how an owner applies the workers' pushes of a step
  std::string pred_path;
  std::string model_in, model_out;  // load before / save after training (model file)
  // binarized block cache of the text files (xf_reader_open_cached): 0 = off; the cache
  // files go next to the data (<file>.xfcsr<cap>) or into block_cache_dir
  int block_cache = 0;
  std::string block_cache_dir;
  int open_reader(xf_reader **rd, const char *path, size_t cap, bool *writes_cache = nullptr);
  // ingest = gpu: the text of a block is tokenised and hashed on the GPU (xf_ingest.hip) and
  // compiled from device arrays; a block that is not of the common shape is parsed on the host
  // as before.  Needs core_num = 1 and no block cache (both checked where the epoch starts).
  bool ingest_gpu = false;
  // ingest = gpu_fields: the same epoch, and the tokeniser also reads what the model needs beside
  // the fid — field0 as fgid (fm_mode = field_aware), the third field as the value
  // (feature_values) — so those two modes train from text tokenised on the GPU; with neither it
  // is ingest = gpu
  bool ingest_fields = false;
  long blocks_gpu = 0, blocks_host = 0;  // how the blocks of the last training run were parsed
  // Feature admission (xf_admit.hip): admit_count = N >= 1: every block compiled from text goes
  // through a counting Bloom filter first (training: counted and filtered, predict: filtered) and a
  // key enters the tables only once the filter has seen it N times; 0 = off, nothing is created.
  // One worker, core_num 1, key_build=gpu, parity=exact (checked where training starts).  The
  // filter's seed is the worker's `seed`; its counters travel with the model as <model>.admit.
  int admit_count = 0;
  int admit_log2_slots = 26;  // 2^26 8-bit counters: 64 MiB
  int admit_hashes = 3;
  // admit_shared = 1: the ranks of a group share ONE filter (xf_admit_create_shared: the counters
  // sharded by slot range, every apply collective), which lifts "one worker"; every turn of the
  // training loop and of predict then applies on every rank — the empty minibatch where a rank has
  // no rows.  Not with the owner-compute schedules.  0: as before.
  int admit_shared = 0;
  // Negative subsampling (xf_negsample.hip): neg_keep = r < 1: every TRAINING block is sampled
  // first — every positive row kept, a negative row with probability r, decided by a hash of (seed,
  // (epoch << 32) | rank, the row's index in this rank's training file in this epoch) — then goes
  // through admission, when on, and into the matching _dev compile; the trainer multiplies a kept
  // negative's loss by 1 / r.  1 = off, nothing is created.  core_num 1, key_build=gpu,
  // parity=exact, not with the owner-compute schedules on several workers (checked where training
  // starts).  Stateless: nothing travels with the model.  Test blocks are never sampled.
  float neg_keep = 1.0f;
  // Feature crosses (xf_cross.hip): cross = "2*3,16*17": every block gains, behind each row's own
  // nonzeros, one nonzero per listed pair of fields and per (member, member), on the GPU — training:
  // after negative subsampling (which drops rows) and before admission (which must see the crossed
  // keys); predict: before admission.  Empty = off, nothing is created.  Every rank crosses its own
  // rows, on every schedule.  core_num 1, key_build=gpu, parity=exact, not ingest=gpu (checked where
  // training starts).  cross_fgid_base: the crossed nonzeros' fgids are base + the pair's index,
  // read only with fm_mode=field_aware (base + pairs <= fields).  Nothing travels with the model.
  std::string cross_spec;
  int cross_fgid_base = 0;
  // Row normalisation (xf_rownorm.hip): row_norm = l2: every minibatch of this rank's own rows —
  // training, the held part of holdout, predict — gets unit L2 length per row on the GPU.  The
  // LAST stage, immediately ahead of the key build: ingest, split, negsample, slices, cross,
  // admission, row norm, compile — over the nonzeros the model receives.  Off = nothing is
  // created.  Needs feature_values=on, core_num 1, key_build=gpu, parity=exact (checked where
  // training starts).  Nothing travels with the model: predict needs the same row_norm=.
  bool row_norm = false;
  // Progressive validation (xf_progress.hip): progress = 1: every training step counts its rows'
  // losses — formed under the weights the step is about to change — on the GPU, with no host wait
  // inside an epoch; at the end of each epoch (replayed ones included) the counts are read, merged
  // over the ranks and reset, and rank 0 prints one line.  A negative weighs the sampler's weight.
  // Not with the owner-compute schedules on several workers (checked where training starts).
  int progress = 0;
  // Sliced progressive validation (xf_slices.hip): progress_by = F (with progress = 1): every
  // TRAINING block's rows are named by the key of their first nonzero of field F — after negative
  // subsampling, which drops rows, and before the cross, so a slice is a value of an input field —
  // the ids travel with the compiled minibatch (replayed with it), and the trainer counts per
  // slice beside the progress.  At the end of each epoch rank 0 prints a summary line and the
  // progress_top slices by weighted rows, and appends a TSV line per slice to progress_slices_out.
  // core_num 1, key_build=gpu, parity=exact, not ingest=gpu (checked where training starts).
  // Nothing travels with the model.
  bool progress_by_set = false;
  long long progress_by = -1;
  int progress_slots = 16;
  int progress_top = 10;
  std::string progress_slices_out;
  // Table eviction (xf_evict.hip): evict_n = x > 0 (or inf): at the end of every evict_every-th
  // training epoch — in place of that boundary's defrag — and after the last one, ahead of
  // save_model and predict, every rank drops the keys of its shard whose w is 0 and whose n (the
  // sum of squared minibatch-mean gradients) is below x.  0 = off, nothing changes.  LR with FTRL
  // only, not with the owner-compute schedules on several workers (checked where training starts).
  float evict_n = 0.0f;
  int evict_every = 1;
  // Held-out validation (xf_holdout.hip): holdout = r in (0, 1): every TRAINING block is split
  // first — a row is held iff xf_holdout_held(seed, rank, the row's index in this rank's training
  // file, r): no epoch in the stream, so the SAME rows are held in every epoch — and only the train
  // part goes on to negative subsampling (which then numbers the rows of the train part: a second
  // running count), slices, cross, admission, compile and step.  The held part goes through the
  // cross and through admission with update = 0 (filtered, not counted, as test rows are), is
  // compiled with keep = 1 and stays in HBM for the whole run, whatever cache_batches says; an
  // epoch that reads the text again drops it.  After the flush of every holdout_every-th epoch
  // and of the last one the held list is scored forward-only (xf_sharded_validate), the counts are
  // merged over the ranks and rank 0 prints one line.  early_stop = P > 0: training ends after P
  // validated epochs without an improvement of the held-out logloss by more than early_stop_delta
  // (xf_holdout_should_stop); that epoch counts as the last one.  0 = off, nothing is created.
  // core_num 1, key_build=gpu, parity=exact, not with the owner-compute schedules on several
  // workers (checked where training starts).  Nothing travels with the model.
  float holdout = 0.0f;
  int holdout_every = 1;
  int early_stop = 0;
  double early_stop_delta = 0.0;
  // Grouped AUC on the held-out rows (xf_gauc.hip): holdout_by = F (with holdout > 0): the held
  // part's rows are named by the key of their first nonzero of field F as the split hands it over —
  // before the cross and admission, which neither add nor remove rows — and the ids stay with the
  // held minibatch.  Every validated epoch appends the held rows' records; after the holdout line
  // the records are reduced (merged on rank 0 over the ranks) and reset, rank 0 prints one line
  // and appends a TSV line per group to holdout_groups_out.  The early-stop rule keeps reading the
  // logloss.  core_num 1, key_build=gpu, not ingest=gpu (checked where training starts).  Nothing
  // travels with the model.
  bool holdout_by_set = false;
  long long holdout_by = -1;
  std::string holdout_groups_out;

 private:
  int check_gauc() const;  // the refusals of holdout_by, before any rendezvous
  int gauc_epoch(int epoch);  // COLLECTIVE at world > 1: reduce (merged), reset, summarise, print
  // the stage that names the held rows' groups (its own table is never fed); created with the split
  xf_slices *gslicer_ = nullptr;
  xf_gauc_metrics gauc_last_{};
  bool gauc_have_ = false;
  int check_holdout() const;  // the refusals of holdout / early_stop, before any rendezvous
  int create_holdout();
  // COLLECTIVE at world > 1: validate the held list, read, merge, reset, summarise, print; *stop:
  // the early-stop rule says this epoch is the last one
  int holdout_epoch(int epoch, bool last, bool *stop);
  xf_holdout *split_ = nullptr;     // holdout > 0: the split stage, created with the tables
  std::vector<xf_sbatch *> held_;   // the held parts of the first epoch's blocks, kept in HBM
  bool held_complete_ = false;      // the first epoch has ended: later splits drop the held part
  uint64_t train_ordinal_ = 0;      // rows of the train part so far in this epoch ...
  uint64_t train_block_first_ = 0;  // ... and before the block at hand: the sampler's first ordinal
  std::vector<double> holdout_curve_;  // the held-out logloss of every validated epoch ...
  std::vector<int> holdout_epochs_;    // ... and which epoch that was
  xf_progress_metrics holdout_last_{}, holdout_first_{};
  int epochs_run_ = 0;
  // split a training block (device arrays): the train part in the arguments, the held part in
  // pending_held_
  int split_dev(size_t first_row, const uint64_t **d_keys, const int32_t **d_fgid,
                const float **d_vals, const uint32_t **d_rowptr, const int32_t **d_labels,
                uint32_t *R, uint32_t *NNZ);
  int keep_held(const xf_holdout_part &held);
  xf_holdout_part pending_held_{};  // split_dev's held part, until the train part is compiled
  // ... or rows [start, end) of host arrays; then the train part's stages and compile
  int compile_split(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                    const int32_t *fgid, const float *vals, const int32_t *labels, size_t start,
                    size_t end, int keep);
  int check_evict() const;      // the refusals of evict_n, before any rendezvous
  int evict_epoch(int epoch);   // COLLECTIVE at world > 1: evict, sum the counts, print
  uint64_t evict_seen_ = 0, evict_dropped_ = 0;  // totals of the run, summed over the ranks
  int check_progress() const;  // the refusals of progress=1, before any rendezvous
  int progress_epoch(int epoch);  // COLLECTIVE at world > 1: read, merge, reset, summarise, print
  xf_progress_metrics progress_last_{}, progress_first_{};
  bool progress_have_ = false;
  int check_slices() const;  // the refusals of progress_by, before any rendezvous
  int slices_epoch(int epoch);  // COLLECTIVE at world > 1: read, merge, reset, summarise, print
  // the stage that names the rows' slices (its own table is never fed: the trainer owns the
  // counters, xf_sharded_slices); created with the tables
  xf_slices *slicer_ = nullptr;
  double slices_last_[4] = {0, 0, 0, 0};  // slices, rows, none rows, overflow rows of the last epoch
  bool slices_have_ = false;
  // rows [start, end) of host arrays with the feature on: the ids from the stage's own upload,
  // then the compile the block would have taken, then the ids onto the minibatch
  int compile_sliced(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                     const int32_t *fgid, const float *vals, const int32_t *labels, size_t start,
                     size_t end, int keep);
  int compile_rows_unsliced(xf_sharded *trainer, xf_sbatch **b, int update, const uint64_t *rowptr,
                            const uint64_t *keys, const int32_t *fgid, const float *vals,
                            const int32_t *labels, size_t start, size_t end, int keep);
  int create_tables();
  int defrag_if_grown(int percent);
  int any_rank(bool mine, bool *any);
  xf_admit *admit_ = nullptr;  // admit_count >= 1: the filter, created with the tables
  int check_admit() const;     // the refusals of admit_count >= 1, before any rendezvous
  int create_admit();
  xf_negsample *sample_ = nullptr;  // neg_keep < 1: the sampler, created with the tables
  uint64_t ordinal_ = 0;            // rows of this rank's training file read so far in this epoch
  uint64_t sample_stream_ = 0;      // (epoch << 32) | rank of the running epoch
  int check_negsample() const;      // the refusals of neg_keep, before any rendezvous
  int create_negsample();
  // sample a training block (device arrays, replaced in place by the sampler's; fgid / vals only
  // in the modes that read them), rows numbered from ordinal_ + first_row
  int sample_dev(size_t first_row, const uint64_t **d_keys, const int32_t **d_fgid,
                 const float **d_vals, const uint32_t **d_rowptr, const int32_t **d_labels,
                 uint32_t *R, uint32_t *NNZ);
  // ... or rows [start, end) of host arrays; then admission, when on, and the _dev compile.  A
  // block whose rows are all dropped is a block without rows: on one worker no minibatch
  // (*b = nullptr), in a group the empty minibatch
  int compile_sampled(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                      const int32_t *fgid, const float *vals, const int32_t *labels,
                      size_t start, size_t end, int keep);
  int compile_sampled_dev(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                          const float *d_vals, const uint32_t *d_rowptr, const int32_t *d_labels,
                          uint32_t R, uint32_t NNZ, int keep);
  xf_cross *cross_ = nullptr;  // cross=SPEC: the stage, created with the tables
  int check_cross() const;     // the refusals of cross, before any rendezvous
  int create_cross();
  // device arrays: the cross, when on, then admission, when on, then the _dev compile
  int compile_staged_dev(xf_sbatch **b, int update, const uint64_t *d_keys, const int32_t *d_fgid,
                         const float *d_vals, const uint32_t *d_rowptr, const int32_t *d_labels,
                         uint32_t R, uint32_t NNZ, int keep);
  // ... rows [start, end) of host arrays, uploaded by the cross
  int compile_crossed(xf_sbatch **b, int update, const uint64_t *rowptr, const uint64_t *keys,
                      const int32_t *fgid, const float *vals, const int32_t *labels, size_t start,
                      size_t end, int keep);
  // filter a block (host arrays and a row slice / device arrays), then the matching _dev compile
  int compile_admitted(xf_sbatch **b, int update, const uint64_t *rowptr, const uint64_t *keys,
                       const int32_t *fgid, const float *vals, const int32_t *labels,
                       size_t row_begin, size_t row_end, int keep);
  int compile_admitted_dev(xf_sbatch **b, int update, const uint64_t *d_keys,
                           const int32_t *d_fgid, const float *d_vals, const uint32_t *d_rowptr,
                           const int32_t *d_labels, uint32_t R, uint32_t NNZ, int keep);
  // the compile of the worker's mode: rows [start, end) of host arrays on `trainer` (admitted,
  // fielded, valued, plain, or — no rows — the empty minibatch), device arrays on sharded_
  int compile_rows(xf_sharded *trainer, xf_sbatch **b, int update, const uint64_t *rowptr,
                   const uint64_t *keys, const int32_t *fgid, const float *vals,
                   const int32_t *labels, size_t start, size_t end, int keep);
  int compile_no_rows(xf_sharded *trainer, xf_sbatch **b, int keep);
  int compile_dev_arrays(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                         const float *d_vals, const uint32_t *d_rowptr, const int32_t *d_labels,
                         uint32_t R, uint32_t NNZ, int keep);
  // ... compile_dev_arrays without row normalisation in front (the values are normalised already)
  int compile_dev_mode(xf_sbatch **b, const uint64_t *d_keys, const int32_t *d_fgid,
                       const float *d_vals, const uint32_t *d_rowptr, const int32_t *d_labels,
                       uint32_t R, uint32_t NNZ, int keep);
  xf_rownorm *norm_ = nullptr;  // row_norm=l2: the stage, created with the tables
  int check_rownorm() const;    // the refusals of row_norm, before any rendezvous
  int create_rownorm();
  // rows [start, end) of host arrays with no other stage on: uploaded by the stage, then the
  // _dev compile
  int compile_normed(xf_sbatch **b, const uint64_t *rowptr, const uint64_t *keys,
                     const int32_t *fgid, const float *vals, const int32_t *labels, size_t start,
                     size_t end, int keep);
  uint64_t keys_seen_ = 0;  // the table's keys at the last look (defrag_if_grown: the inflow per minibatch)
  bool rank_given_ = false;

  int model_;
  std::string train_file_path, test_file_path;
  char train_data_path[1200];
  char test_data_path[1200];
  xf_group *group_ = nullptr;      // ps-lite's postoffice: the other workers
  xf_sharded *sharded_ = nullptr;  // owns the tables; with one worker: the fused single shard
  xf_table *table_w_ = nullptr, *table_v_ = nullptr;  // kv_w_ / kv_v of the reference
  std::vector<xf_sbatch *> cache_;
  // the two block buffers that go round between the parser thread and the trainer: pinned host
  // memory, allocated once per worker (pinning and unpinning ~200 MB per epoch cost 30-80 ms)
  xf_block *blocks_[2] = {nullptr, nullptr};
  xf_ingest *ingest_[2] = {nullptr, nullptr};  // ingest = gpu: two staging / tokeniser buffers
  int start_ingest();                          // the buffers + first launches, before the clock
  bool gpu_ingest_applies() const;
  int set_ingest_fields(xf_ingest *g);         // the tokeniser's modes from fm_mode / feature_values
  int text_epoch(int epoch, int keep, bool *took);  // one epoch from the text, tokenised on the GPU
  std::vector<std::thread> closers_;  // readers being closed (munmap of the text) off the clock
  long rows_trained_ = 0;
  double train_seconds_ = 0.0;
  float logloss_acc_ = 0.0f, auc_ = 0.0f;
  double logloss_nat_ = 0.0;
  int tp_ = 0, fp_ = 0;
};

class LRWorker : public Worker {
 public:
  LRWorker(const char *train_file, const char *test_file) : Worker(0, train_file, test_file) {}
};

class FMWorker : public Worker {
 public:
  FMWorker(const char *train_file, const char *test_file) : Worker(1, train_file, test_file) {}
};

}  // namespace xflow_amd
#endif  // XF_WORKER_H_
